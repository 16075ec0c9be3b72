"""numpy restatement of the log transform of the device prologues (CnChipStore<true>, cultionet_amd/csrc/cn_chip_store.h;
EdgeDataset.get, data/datasets.py:481-484 of the reference: torch.log(x * 50.0 + 1.0).clamp_min(1e-9) between the
augmentation and the z-score), the tolerance the kernels are held to, and the log-domain form of tests/stats_ref.py.

For a value v that has been scaled, augmented and clipped to [lo, hi], in fp32 step by step:
    t = v * gain            one rounding
    u = t + 1               one rounding (no fma with the line above)
    w = max(log u, floor)   the logarithm in float64, rounded once to fp32
    out = (w - mean[c]) * (1 / std[c])
Nothing here reads a kernel's output. tests/test_log_transform_ref.py pins `log_w` to torch's own fp32 arithmetic.
"""
import numpy as np
import torch

import pointwise_ref as P
import stats_ref as S

F = np.float32
GAIN, FLOOR = 50.0, 1e-9


def ulp32(a):
    """The spacing of fp32 at |a| (float64 array)."""
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def log_w(v, gain=GAIN, floor=FLOOR):
    """v: float32, already in [lo, hi]. Returns (w32, w64, u): the fp32 result, the float64 value max(log u, floor) of the
    SAME fp32 u before its one rounding, and u."""
    v = np.asarray(v, dtype=np.float32)
    t = (v * F(gain)).astype(np.float32)
    u = (t + F(1)).astype(np.float32)
    l64 = np.log(u.astype(np.float64))
    w64 = np.maximum(l64, np.float64(F(floor)))
    w32 = np.fmax(l64.astype(np.float32), F(floor))
    return w32, w64, u


def _per_channel(a, ndim, C):
    return np.asarray(a, dtype=np.float32).reshape((1, C) + (1,) * (ndim - 2))


def log_zscore(v, mean, std, gain=GAIN, floor=FLOOR):
    """v: float32 [B][C][...] in [lo, hi]; mean / std: float32 [C] or None. Returns a dict:
    out  float32, the restatement's own result;
    z64  float64 (w64 - m) * inv with the kernel's fp32 m and fp32 reciprocal inv: what a kernel is compared with;
    tol  float64, |inv| (ulp32(w) + 0.5 ulp32(w - m)) + 0.5 ulp32(z): one ulp on w and half an ulp for each of the two
         roundings after it, each ulp taken at the far end of what the error before it allows; without mean and std the
         output is w itself and tol is ulp32(w);
    floor_at  bool, where u == 1: the output is exactly (fp32 floor - m) * inv there."""
    v = np.asarray(v, dtype=np.float32)
    C = v.shape[1]
    w32, w64, u = log_w(v, gain, floor)
    m = _per_channel(mean, v.ndim, C) if mean is not None else np.zeros((1, C) + (1,) * (v.ndim - 2), np.float32)
    inv = (F(1) / _per_channel(std, v.ndim, C)).astype(np.float32) if std is not None else np.ones_like(m)
    out = ((w32 - m).astype(np.float32) * inv).astype(np.float32)
    m64, inv64 = m.astype(np.float64), np.abs(inv.astype(np.float64))
    d64 = w64 - m64
    z64 = d64 * inv.astype(np.float64)
    e_w = ulp32(w64)
    e_d = e_w + 0.5 * ulp32(np.abs(d64) + e_w)
    tol = inv64 * e_d + 0.5 * ulp32(np.abs(z64) + inv64 * e_d)
    if mean is None and std is None:  # (w - 0) * 1 rounds nothing
        tol = e_w
    return {"out": out, "w32": w32, "w64": w64, "z64": z64, "tol": tol, "floor_at": u == F(1)}


def log_prepare_chips(x, mean, std, scale=1.0 / 10000.0, lo=1e-9, hi=1.0):
    """Raw x [B][C][...] (float32 / int32 / int16 / uint16) -> log_zscore of the prologue's v (pointwise_ref.prepare_chips_ref
    without a z-score: x.astype(f32) * f32(scale), clipped)."""
    return log_zscore(P.prepare_chips_ref(x, None, None, scale, lo, hi), mean, std)


def check(got, exp, what):
    """got: float32 array from a kernel; exp: a dict of log_zscore. Prints the worst err / tol before it asserts."""
    got = np.asarray(got, dtype=np.float32)
    assert got.shape == exp["z64"].shape, (what, got.shape, exp["z64"].shape)
    err = np.abs(got.astype(np.float64) - exp["z64"])
    ratio = float(np.max(err / exp["tol"]))
    at_floor = exp["floor_at"]
    nfloor = int((got[at_floor].view(np.uint32) != exp["out"][at_floor].view(np.uint32)).sum())
    print(f"LOG {what}: worst err / tol {ratio:.3f} over {got.size} values; {nfloor} of {int(at_floor.sum())} floor values "
          "differ in their bits")
    assert np.isfinite(got).all(), what
    assert ratio <= 1.0, f"{what}: err / tol {ratio}"
    assert nfloor == 0, f"{what}: {nfloor} values at u == 1 are not the floor exactly"


def fma_sensitive_bins(scale=1.0 / 10000.0):
    """The stored values k in 1..10000 at which a contracted fma(v, 50, 1) misses `tol` without a z-score (v = k *
    fp32(scale), the prologue's): the fused form lands on another fp32 u than the two roundings of t = v * 50 and
    u = t + 1 at 181 of the 10000 bins for scale = 1e-4, and at the 23 lowest of them (38, 39, 40, 61, ..., 305) one ulp
    of u is more than the two ulp of w the bound allows, by a factor of up to 3.5."""
    k = np.arange(1, 10001, dtype=np.float32)
    v = np.fmin(np.fmax((k * F(scale)).astype(np.float32), F(1e-9)), F(1))
    u_fused = (v.astype(np.float64) * GAIN + 1.0).astype(np.float32)  # the product is exact in float64: one rounding
    exp = log_zscore(v.reshape(1, 1, -1), None, None)
    w_fused = np.fmax(np.log(u_fused.astype(np.float64)).astype(np.float32), F(FLOOR)).astype(np.float64)
    return k[np.abs(w_fused - exp["z64"].reshape(-1)) > exp["tol"].reshape(-1)].astype(np.int64)


def corner_raw(shape, code, seed):
    """Random raw values of the type (codes of cn_prepare_chips_f32) with, in every channel of every sample, the corners
    of the clip, -32768, -1, 0, 1, 9999, 10000, 10001, 32767 (what the type cannot hold is left out), and the first eight
    fma_sensitive_bins, so that a contracted t, u shows in every plane."""
    rng = np.random.default_rng(seed)
    dt = {0: np.float32, 1: np.int32, 2: np.int16, 3: np.uint16}[code]
    lo = 0 if code == 3 else -300
    x = rng.integers(lo, 10300, shape).astype(dt)
    corners = [c for c in (-32768, -1, 0, 1, 9999, 10000, 10001, 32767) if code != 3 or c >= 0]
    corners += fma_sensitive_bins()[:8].tolist()
    flat = x.reshape(shape[0], shape[1], -1)
    for b in range(shape[0]):
        for c in range(shape[1]):
            at = rng.choice(flat.shape[2], len(corners), replace=False)
            flat[b, c, at] = np.array(corners).astype(dt)
    return flat.reshape(shape)


# ---- dataset statistics in the log domain (tests/stats_ref.py restated for what a log_transform dataset feeds) --------
def prepared_log(x_raw):
    """(x / 10000).clip(1e-9, 1) then torch.log(x * 50.0 + 1.0).clamp_min(1e-9), by torch in fp32 (data/datasets.py:443,
    481-484), rearranged 'b c t h w -> (b t h w) c' and widened to float64."""
    x = (torch.from_numpy(np.asarray(x_raw)).float() / 10000.0).clip(1e-9, 1)
    x = torch.log(x * 50.0 + 1.0).clamp_min(1e-9)
    return x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1]).double().numpy()


def dataset_stats_log(x_batches, centering="median", lower_quantile=0.05, upper_quantile=0.95):
    """stats_ref.dataset_stats over prepared_log: Variance(method='median') and the sketch's quantile rule in float64."""
    fed = [prepared_log(x) for x in x_batches]
    rows = np.concatenate(fed)
    q = S.sketch_quantiles(rows, [lower_quantile, 0.5, upper_quantile])
    return {"std": S.variance_median_std(fed), "mean": S.sketch_mean(rows) if centering == "mean" else q[:, 1],
            "lower_bound": q[:, 0], "upper_bound": q[:, 2]}
