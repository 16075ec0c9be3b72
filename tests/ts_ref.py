"""Float64 numpy restatement of the series ops of the device augmentation stage (cn_augment_series_kernel of
cultionet_amd/csrc/cn_augment.hip: tswarp, tsnoise, tsdrift, tspeaks), without scipy and without torch: the GPU tests must
not need more than numpy. tests/test_ts_ref.py pins `halves` to F.interpolate and `apply_series` to what the reference's own
augment_time made of two samples (tests/golden/augment_series.npz); tests/test_series_augment_gpu.py holds the kernel to it.

  halves(v)                                               v [..., T] -> concat(resize(v, T // 2), resize(v, T - T // 2))
  apply_series(x, labels, op, pos, drift, nscale, seed)   x [C, T, H, W] in [0, 1], labels [H, W] -> [C, T, H, W] in [0, 1]
  identity_tables, hand_tables                            the tables the tests feed
"""
import numpy as np

from augment_ref import normal_noise

SERIES = ("tswarp", "tsnoise", "tsdrift", "tspeaks")
CODES = {"tswarp": 11, "tsnoise": 12, "tsdrift": 13, "tspeaks": 14}
SLOTS = 256


def resize_linear(v, n):
    """F.interpolate(v, size=n, mode="linear", align_corners=False) along the last axis."""
    T = v.shape[-1]
    s = np.maximum((np.arange(n) + 0.5) * (T / n) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), T - 1)
    i1 = np.minimum(i0 + 1, T - 1)
    lam = s - i0
    return (1.0 - lam) * v[..., i0] + lam * v[..., i1]


def halves(v):
    T = v.shape[-1]
    return np.concatenate((resize_linear(v, T // 2), resize_linear(v, T - T // 2)), axis=-1)


def apply_series(x, labels, op, pos, drift, nscale, seed):
    """The five steps of the device op in float64. pos [256, T], drift [256, C, T], nscale [256], indexed by label & 255."""
    x = np.asarray(x, dtype=np.float64)
    C, T, H, W = x.shape
    k = np.asarray(labels) & (SLOTS - 1)                                   # [H, W]
    assert pos.shape == (SLOTS, T) and drift.shape == (SLOTS, C, T) and nscale.shape == (SLOTS,)
    v = np.moveaxis(x, 1, -1)                                              # [C, H, W, T]
    u = np.where((k != 0)[None, :, :, None], halves(v), v) if op == "tspeaks" else v  # slot 0 is no prop: left alone
    if op in ("tswarp", "tspeaks"):
        p = np.asarray(pos, dtype=np.float64)[k][None]                     # [1, H, W, T]
        j = np.minimum(np.floor(p).astype(np.int64), T - 1)
        j1 = np.minimum(j + 1, T - 1)
        p, j, j1 = (np.broadcast_to(a, u.shape) for a in (p, j, j1))
        uj, uj1 = np.take_along_axis(u, j, -1), np.take_along_axis(u, j1, -1)
        w = uj + (p - j) * (uj1 - uj)
    else:
        w = u
    if op == "tsdrift":
        r = w.max(-1, keepdims=True) - w.min(-1, keepdims=True)
        d = w + np.moveaxis(np.asarray(drift, dtype=np.float64)[k], 2, 0) * r   # drift[k]: [H, W, C, T] -> [C, H, W, T]
    else:
        d = w
    r2 = d.max(-1, keepdims=True) - d.min(-1, keepdims=True)
    n = np.moveaxis(normal_noise(seed, x.size).reshape(C, T, H, W), 1, -1)      # element (c*T + t) * H*W + h*W + w
    ns = np.asarray(nscale, dtype=np.float64)[k][None, :, :, None]
    e = np.where(ns > 0, d + n * ns * r2, d)
    return np.moveaxis(np.clip(e, 0.0, 1.0), -1, 1)


# ---- tables ---------------------------------------------------------------------------------------------------------

def identity_tables(C, T):
    pos = np.tile(np.arange(T, dtype=np.float32), (SLOTS, 1))
    return pos, np.zeros((SLOTS, C, T), dtype=np.float32), np.zeros(SLOTS, dtype=np.float32)


def hand_tables(C, T, seed):
    """Monotone source times on and between integers that reach exactly T-1, drifts of both signs up to 0.1, noise
    scales 0 and 0.05; slot 0 the identity."""
    g = np.random.default_rng(seed)
    pos, drift, nscale = identity_tables(C, T)
    steps = g.random((SLOTS, T)) * g.integers(0, 2, (SLOTS, T))            # some steps are 0: repeated source times
    p = np.cumsum(steps, axis=1)
    p = p / np.maximum(p[:, -1:], 1e-9) * (T - 1)
    p[:, -1] = T - 1
    p[::3] = np.round(p[::3])                                              # every third slot sits on integers only
    p[5] = T - 1                                                           # a slot that reads the last time throughout
    pos[1:] = np.clip(np.maximum.accumulate(p, axis=1), 0, T - 1)[1:]
    drift[1:] = g.uniform(-0.1, 0.1, (SLOTS - 1, C, T))
    drift[1:, :, 0] = 0.1
    drift[1:, :, -1] = -0.1
    nscale[1::2] = 0.05
    assert pos.dtype == np.float32 and (np.diff(pos, axis=1) >= 0).all() and pos.max() == T - 1 and pos.min() == 0
    return pos, drift, nscale
