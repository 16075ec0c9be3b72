"""The chip prologue (cn_prepare_chips_f32), the uint16 prediction writer (cn_predictions_to_u16) and the validation
metrics (cn_eval_metrics_f32) through the C ABI and through their Python wrappers, against the restatements of
tests/pointwise_ref.py and tests/metrics_ref.py (pinned on the CPU by tests/test_pointwise_ref.py and
tests/test_metrics_ref.py).

* The prologue and the writer are one IEEE fp32 operation per step, so they are held BIT-EQUAL to numpy (uint32 views /
  array_equal): all four input types, values on and next to the clip edges, +-0, +-inf and NaN, mean and std each on its
  own, both sides of every grid step and the capped grid.
* The metrics kernel is checked through its `counts` scratch as well as through `out`: the nine integer counts equal
  the restatement, the two double sums differ from the correctly rounded ones by the order of the additions only
  (n 2^-53 of the sum), and each fp32 output lies within half an fp32 ulp + n 2^-52 relative + 1e-12 of the float64
  restatement (metrics_ref.out_bound). `counts` is NaN before every call: the call's own memset has to clear it.

Every output lives in a NaN- or sentinel-filled buffer with slack behind it that must survive. Nothing here is fitted to
what the GPU returns. Run with -s to read the mismatch counts and err/bound ratios.
"""
import math

import numpy as np
import pytest
import torch

import metrics_ref as M
import pointwise_ref as R
from conv_exact_worker import Flat, lib, stream
from conv_exact_worker import dev as _dev

pytestmark = pytest.mark.gpu

NAN = float("nan")
F = np.float32
NP_DTYPES = {0: np.float32, 1: np.int32, 2: np.int16, 3: np.uint16}
SENT16 = -7776  # 57760 as uint16: no count reaches it


def _launches():
    return lib().query("cn_launch_count", 0)


# ---------------------------------------------------------------------------------------------------------------------
# cn_prepare_chips_f32
# ---------------------------------------------------------------------------------------------------------------------
PLANTED = {
    # on and next to the clip edges 1e-9 (raw 1e-5) and 1 (raw 10000), signed zeros, infinities, NaN, a denormal
    0: [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 10000.0, 10001.0, -1.0, 1e-5, np.nextafter(F(1e-5), F(0)),
        np.nextafter(F(1e-5), F(1)), np.nextafter(F(10000), F(0)), np.nextafter(F(10000), F(1e9)), 1e-40, 9999.5],
    1: [0, 1, 10000, 10001, -1, -10000, 9999, 2 ** 24 + 1, -(2 ** 24 + 1), 2 ** 24 + 3, 2 ** 31 - 1, -2 ** 31,
        2 ** 30 + 65, -(2 ** 30 + 65)],
    2: [0, 1, 10000, 10001, -1, -10000, 9999, -32768, 32767],
    3: [0, 1, 10000, 10001, 9999, 32767, 32768, 65535, 55536],
}


def _raw(code, shape, seed):
    """Random raw values of the type, with PLANTED spread over the whole buffer (first and last element included)."""
    rng = np.random.default_rng(seed)
    n = math.prod(shape)
    if code == 0:
        x = rng.normal(3000, 4000, n).astype(np.float32)
    elif code == 1:
        x = rng.integers(-50, 12000, n)
        far = rng.random(n) < 0.3
        x[far] = rng.integers(-2 ** 31, 2 ** 31, n)[far]
        x = x.astype(np.int32)
    elif code == 2:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
    else:
        x = rng.integers(0, 65536, n).astype(np.uint16)
    k = min(len(PLANTED[code]), n)
    x[np.linspace(0, n - 1, k).astype(np.int64)] = np.array(PLANTED[code][:k]).astype(NP_DTYPES[code])
    if n >= 1000:
        if code == 1:
            assert (np.abs(x.astype(np.int64)) > 2 ** 24).any()
        if code == 2:
            assert (x < 0).any()
        if code == 3:
            assert (x > 32767).any()
    return x.reshape(shape)


def _to_dev(x):
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(_dev())


def _prepare(code, x, mean, std, scale, lo, hi, what):
    """One call on a NaN-filled output; bit-equal to prepare_chips_ref."""
    dev, L = _dev(), lib()
    B, C, Ln = x.shape
    want = R.prepare_chips_ref(x, mean, std, scale, lo, hi)
    xd = _to_dev(x)
    md = None if mean is None else torch.from_numpy(mean).to(dev)
    sd = None if std is None else torch.from_numpy(std).to(dev)
    out = Flat(x.shape, dev)
    L.call("cn_prepare_chips_f32", xd.data_ptr(), code, out.ptr, None if md is None else md.data_ptr(),
           None if sd is None else sd.data_ptr(), B, C, Ln, scale, lo, hi, stream())
    torch.cuda.synchronize()
    got = out.t.cpu().numpy()
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"EXACT {what}: {bad} of {want.size} values differ in their bits")
    assert bad == 0, f"{what}: {bad} of {want.size} values differ"
    assert np.isfinite(want).all()  # clipping leaves nothing non-finite, whatever came in
    out.assert_slack(what)


def _stats(C, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(C) * 0.5).astype(np.float32), (rng.random(C) * 0.3 + 0.02).astype(np.float32)


# (B, C, L): the smallest L; either side of the one-block / two-block step (a block covers 1024 values); the capped grid
# (1025 blocks wanted, 1024 launched: some threads loop five times)
PREP_SHAPES = [(3, 4, 1), (2, 3, 1023), (2, 3, 1025), (1, 2, 1024 * 1024 + 300)]


@pytest.mark.parametrize("code", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", PREP_SHAPES)
def test_prepare_chips_f32_bit_exact(code, shape):
    """All four type codes (int16 with negatives, uint16 above 32767, int32 beyond +-2^24, fp32 with +-0, +-inf, NaN and
    a denormal), values on and next to both clip edges, and mean only, std only, both and neither, at the prologue's
    constants (scale 1e-4, clip to [1e-9, 1])."""
    B, C, Ln = shape
    if Ln > 1 << 20:
        bx = (Ln + 1023) // 1024
        assert bx > 1024 and Ln > 4 * 1024 * 256
    x = _raw(code, shape, 100 + code)
    mean, std = _stats(C, 7 + C)
    for name, m, s in (("mean and std", mean, std), ("mean only", mean, None), ("std only", None, std),
                       ("no z-score", None, None)):
        _prepare(code, x, m, s, 1.0 / 10000.0, 1e-9, 1.0, f"prepare_chips code {code} {shape} {name}")


def test_prepare_chips_f32_int32_conversion_rounds_to_nearest_even():
    """Scale 2^-31 and a clip to [-1, 1] keep every int32 inside the clip, so the int32 -> fp32 conversion of values
    beyond +-2^24 (round to nearest, ties to even) reaches the output."""
    x = _raw(1, (2, 3, 1025), 120)
    ties = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 31 - 1, 2 ** 31 - 64,
                     2 ** 31 - 65], dtype=np.int64)
    x.reshape(-1)[100:100 + ties.size] = ties.astype(np.int32)
    mean, std = _stats(3, 9)
    _prepare(1, x, mean, std, 2.0 ** -31, -1.0, 1.0, "prepare_chips int32 conversion")


def test_prepare_chips_f32_empty_and_unknown_type():
    """B = 0 and L = 0 return OK and leave the output alone; type code 4 is an argument error, nothing written."""
    dev, L, st = _dev(), lib(), stream()
    x = torch.zeros(64, device=dev)
    m = torch.ones(4, device=dev)
    out = Flat((64,), dev)
    L.call("cn_prepare_chips_f32", x.data_ptr(), 0, out.ptr, m.data_ptr(), m.data_ptr(), 0, 4, 16, 1e-4, 1e-9, 1.0, st)
    L.call("cn_prepare_chips_f32", x.data_ptr(), 2, out.ptr, m.data_ptr(), m.data_ptr(), 1, 4, 0, 1e-4, 1e-9, 1.0, st)
    with pytest.raises(L.HipKernelError):
        L.call("cn_prepare_chips_f32", x.data_ptr(), 4, out.ptr, m.data_ptr(), m.data_ptr(), 1, 4, 16, 1e-4, 1e-9, 1.0,
               st)
    with pytest.raises(L.HipKernelError):
        L.call("cn_prepare_chips_f32", x.data_ptr(), -1, out.ptr, None, None, 1, 4, 16, 1e-4, 1e-9, 1.0, st)
    torch.cuda.synchronize()
    assert bool(out.buf.isnan().all()), "an empty or refused call wrote to the output"


@pytest.mark.parametrize("dtype", [torch.int16, torch.uint16, torch.int32, torch.float32])
def test_prepare_chips_wrapper_bit_exact(dtype):
    """edges.prepare_chips on [B, C, T, H, W]: the type code it picks, L = T*H*W, mean / std of any shape holding C
    values and each optional on its own."""
    from cultionet_amd.edges import prepare_chips

    code = {torch.float32: 0, torch.int32: 1, torch.int16: 2, torch.uint16: 3}[dtype]
    B, C, T, H, W = 2, 3, 5, 7, 9
    x = _raw(code, (B, C, T * H * W), 130 + code)
    mean, std = _stats(C, 11)
    xd = _to_dev(x).view(B, C, T, H, W)
    if code == 3:
        xd = xd.view(torch.uint16)
    assert xd.dtype == dtype
    for m, s in ((mean, std), (mean, None), (None, std), (None, None)):
        mt = None if m is None else torch.from_numpy(m).view(1, C, 1, 1, 1)  # as NormValues stores them
        st_ = None if s is None else torch.from_numpy(s)
        got = prepare_chips(xd, mt, st_).cpu().numpy()
        want = R.prepare_chips_ref(x, m, s, 1.0 / 10000.0, 1e-9, 1.0).reshape(B, C, T, H, W)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_prepare_chips_wrapper_refuses_statistics_of_the_wrong_length():
    """A mean or std that does not hold exactly C values is a ValueError before any launch (the kernel would index it
    by channel, past its end)."""
    from cultionet_amd.edges import prepare_chips

    x = torch.zeros(2, 4, 3, 5, 5, dtype=torch.int16, device=_dev())
    good = torch.ones(4)
    for mean, std in ((good, torch.ones(3)), (good, torch.ones(1)), (None, torch.ones(5)), (torch.ones(3), good),
                      (good, torch.ones(2, 4))):
        before = _launches()
        with pytest.raises(ValueError):
            prepare_chips(x, mean, std)
        assert _launches() == before, "a kernel was launched before the check"
    before = _launches()
    prepare_chips(x, good, good.view(1, 4, 1, 1, 1))
    assert _launches() == before + 1  # the counter does move for a valid call


# ---------------------------------------------------------------------------------------------------------------------
# cn_predictions_to_u16
# ---------------------------------------------------------------------------------------------------------------------
# H, W, pad_top, pad_left, h, w
U16_CASES = [
    (40, 44, 4, 4, 32, 36),        # the standard window
    (16, 16, 0, 0, 16, 16),        # no padding, h*w = 256: exactly one block
    (17, 19, 3, 5, 14, 14),        # unequal pads, the last row and column reached exactly, a ragged last block
    (9, 300, 1, 2, 1, 257),        # a single row across a block boundary
]
SPECIALS = (np.nan, -0.25, 1.5, 7.0)


def _maps(B, H, W, pt, pl, h, w, seed):
    """Three different [B][1][H][W] maps of probabilities on and next to integer counts, with NaN, -0.25, 1.5 and 7.0
    planted inside every sample's window."""
    maps = []
    for k in range(3):
        v = R.count_neighbours(B * H * W, seed + k).reshape(B, 1, H, W)
        for b in range(B):
            for j, s in enumerate(SPECIALS):
                i = (37 * b + 11 * k + 5 * j) % (h * w)
                v[b, 0, pt + i // w, pl + i % w] = s
        maps.append(v)
    return maps


@pytest.mark.parametrize("H,W,pt,pl,h,w", U16_CASES)
def test_predictions_to_u16_bit_exact(H, W, pt, pl, h, w):
    """array_equal to predictions_u16_ref: B = 3 and three different maps, so a swapped map or sample shows."""
    dev, L = _dev(), lib()
    B = 3
    assert pt + h <= H and pl + w <= W
    if (H, W) == (17, 19):
        assert pt + h == H and pl + w == W and pt != pl and (h * w) % 256 != 0
    maps = _maps(B, H, W, pt, pl, h, w, 200 + H)
    want = R.predictions_u16_ref(maps[0], maps[1], maps[2], pt, pl, h, w, 10000.0)
    assert (want == 10000).any() and (want == 0).any()
    assert not np.array_equal(want[:, 0], want[:, 1]) and not np.array_equal(want[0], want[1])
    md = [torch.from_numpy(m).to(dev) for m in maps]
    out = Flat((B, 3, h, w), dev, fill=SENT16, dtype=torch.int16)
    L.call("cn_predictions_to_u16", md[0].data_ptr(), md[1].data_ptr(), md[2].data_ptr(), out.ptr, B, H, W, pt, pl, h, w,
           10000.0, stream())
    torch.cuda.synchronize()
    got = out.t.cpu().numpy().view(np.uint16)
    bad = int((got != want).sum())
    print(f"EXACT predictions_to_u16 {H}x{W} pads {pt},{pl} window {h}x{w}: {bad} of {want.size} counts differ")
    assert np.array_equal(got, want), f"{bad} of {want.size} counts differ"
    out.assert_slack("counts")


def test_predictions_to_u16_refuses_windows_outside_the_map():
    """pad_top + h = H + 1, pad_left + w = W + 1 and a negative pad are argument errors; nothing is written."""
    dev, L, st = _dev(), lib(), stream()
    B, H, W, h, w = 3, 40, 44, 32, 36
    m = torch.rand(B, 1, H, W, device=dev)
    out = Flat((B, 3, h, w), dev, fill=SENT16, dtype=torch.int16)
    for pt, pl in ((H + 1 - h, 4), (4, W + 1 - w), (-1, 4), (4, -1)):
        with pytest.raises(L.HipKernelError):
            L.call("cn_predictions_to_u16", m.data_ptr(), m.data_ptr(), m.data_ptr(), out.ptr, B, H, W, pt, pl, h, w,
                   10000.0, st)
    torch.cuda.synchronize()
    assert bool((out.buf == SENT16).all()), "a refused call wrote to the output"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_predictions_to_uint16_wrapper(dtype):
    """edges.predictions_to_uint16 on fp32 and on bf16 maps (the bf16-mixed forward's): equal to predictions_u16_ref of
    the values widened to fp32. The edge map is a non-contiguous view."""
    from cultionet_amd.edges import predictions_to_uint16

    dev = _dev()
    B, H, W, pad, h, w = 3, 40, 44, 4, 32, 36
    maps = [torch.from_numpy(m).to(dtype) for m in _maps(B, H, W, pad, pad, h, w, 260)]
    want = R.predictions_u16_ref(*(m.float().numpy() for m in maps), pad, pad, h, w, 10000.0)
    wide = torch.full((B, 3, H, W), 0.5, dtype=dtype)
    wide[:, 1:2] = maps[1]
    edge = wide.to(dev)[:, 1:2]
    assert not edge.is_contiguous()
    got = predictions_to_uint16({"distance": maps[0].to(dev), "edge": edge, "crop": maps[2].to(dev)}, pad, h, w)
    assert got.dtype == torch.uint16 and got.shape == (B, 3, h, w)
    assert np.array_equal(got.cpu().numpy(), want), f"{int((got.cpu().numpy() != want).sum())} of {want.size} differ"
    if dtype == torch.bfloat16:  # read as fp32 the bf16 buffer would give other counts
        assert not np.array_equal(want, R.predictions_u16_ref(*_maps(B, H, W, pad, pad, h, w, 260), pad, pad, h, w, 1e4))


def test_predictions_to_uint16_wrapper_refuses_bad_maps():
    """CPU maps, maps of different shapes, a channel dimension that is not 1, and a window that does not fit are
    ValueErrors before any launch: the kernel never sees them."""
    from cultionet_amd.edges import predictions_to_uint16

    dev = _dev()
    B, H, W = 2, 20, 24
    ok = lambda: torch.rand(B, 1, H, W, device=dev)
    pred = lambda **kw: {**{k: ok() for k in ("distance", "edge", "crop")}, **kw}
    bad = [
        (pred(edge=torch.rand(B, 1, H, W)), 2, 16, 20),                          # a CPU tensor
        ({k: torch.rand(B, 1, H, W) for k in ("distance", "edge", "crop")}, 2, 16, 20),
        (pred(crop=torch.rand(B, 1, H, W + 1, device=dev)), 2, 16, 20),          # shapes differ
        (pred(edge=torch.rand(B + 1, 1, H, W, device=dev)), 2, 16, 20),
        ({k: torch.rand(B, 2, H, W, device=dev) for k in ("distance", "edge", "crop")}, 2, 16, 20),  # channels
        (pred(), 2, H - 1, 20),                                                   # padding + height = H + 1
        (pred(), 2, 16, W - 1),                                                   # padding + width = W + 1
        (pred(), -1, 16, 20),
    ]
    for p, pad, h, w in bad:
        before = _launches()
        with pytest.raises(ValueError):
            predictions_to_uint16(p, pad, h, w)
        assert _launches() == before, "a kernel was launched before the check"
    before = _launches()
    predictions_to_uint16(pred(), 2, H - 2, W - 2)  # the largest window that fits
    assert _launches() == before + 1


# ---------------------------------------------------------------------------------------------------------------------
# cn_eval_metrics_f32
# ---------------------------------------------------------------------------------------------------------------------
LOSS = F(0.625)


def _metric_inputs(n, seed, lo=-1, hi=3):
    """dist, edge, crop, bdist ~ U[0, 1) and labels in lo..hi."""
    rng = np.random.default_rng(seed)
    dist, edge, crop, bdist = (rng.random(n, dtype=np.float32) for _ in range(4))
    return dist, edge, crop, bdist, rng.integers(lo, hi + 1, n)


def _metrics(dist, edge, crop, bdist, y, klass, thresh, n=None):
    """One call with `counts` and `out` NaN beforehand; returns counts (float64 [11]) and out (float32 [7])."""
    dev, L = _dev(), lib()
    d = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1)).to(dev) for a in (dist, edge, crop, bdist)]
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.int64).reshape(-1)).to(dev)
    ld = torch.tensor([float(LOSS)], device=dev)
    counts = Flat((11,), dev, dtype=torch.float64)
    out = Flat((7,), dev)
    assert bool(counts.buf.isnan().all())
    L.call("cn_eval_metrics_f32", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), yd.data_ptr(),
           klass, thresh, yd.numel() if n is None else n, ld.data_ptr(), counts.ptr, out.ptr, stream())
    torch.cuda.synchronize()
    counts.assert_slack("counts")
    out.assert_slack("out")
    return counts.t.cpu().numpy(), out.t.cpu().numpy()


INTEGER_COUNTS = [0, 3, 4, 5, 6, 7, 8, 9, 10]


def _check_metrics(what, counts, out, ref_c, n):
    """counts and out against the restatement of the same inputs; returns the restated outputs."""
    ref_o = M.eval_metrics_ref(ref_c, float(LOSS))
    assert np.array_equal(counts[INTEGER_COUNTS], ref_c[INTEGER_COUNTS]), \
        f"{what}: counts {dict(zip(M.NAMES, counts))}, want {dict(zip(M.NAMES, ref_c))}"
    worst_c = 0.0
    for k in (1, 2):
        if math.isnan(ref_c[k]):
            assert math.isnan(counts[k]), f"{what}: {M.NAMES[k]} = {counts[k]}, want NaN"
            continue
        bound = n * 2.0 ** -53 * ref_c[k]  # every term is exact and not negative: only the order of the sum differs
        err = abs(counts[k] - ref_c[k])
        assert err <= bound, f"{what}: {M.NAMES[k]} off by {err:.3e}, bound {bound:.3e}"
        worst_c = max(worst_c, err / bound if bound > 0 else 0.0)
    nan = np.isnan(ref_o)
    assert np.array_equal(np.isnan(out), nan), f"{what}: out {out}, want {ref_o}"
    err = np.abs(out.astype(np.float64) - ref_o)[~nan]
    ratio = err / M.out_bound(ref_o[~nan], n)
    print(f"BOUND {what}: sums worst err/bound {worst_c:.1e}, out worst err/bound {float(ratio.max()):.3f}")
    assert (ratio <= 1.0).all(), f"{what}: out {dict(zip(M.OUT_NAMES, out))}, want {dict(zip(M.OUT_NAMES, ref_o))}"
    return ref_o


# n = 1; either side of the one-block / two-block step; the capped grid (1024 blocks, every thread loops twice)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1024 * 256 + 777])
@pytest.mark.parametrize("klass", [2, 3])
def test_eval_metrics_f32_counts_and_outputs(n, klass):
    """Labels in -1..3: with klass = 2 a label 3 is neither edge nor crop."""
    if n > 1 << 18:
        assert (n + 255) // 256 > 1024 and n > 1024 * 256
    dist, edge, crop, bdist, y = _metric_inputs(n, 300 + n % 1000 + klass)
    if n == 1:
        y[0] = klass
    if n > 100:
        assert set(np.unique(y).tolist()) == {-1, 0, 1, 2, 3}
    ref_c = M.eval_counts_ref(dist, edge, crop, bdist, y, klass, 0.5)
    counts, out = _metrics(dist, edge, crop, bdist, y, klass, 0.5)
    _check_metrics(f"eval metrics n={n} klass={klass}", counts, out, ref_c, n)
    if n > 100 and klass == 2:  # the case can tell klass apart
        assert not np.array_equal(ref_c, M.eval_counts_ref(dist, edge, crop, bdist, y, 3, 0.5))


@pytest.mark.parametrize("thresh", [0.5, 0.3])
def test_eval_metrics_f32_positive_means_strictly_greater(thresh):
    """Three dozen edge and crop probabilities exactly at the threshold and at its two fp32 neighbours, under every
    valid label. 0.3 is not an fp32 number: the kernel and the restatement both compare with fp32(0.3)."""
    n, klass = 1000, 2
    dist, edge, crop, bdist, y = _metric_inputs(n, 320, hi=2)
    t = F(thresh)
    trio = [np.nextafter(t, F(0)), t, np.nextafter(t, F(1))]
    at = np.arange(36) * 27 + 3
    for j, i in enumerate(at):
        edge[i], crop[i + 1] = trio[j % 3], trio[(j + 1) % 3]
        y[i], y[i + 1] = j % 3, (j // 3) % 3
    ref_c = M.eval_counts_ref(dist, edge, crop, bdist, y, klass, thresh)
    # a kernel comparing with >= would count these as positive
    valid = y != -1
    assert int((valid & (edge == t)).sum()) >= 12 and int((valid & (crop == t)).sum()) >= 12
    counts, out = _metrics(dist, edge, crop, bdist, y, klass, thresh)
    _check_metrics(f"eval metrics at the threshold {thresh}", counts, out, ref_c, n)


def _plant_nans(arrays, at):
    """NaN into dist, bdist, edge and crop in turn (and all four at every fifth position)."""
    out = [a.copy() for a in arrays]
    for j, i in enumerate(at):
        for k in range(4):
            if j % 5 == 4 or j % 5 == k:
                out[k][i] = np.nan
    return out


def test_eval_metrics_f32_skips_nans_under_masked_labels():
    """NaN in dist / bdist / edge / crop at pixels labelled -1: all 7 outputs stay finite and equal, bit for bit, those
    of the NaN-free run (a kernel multiplying by the mask would turn 0 * NaN into NaN)."""
    n, klass = 700, 2  # three blocks add their partial sums atomically, in an order that changes from run to run
    dist, edge, crop, bdist, y = M.grid_inputs(n, 330, hi=2)
    at = np.arange(40) * 17 + 5
    y[at] = -1
    M.grid_premise(dist, bdist, y)  # the two real sums are exact in any order: equality of two runs is a theorem
    clean_c, clean_o = _metrics(dist, edge, crop, bdist, y, klass, 0.5)
    nd, nb, ne, nc = _plant_nans((dist, bdist, edge, crop), at)
    assert all(np.isnan(a).sum() >= 16 for a in (nd, nb, ne, nc))
    M.grid_premise(nd, nb, y)
    counts, out = _metrics(nd, ne, nc, nb, y, klass, 0.5)
    ref_c = M.eval_counts_ref(nd, ne, nc, nb, y, klass, 0.5)
    _check_metrics("eval metrics NaN under masked labels", counts, out, ref_c, n)
    assert np.isfinite(out).all() and np.isfinite(counts).all()
    assert np.array_equal(counts, clean_c) and np.array_equal(out.view(np.uint32), clean_o.view(np.uint32))


def test_eval_metrics_f32_nans_at_valid_pixels():
    """The same NaNs at valid pixels whose edge / crop probabilities were below the threshold: MAE, MSE and the score
    are NaN, the eight confusion counts are those of the NaN-free run (a NaN is not greater than the threshold). NaN in
    edge / crop alone changes nothing."""
    n, klass = 700, 3
    dist, edge, crop, bdist, y = _metric_inputs(n, 340)
    at = np.arange(10) * 61 + 7
    y[at] = np.arange(10) % 4
    edge[at], crop[at] = F(0.25), F(0.125)
    clean_c, clean_o = _metrics(dist, edge, crop, bdist, y, klass, 0.5)
    ref_c = M.eval_counts_ref(dist, edge, crop, bdist, y, klass, 0.5)
    _check_metrics("eval metrics before the NaNs", clean_c, clean_o, ref_c, n)
    nd, nb, ne, nc = _plant_nans((dist, bdist, edge, crop), at)
    counts, out = _metrics(nd, ne, nc, nb, y, klass, 0.5)
    ref_c = M.eval_counts_ref(nd, ne, nc, nb, y, klass, 0.5)
    _check_metrics("eval metrics NaN at valid pixels", counts, out, ref_c, n)
    assert np.isnan(out[[0, 1, 6]]).all() and np.isfinite(out[2:6]).all()
    assert np.array_equal(counts[INTEGER_COUNTS], clean_c[INTEGER_COUNTS])
    # two runs are compared bit for bit on grid inputs only: there the sums do not depend on the order of the atomics
    dist, _, _, bdist, _ = M.grid_inputs(n, 341)
    M.grid_premise(dist, bdist, y)
    clean_c, clean_o = _metrics(dist, edge, crop, bdist, y, klass, 0.5)
    counts, out = _metrics(dist, ne, nc, bdist, y, klass, 0.5)
    assert np.array_equal(counts, clean_c) and np.array_equal(out.view(np.uint32), clean_o.view(np.uint32))


# n = 257: two blocks; the capped grid: 1024 blocks race on the atomics and every thread loops twice
@pytest.mark.parametrize("n", [257, 1024 * 256 + 777])
@pytest.mark.parametrize("klass", [2, 3])
def test_eval_metrics_f32_grid_inputs_equal_the_restatement(n, klass):
    """dist and bdist on the grid k / 1024 (metrics_ref.grid_inputs): every |d| and d^2 and every partial sum of them is
    exact in double (grid_premise asserts it), so the kernel's sums cannot depend on the order of its additions and
    ALL ELEVEN counts must EQUAL the float64 restatement -- the two real sums included, which random inputs only bound
    by n 2^-53. The seven outputs stay within metrics_ref.out_bound."""
    if n > 1 << 18:
        assert (n + 255) // 256 > 1024 and n > 1024 * 256
    dist, edge, crop, bdist, y = M.grid_inputs(n, 360 + n % 1000 + klass)
    assert set(np.unique(y).tolist()) == {-1, 0, 1, 2, 3}
    M.grid_premise(dist, bdist, y)
    ref_c = M.eval_counts_ref(dist, edge, crop, bdist, y, klass, 0.5)
    assert ref_c[1] > 0 and ref_c[2] > 0 and ref_c[1] != ref_c[2]
    counts, out = _metrics(dist, edge, crop, bdist, y, klass, 0.5)
    print(f"EXACT eval metrics on the grid n={n} klass={klass}: {int((counts != ref_c).sum())} of 11 counts differ")
    assert np.array_equal(counts, ref_c), f"counts {dict(zip(M.NAMES, counts))}, want {dict(zip(M.NAMES, ref_c))}"
    _check_metrics(f"eval metrics on the grid n={n} klass={klass}", counts, out, ref_c, n)


def test_eval_metrics_f32_all_masked_and_empty():
    """Every label -1, and n = 0 passed: the counts are zero (cleared by the call), n -> 1, MAE = MSE = F = 0, the MCC
    takes its eps branch (0), score = loss + 4; the finalize kernel writes `out` in both cases."""
    n = 300
    dist, edge, crop, bdist, y = _metric_inputs(n, 350)
    masked = np.full(n, -1)
    ref_c = M.eval_counts_ref(dist, edge, crop, bdist, masked, 2, 0.5)
    assert not ref_c.any()
    for what, labels, n_arg in (("all masked", masked, None), ("n = 0", y, 0)):
        counts, out = _metrics(dist, edge, crop, bdist, labels, 2, 0.5, n=n_arg)
        ref_o = _check_metrics("eval metrics " + what, counts, out, ref_c, n)
        assert not counts.any() and ref_o.tolist() == [0, 0, 0, 0, 0, 0, float(LOSS) + 4.0]
        assert out.tolist() == [0, 0, 0, 0, 0, 0, 4.625]


@pytest.mark.parametrize("klass", [2, 3])
def test_eval_metrics_f32_degenerate_confusion_matrices(klass):
    """The random and degenerate cases of test_eval_metrics_kernel_against_restatement (metrics_ref.eval_cases; each is
    shown to reach its branch by tests/test_metrics_ref.py), at both edge classes."""
    for name, dist, edge, crop, bdist, y in M.eval_cases(klass):
        ref_c = M.eval_counts_ref(dist, edge, crop, bdist, y, klass, 0.5)
        counts, out = _metrics(dist, edge, crop, bdist, y, klass, 0.5)
        ref_o = _check_metrics(f"eval metrics klass={klass} {name}", counts, out, ref_c, y.size)
        if name == "edge all right, crop all wrong":
            assert out[4] == 1.0 and out[5] == -1.0 and ref_o[4] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the Lightning route: validation_step -> cn_eval_metrics_f32
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed"])
@pytest.mark.parametrize("edge_class", [2, 3])
def test_validation_step_hands_the_maps_and_the_edge_class_to_the_kernel(edge_class, precision):
    """One validation_step at hidden 8, B = 2, 28 x 28, some labels -1. The eval forward is bit-reproducible
    (test_forward_is_bit_reproducible), so a second forward gives the maps the step saw: widened with .float() and fed,
    with the step's own val_loss, to the float64 restatement they must give vef1, vcf1, vmae and val_score within the
    kernel's bound -- whatever the model's precision and memory layout, and for the module's own edge class."""
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel

    dev = _dev()
    B, H, W = 2, 28, 28
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0, edge_class=edge_class)
    model = lit.cultionet_model.mask_model
    model.load_state_dict(S.seeded_state_dict(model.state_dict()))
    lit = lit.to(dev).eval()
    lit.hip_precision = precision
    x, _, bdist = S.seeded_batch(B, height=H, width=W, seed=11)
    y = torch.randint(-1, edge_class + 1, (B, H, W), generator=torch.Generator().manual_seed(12))
    assert set(y.unique().tolist()) == set(range(-1, edge_class + 1))
    batch = Data(x=x.to(dev), y=y.to(dev), bdist=bdist.to(dev), lon=torch.zeros(B, device=dev),
                 lat=torch.zeros(B, device=dev))
    with torch.no_grad():
        lit(batch)
        met = {k: float(v) for k, v in lit.validation_step(batch).items()}  # read before anything else runs
        pred = lit(batch)
        maps = [pred[k].clone() for k in ("distance", "edge", "crop")]
        if precision == "bf16-mixed":  # the mixed-precision forward really ran
            lit.hip_precision = "32-true"
            assert not torch.equal(lit(batch)["edge"].float(), maps[1].float())
    d, e, c = (m.float().cpu().numpy() for m in maps)
    n = y.numel()
    ref_c = M.eval_counts_ref(d, e, c, bdist.numpy(), y.numpy(), edge_class, 0.5)
    ref_o = M.eval_metrics_ref(ref_c, float(met["val_loss"]))
    got = np.array([float(met[k]) for k in ("vmae", "vef1", "vcf1", "val_score")])
    want = ref_o[[0, 2, 3, 6]]
    ratio = np.abs(got - want) / M.out_bound(want, n)
    print(f"BOUND validation_step edge_class={edge_class} {precision} ({maps[1].dtype} maps): worst err/bound "
          f"{float(ratio.max()):.3f}")
    assert (ratio <= 1.0).all(), (got, want)
    # the case tells the edge classes apart, and the masked pixels matter
    other = M.eval_counts_ref(d, e, c, bdist.numpy(), y.numpy(), 5 - edge_class, 0.5)
    assert not np.array_equal(other[3:], ref_c[3:]) and ref_c[0] < n
