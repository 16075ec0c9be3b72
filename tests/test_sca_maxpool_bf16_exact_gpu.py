"""The bf16 NHWC kernels of cn_sca_bf16.hip -- cn_sca_pool_fwd/bwd_bf16, cn_sca_apply_fwd/bwd_bf16,
cn_adaptive_maxpool_fwd/bwd_bf16 -- through the C ABI, and engine.spatial_channel_attention on bf16 Vars, against the
float64 references of tests/pointwise_ref.py. The two layers of tests/test_pointwise_exact_gpu.py:

* exact: few-valued / small-integer data arranged so that every intermediate is representable (the premise is
  asserted); results must EQUAL float64;
* bounded: random bf16-representable data, per element e = D * 2^-24 * A (A: the same expression on absolute values,
  D: the fp32 roundings on the way to one output, counted from the kernel in each docstring), and for a bf16 store
  bound = e + half_ulp_bf16(|ref| + e). No floors, nothing fitted to what the GPU returns.

The shapes are the corners of the block tiling (pointwise_ref.sca_tile): 256 threads = R pixel rows x G = C/8 channel
groups, 8 R pixels per block. Outputs live in NaN- or sentinel-filled canvases with slack behind them, which must
survive; the gaps of the inputs hold garbage. tests/test_pointwise_ref.py shows on the CPU that these bounds pass a
perfect kernel and fail kernels that leave out a term or break a tie rule. Run with -s to read the err/bound ratios.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from conv_exact_worker import (BF, GARB, RED, SENT, U32, Canvas, Flat, assert_exact, bounded, half_ulp_bf16, ints, lib,
                               premise, rb, stream)
from conv_exact_worker import act_err as _act_err, canary as _canary, dev as _dev, same as _same

pytestmark = pytest.mark.gpu

NAN = float("nan")
I32 = torch.int32


def _ws(B, C, L, dev):
    n = lib().query("cn_sca_workspace_floats_bf16", B, C, L)
    assert n > 0
    return Flat((n,), dev), n


def _pitch(C, ld):
    return ld if ld is not None else C + 8


# ---------------------------------------------------------------------------------------------------------------------
# pools: cn_sca_pool_fwd_bf16
# ---------------------------------------------------------------------------------------------------------------------

def _pool_fwd(x, ld):
    dev = _dev()
    B, C, H, W = x.shape
    Lp = H * W
    xc = Canvas(x.shape, BF, dev, pitch=ld, fill=GARB, data=x)
    avg, mx, pooled = Flat((B, C), dev), Flat((B, C), dev), Flat((B, 2, H, W), dev)
    idx = Flat((B, C), dev, fill=-7, dtype=I32)
    ws, n = _ws(B, C, Lp, dev)
    lib().call("cn_sca_pool_fwd_bf16", xc.ptr, xc.pitch, B, C, Lp, avg.ptr, mx.ptr, idx.ptr, pooled.ptr, ws.ptr, n,
               stream())
    torch.cuda.synchronize()
    for f, name in ((avg, "avg"), (mx, "mx"), (pooled, "pooled"), (idx, "idx"), (ws, "workspace")):
        f.assert_slack(name)
    return avg, mx, idx, pooled


def _geometry(C, Lp, ld):
    """The case still sits on the corner of the tiling its comment names."""
    G, Rr, px, nchunk = R.sca_tile(C, Lp)
    assert px <= 2048 and Rr * C <= 2048
    if C == 8:
        assert px == 2048
    if C == 24:
        assert Rr * G == 255
    if C == 1024:
        assert Rr * C == 2048
    if Lp in (2049, 681):
        assert Lp == px + 1 and nchunk == 2
    return G, Rr, px, nchunk


@pytest.mark.parametrize("B,C,H,W,ld", R.SCA_BF16_SHAPES + [s + (None,) for s in R.SCA_BF16_POW2])
def test_sca_pool_fwd_bf16_few_valued(B, C, H, W, ld):
    """Multiples of 1/2 from five values: ties in both maxima. Every sum is exact, so avg and the channel mean differ
    from float64 by their one division (D = 1); mx, idx (first maximum, as nn.AdaptiveMaxPool2d) and the channel max
    are equal."""
    _geometry(C, H * W, ld)
    x = R.bf_few((B, C, H, W), 1000 + C + H)
    premise("sca pool sums (in halves)", 2.0 * max(C, H * W))
    avg, mx, idx, pooled = _pool_fwd(x, _pitch(C, ld))
    ravg, rmx, ridx, rcm, rcx = R.sca_pools64(x)
    what = f"sca pool fwd bf16 few {B}x{C}x{H}x{W}"
    bounded(avg.t, ravg, U32 * ravg.abs(), what + " avg")
    bounded(pooled.t[:, 0], rcm, U32 * rcm.abs(), what + " channel mean")
    assert_exact(mx.t, rmx, "mx")
    assert torch.equal(idx.t.cpu().long(), ridx), "idx (first maximum)"
    assert_exact(pooled.t[:, 1], rcx, "channel max")
    assert bool(((x == rcx.unsqueeze(1)).sum(1) > 1).any()) and bool((ridx > 0).any())  # ties, in both maxima


@pytest.mark.parametrize("B,C,H,W,ld", R.SCA_BF16_SHAPES)
def test_sca_pool_fwd_bf16_random_bound(B, C, H, W, ld):
    """avg: a thread adds its 8 pixels, the block its R rows, the finisher the nchunk blocks, one division:
    D = 8 + R + nchunk + 1 on mean |x|. Channel mean: 8 channels in a thread, G groups, the division: D = 8 + G + 1.
    The maxima are exact."""
    G, Rr, px, nchunk = _geometry(C, H * W, ld)
    x = R.bf_randn((B, C, H, W), 1010 + C + H)
    avg, mx, idx, pooled = _pool_fwd(x, _pitch(C, ld))
    ravg, rmx, ridx, rcm, rcx = R.sca_pools64(x)
    what = f"sca pool fwd bf16 {B}x{C}x{H}x{W}"
    bounded(avg.t, ravg, (8 + Rr + nchunk + 1) * U32 * x.abs().mean((2, 3)), what + " avg")
    bounded(pooled.t[:, 0], rcm, (8 + G + 1) * U32 * x.abs().mean(1), what + " channel mean")
    assert_exact(mx.t, rmx, "mx")
    assert torch.equal(idx.t.cpu().long(), ridx), "idx"
    assert_exact(pooled.t[:, 1], rcx, "channel max")


def test_sca_pool_fwd_bf16_nan_and_minus_inf():
    """Four blocks per image (168 px each). A NaN wins both maxima and keeps its index; of two NaNs in a plane the
    later one wins, whether they meet in one thread (pixels 3 and 45: row 3, iterations 0 and 2), in one block, or in
    two blocks; a plane of -inf has pixel 0 as its maximum; avg and the channel mean are NaN / -inf where float64
    says so (the finite ones keep the random bound)."""
    B, C, H, W = 2, 96, 25, 25
    G, Rr, px, nchunk = R.sca_tile(C, H * W)
    assert nchunk == 4 and Rr == 21
    x = R.bf_randn((B, C, H, W), 1020)
    xf = x.view(B, C, H * W)
    xf[0, 1, 200] = NAN
    xf[0, 5, 10] = xf[0, 5, 400] = NAN    # two blocks
    xf[0, 7, 3] = xf[0, 7, 100] = NAN     # one block, two threads
    xf[0, 9, 3] = xf[0, 9, 45] = NAN      # one thread
    x[1, 2] = -math.inf
    x[1, :, 7, 7] = -math.inf
    avg, mx, idx, pooled = _pool_fwd(x, C + 8)
    ravg, rmx, ridx, rcm, rcx = R.sca_pools64(x)
    assert [int(ridx[0, c]) for c in (1, 5, 7, 9)] == [200, 400, 100, 45] and int(ridx[1, 2]) == 0
    assert math.isnan(float(ravg[0, 1])) and float(ravg[1, 2]) == -math.inf and float(rcx[1, 7, 7]) == -math.inf
    assert math.isnan(float(rcx.view(B, -1)[0, 200])) and bool((rcm[1] == -math.inf).all())
    _same(mx.t, rmx, "mx")
    assert torch.equal(idx.t.cpu().long(), ridx), "idx"
    _same(pooled.t[:, 1], rcx, "channel max")
    got_avg, got_cm = avg.t.cpu().double(), pooled.t[:, 0].cpu().double()
    for got, ref, D, mag, name in ((got_avg, ravg, 8 + Rr + nchunk + 1, x.abs().mean((2, 3)), "avg"),
                                   (got_cm, rcm, 8 + G + 1, x.abs().mean(1), "channel mean")):
        fin = ref.isfinite()
        assert torch.equal(got.isnan(), ref.isnan()) and torch.equal(got == -math.inf, ref == -math.inf), name
        assert int(fin.sum()) > 0 and bool(((got - ref).abs()[fin] <= (D * U32 * mag)[fin]).all()), name


# ---------------------------------------------------------------------------------------------------------------------
# pools: cn_sca_pool_bwd_bf16
# ---------------------------------------------------------------------------------------------------------------------

def _pool_bwd(x, davg, dmx, dpool, base, accumulate, ld, idx=None):
    """cn_sca_pool_bwd_bf16 with float64 torch's first-maximum indices; returns dx [B,C,H,W] (CPU float64)."""
    dev = _dev()
    B, C, H, W = x.shape
    xc = Canvas(x.shape, BF, dev, pitch=ld, fill=GARB, data=x)
    if idx is None:
        idx = R.sca_pools64(x)[2]
    g = [Flat(t.shape, dev, data=t) for t in (davg, dmx, dpool)]
    ix = Flat((B, C), dev, fill=-7, dtype=I32, data=idx)
    dxc = Canvas(x.shape, BF, dev, pitch=ld, fill=NAN, data=base if accumulate else None)
    lib().call("cn_sca_pool_bwd_bf16", xc.ptr, xc.pitch, g[0].ptr, g[1].ptr, ix.ptr, g[2].ptr, dxc.ptr, dxc.pitch, B, C,
               H * W, accumulate, stream())
    torch.cuda.synchronize()
    _canary(dxc, "sca pool dx")
    return dxc.t.cpu().double()


@pytest.mark.parametrize("B,C,H,W", R.SCA_BF16_POW2)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_sca_pool_bwd_bf16_exact(B, C, H, W, accumulate):
    """Planes of 2^k pixels, 1, 2, 4 or 8 channels at every pixel's maximum, gradients that divide evenly: every
    float64 dx is an integer of at most 256 (asserted) and the kernel must return it. All four gradients together, then
    each one alone with the other three zero, so that a missing path cannot hide behind another."""
    x, davg, dmx, dpool, base = R.sca_pool_bwd_exact_inputs(B, C, H, W, 950 + C)
    n = (x == x.amax(1, keepdim=True)).sum(1)
    assert sorted(n.unique().tolist()) == [1, 2, 4, 8]
    z = torch.zeros_like
    only = {"all": (davg, dmx, dpool),
            "H*W average": (davg, z(dmx), z(dpool)),
            "H*W max": (z(davg), dmx, z(dpool)),
            "channel mean": (z(davg), z(dmx), torch.stack([dpool[:, 0], z(dpool[:, 1])], 1)),
            "channel max": (z(davg), z(dmx), torch.stack([z(dpool[:, 0]), dpool[:, 1]], 1))}
    for name, (a, m, p) in only.items():
        g, _ = R.sca_pool_bwd_terms64(x, a, m, p)
        ref = sum(g) + (base if accumulate else 0.0)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 256 and float(ref.abs().max()) > 0
        got = _pool_bwd(x, a, m, p, base, accumulate, C + 8)
        assert_exact(got, ref, f"sca pool bwd bf16 {B}x{C}x{H}x{W} acc={accumulate} {name}: dx")


@pytest.mark.parametrize("B,C,H,W,ld,few,accumulate", R.SCA_POOL_BWD_BOUNDED)
def test_sca_pool_bwd_bf16_bound(B, C, H, W, ld, few, accumulate):
    """fl(1/L) and davg * fl(1/L), dpool0 / C, dpool1 / n, three adds: D = 7 on the sum of the four absolute terms,
    one more add (on that sum + |old|) when accumulating, then the store's half bf16 ulp
    (pointwise_ref.sca_pool_bwd_bound)."""
    _geometry(C, H * W, ld)
    x, davg, dmx, dpool, base = R.sca_pool_bwd_inputs(B, C, H, W, few, 900 + C + H)
    g, A = R.sca_pool_bwd_terms64(x, davg, dmx, dpool)
    ref = sum(g) + (base if accumulate else 0.0)
    got = _pool_bwd(x, davg, dmx, dpool, base, accumulate, ld)
    bounded(got, ref, R.sca_pool_bwd_bound(ref, A, base if accumulate else None),
            f"sca pool bwd bf16 {B}x{C}x{H}x{W} few={few} acc={accumulate} dx")


def test_sca_pool_bwd_bf16_nan_and_minus_inf():
    """An all -inf pixel ties in every channel: dpool1 is split over all C. A pixel with a NaN channel has no channel
    equal to its (NaN) maximum: dpool1 goes to nobody (float64 autograd of torch.amax divides 0 by 0 there and returns
    NaN for the whole pixel; the rule checked is the kernel's documented one). The NaN is its plane's H*W maximum and
    takes dmx."""
    B, C, H, W = 1, 24, 9, 11
    x = R.bf_randn((B, C, H, W), 1030)
    x[0, :, 1, 1] = -math.inf
    x[0, 5, 2, 2] = NAN
    davg, dmx, dpool, base = R.f32_randn((B, C), 1031, 4.0), R.f32_randn((B, C), 1032, 4.0), \
        R.f32_randn((B, 2, H, W), 1033), R.bf_randn((B, C, H, W), 1034, 0.05)
    idx = R.sca_pools64(x)[2]
    assert int(idx[0, 5]) == 2 * W + 2
    xs = x.clone()          # a finite stand-in with the same first maxima and an even split at the -inf pixel
    xs[0, :, 1, 1] = -50.0
    xs[0, 5, 2, 2] = 100.0
    assert torch.equal(R.sca_pools64(xs)[2], idx)
    g, _ = R.sca_pool_bwd_terms64(xs, davg, dmx, dpool)
    assert bool((g[3][0, :, 1, 1] == dpool[0, 1, 1, 1] / C).all())
    g[3][0, :, 2, 2] = 0.0
    A = sum(t.abs() for t in g)
    for acc in (0, 1):
        ref = sum(g) + (base if acc else 0.0)
        got = _pool_bwd(x, davg, dmx, dpool, base, acc, C + 8, idx=idx)
        bounded(got, ref, R.sca_pool_bwd_bound(ref, A, base if acc else None), f"sca pool bwd bf16 NaN/-inf acc={acc}")


# ---------------------------------------------------------------------------------------------------------------------
# gating: cn_sca_apply_fwd_bf16, cn_sca_apply_bwd_bf16
# ---------------------------------------------------------------------------------------------------------------------

def _apply(out, dy, ca, sconv, gamma, base, ld, runs):
    """cn_sca_apply_fwd_bf16 once, cn_sca_apply_bwd_bf16 once per (accumulate, with dout) of `runs`.
    Returns y and a list of (dout or None, dca, dsconv, dgamma), all CPU float64; dgamma starts at 0.25."""
    dev, L, st = _dev(), lib(), stream()
    B, C, H, W = out.shape
    Lp = H * W
    oc = Canvas(out.shape, BF, dev, pitch=ld, fill=GARB, data=out)
    dyc = Canvas(dy.shape, BF, dev, pitch=ld, fill=GARB, data=dy)
    yc = Canvas(out.shape, BF, dev, pitch=ld, fill=NAN)
    cad, sd = Flat((B, C), dev, data=ca), Flat((B, 1, H, W), dev, data=sconv)
    gd = Flat((1,), dev, data=torch.tensor([gamma], dtype=torch.float64))
    L.call("cn_sca_apply_fwd_bf16", oc.ptr, oc.pitch, cad.ptr, sd.ptr, gd.ptr, yc.ptr, yc.pitch, B, C, Lp, st)
    torch.cuda.synchronize()
    _canary(yc, "sca apply y")
    res = []
    for acc, with_dout in runs:
        ws, n = _ws(B, C, Lp, dev)
        doc = Canvas(out.shape, BF, dev, pitch=ld, fill=NAN, data=base if acc else None)
        dca, ds = Flat((B, C), dev), Flat((B, 1, H, W), dev)
        dg = Flat((1,), dev, data=torch.tensor([0.25]))
        L.call("cn_sca_apply_bwd_bf16", dyc.ptr, dyc.pitch, oc.ptr, oc.pitch, cad.ptr, sd.ptr, gd.ptr,
               doc.ptr if with_dout else None, doc.pitch if with_dout else 0, acc, dca.ptr, ds.ptr, dg.ptr, ws.ptr, n,
               B, C, Lp, st)
        torch.cuda.synchronize()
        if with_dout:
            _canary(doc, "sca apply dout")
        else:
            assert bool(doc.buf.isnan().all()), "dout is nullable: nothing may be written"
        for f, name in ((dca, "dca"), (ds, "dsconv"), (dg, "dgamma"), (ws, "workspace")):
            f.assert_slack(name)
        res.append((doc.t.cpu().double() if with_dout else None, dca.t.cpu().double(), ds.t.cpu().double(),
                    dg.t.cpu().double()))
    return yc.t.cpu().double(), res


@pytest.mark.parametrize("B,C,H,W,ld", R.SCA_BF16_SHAPES + [s + (None,) for s in R.SCA_BF16_POW2])
def test_sca_apply_bf16_exact(B, C, H, W, ld):
    """gamma = 2 (g = 1), sconv = 0 (the sigmoid is exactly 1/2), ca from {0, 1/2, 1}: the factor is 1.5, 2 or 2.5.
    With small-integer out / dy / base, y, dout (accumulate 0 and 1), dca = S, dsconv = T / 4 and
    dgamma = 1/4 + (sum ca S + sum T / 2) / 2 are sums of multiples of 1/4 below 2^24 / 4 (asserted): they equal
    float64 in any order. dout = NULL writes nothing and gives the same dca / dsconv / dgamma; two runs are
    bit-identical."""
    out, dy, base = ints((B, C, H, W), -4, 4, 1100 + C), ints((B, C, H, W), -3, 3, 1101 + C), \
        ints((B, C, H, W), -8, 8, 1102 + C)
    ca = ints((B, C), 0, 2, 1103 + C, zeros=0.0) * 0.5
    sconv = torch.zeros(B, 1, H, W, dtype=torch.float64)
    t = dy * out
    premise("sca apply sums (in quarters)", 4 * (1.5 * float(t.abs().sum()) + 1))
    att = 1.5 + ca.view(B, C, 1, 1)
    y, res = _apply(out, dy, ca, sconv, 2.0, base, _pitch(C, ld), [(0, True), (1, True), (0, False), (0, True)])
    what = f"sca apply bf16 {B}x{C}x{H}x{W}"
    assert torch.equal(rb(out * att), out * att) and torch.equal(rb(dy * att + base), dy * att + base)
    assert_exact(y, out * att, what + " y")
    S, T = t.sum((2, 3)), t.sum(1, keepdim=True)
    ref_dg = 0.25 + 0.5 * ((ca * S).sum() + 0.5 * T.sum())
    for (acc, with_dout), (dout, dca, ds, dg) in zip([(0, True), (1, True), (0, False), (0, True)], res):
        tag = f"{what} acc={acc} dout={with_dout}"
        if with_dout:
            assert_exact(dout, dy * att + (base if acc else 0.0), tag + " dout")
        assert_exact(dca, S, tag + " dca")
        assert_exact(ds, T / 4, tag + " dsconv")
        assert_exact(dg, ref_dg.view(1), tag + " dgamma")
    for a, b in zip(res[0], res[3]):
        assert torch.equal(a, b), "not bit-reproducible"


@pytest.mark.parametrize("B,C,H,W,ld", R.SCA_BF16_SHAPES)
def test_sca_apply_bf16_random_bound(B, C, H, W, ld):
    """Random fp32 ca, sconv ~ N(0, 4), gamma = 0.9; t = dy out (exact in fp32: two bf16 factors).

    y, dout: the factor 1 + g (ca + sa) costs the sigmoid's (|s| + 8) u sa, an add, a product and an add
    (pointwise_ref.sca_att64), the product with out / dy one more, the accumulate one more, then the store's half bf16
    ulp (pointwise_ref.sca_gate_bound).
    dsconv = g sa (1 - sa) T: T adds 8 channels in a thread and G groups (the products are exact), then 1 - sa and
    three products: D = 8 + G + 4 on sum_c |t|, and the sigmoid's error through |d/ds s (1 - s)| <= 1.
    dca = g S: 8 pixels in a thread, R rows, nchunk blocks, the product with g: D = 8 + R + nchunk + 1 on sum_l |t|.
    dgamma = 1/4 + sum_b 0.5 (sum_c ca S + sum_chunk pT), pT = block sum of sa T over the block's pixels. The longest
    chain: S as above (8 + R + nchunk) and ca S (1), or T (8 + G), sa T (1), a thread's ceil(8 R / 256) pixels and the
    block sum (RED); then the finisher's ceil(C / 256) + ceil(nchunk / 256) adds and block sum (RED), the last kernel's
    ceil(B / 256) adds, block sum (RED) and the add onto the prefill (1); sa's own error is carried per term."""
    G, Rr, px, nchunk = _geometry(C, H * W, ld)
    out, dy = R.bf_randn((B, C, H, W), 1110 + C), R.bf_randn((B, C, H, W), 1111 + C)
    base = R.bf_randn((B, C, H, W), 1112 + C, 0.1)
    ca, sconv = torch.sigmoid(R.f32_randn((B, C), 1113 + C)).float().double(), R.f32_randn((B, 1, H, W), 1114 + C, 2.0)
    gamma = float(torch.tensor(0.9).float())
    g, sa, inner, e_inner, att, mag, e_att = R.sca_att64(ca, sconv, gamma)
    y, res = _apply(out, dy, ca, sconv, gamma, base, ld, [(0, True), (1, True), (0, False)])
    what = f"sca apply bf16 {B}x{C}x{H}x{W}"
    bounded(y, *R.sca_gate_bound(out, att, mag, e_att), what + " y")
    t = dy * out
    ref_dca = g * t.sum((2, 3))
    b_dca = (8 + Rr + nchunk + 1) * U32 * abs(g) * t.abs().sum((2, 3))
    ssum = t.sum(1, keepdim=True)
    ref_ds = g * sa * (1 - sa) * ssum
    b_ds = abs(g) * ((8 + G + 4) * U32 * sa * (1 - sa) * t.abs().sum(1, keepdim=True)
                     + _act_err(sconv, 0.0, sa) * ssum.abs())
    ref_dg = 0.25 + 0.5 * (t * inner).sum()
    chain = max(8 + Rr + nchunk + 1, 8 + G + 1 + math.ceil(8 * Rr / 256) + RED) \
        + math.ceil(C / 256) + math.ceil(nchunk / 256) + RED + math.ceil(B / 256) + RED + 1
    b_dg = 0.5 * float((t.abs() * _act_err(sconv, 0.0, sa)).sum()) \
        + chain * U32 * (0.5 * float((t.abs() * inner).sum()) + 0.25)
    for (acc, with_dout), (dout, dca, ds, dg) in zip([(0, True), (1, True), (0, False)], res):
        tag = f"{what} acc={acc} dout={with_dout}"
        if with_dout:
            bounded(dout, *R.sca_gate_bound(dy, att, mag, e_att, base if acc else None), tag + " dout")
        bounded(dca, ref_dca, b_dca, tag + " dca")
        bounded(ds, ref_ds, b_ds, tag + " dsconv")
        bounded(dg, ref_dg.view(1), torch.full((1,), b_dg, dtype=torch.float64), tag + f" dgamma (chain {chain})")


# ---------------------------------------------------------------------------------------------------------------------
# cn_adaptive_maxpool_fwd_bf16 / cn_adaptive_maxpool_bwd_bf16
# ---------------------------------------------------------------------------------------------------------------------

def _maxpool_fwd(x, Ho, Wo, ld, with_idx=True):
    dev = _dev()
    B, C, Hi, Wi = x.shape
    xc = Canvas(x.shape, BF, dev, pitch=ld, fill=GARB, data=x)
    yc = Canvas((B, C, Ho, Wo), BF, dev, pitch=ld, fill=SENT)  # NaN is a possible result
    idx = Flat((B, Ho, Wo, C), dev, fill=-7, dtype=I32)
    lib().call("cn_adaptive_maxpool_fwd_bf16", xc.ptr, xc.pitch, yc.ptr, yc.pitch, idx.ptr if with_idx else None, B, C,
               Hi, Wi, Ho, Wo, stream())
    torch.cuda.synchronize()
    _canary(yc, "max pool y")
    idx.assert_slack("idx")
    if not with_idx:
        assert bool((idx.buf == -7).all())
    return yc.t.cpu().double(), idx.t.permute(0, 3, 1, 2).cpu().long()


def _maxpool_bwd(dy, idx, Hi, Wi, base, accumulate, ld):
    """idx: [B,C,Ho,Wo] flat input pixels (float64 torch's). Returns dx (CPU float64)."""
    dev = _dev()
    B, C, Ho, Wo = dy.shape
    dyc = Canvas(dy.shape, BF, dev, pitch=ld, fill=GARB, data=dy)
    ix = Flat((B, Ho, Wo, C), dev, fill=-7, dtype=I32, data=idx.permute(0, 2, 3, 1))
    dxc = Canvas((B, C, Hi, Wi), BF, dev, pitch=ld, fill=NAN, data=base if accumulate else None)
    lib().call("cn_adaptive_maxpool_bwd_bf16", dyc.ptr, dyc.pitch, ix.ptr, dxc.ptr, dxc.pitch, B, C, Hi, Wi, Ho, Wo,
               accumulate, stream())
    torch.cuda.synchronize()
    _canary(dxc, "max pool dx")
    return dxc.t.cpu().double()


@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo,ld", R.MAXPOOL_BF16_CASES)
def test_adaptive_maxpool_bf16_exact(B, C, Hi, Wi, Ho, Wo, ld):
    """Few-valued x: y and idx (first maximum of the window) equal float64 F.adaptive_max_pool2d, idx = NULL gives the
    same y, and with small-integer dy and base dx equals float64 autograd at accumulate 0 and 1. Where the windows
    overlap, some input pixel is the first maximum of two windows and some of four."""
    x = R.maxpool_inputs(B, C, Hi, Wi, Ho, Wo, 960)
    dy, base = ints((B, C, Ho, Wo), -3, 3, 1200, zeros=0.0), ints((B, C, Hi, Wi), -8, 8, 1201)
    y64, i64, dx64, _, cnt = R.maxpool_bwd64(x, dy, (Ho, Wo))
    if Hi % Ho:
        assert bool((cnt == 2).any()) and bool((cnt == 4).any())
    else:
        assert (Hi, Wi) == (Ho, Wo) and torch.equal(y64, x)
    y, idx = _maxpool_fwd(x, Ho, Wo, ld)
    assert_exact(y, y64, "y")
    assert torch.equal(idx, i64), "idx (first maximum of the window)"
    y2, _ = _maxpool_fwd(x, Ho, Wo, ld, with_idx=False)
    assert_exact(y2, y64, "y (no idx)")
    for acc in (0, 1):
        got = _maxpool_bwd(dy, i64, Hi, Wi, base, acc, ld)
        assert_exact(got, dx64 + (base if acc else 0.0), f"max pool bf16 {Hi}x{Wi}->{Ho}x{Wo} dx acc={acc}")


@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo,ld", R.MAXPOOL_BF16_CASES)
@pytest.mark.parametrize("few", [True, False])
def test_adaptive_maxpool_bwd_bf16_bound(B, C, Hi, Wi, Ho, Wo, ld, few):
    """Random bf16 dy: an input pixel adds the dy of the w windows it is the first maximum of (at most w roundings),
    then the old value: D = w + accumulate on sum |dy| + |old|, and the store's half bf16 ulp. A pixel that is nobody's
    maximum gets exactly 0 (or keeps its old value)."""
    x = R.maxpool_inputs(B, C, Hi, Wi, Ho, Wo, 960) if few else R.bf_randn((B, C, Hi, Wi), 1210)
    dy, base = R.bf_randn((B, C, Ho, Wo), 961), R.bf_randn((B, C, Hi, Wi), 962, 0.05)
    y64, i64, dx64, dxa, cnt = R.maxpool_bwd64(x, dy, (Ho, Wo))
    for acc in (0, 1):
        ref = dx64 + (base if acc else 0.0)
        got = _maxpool_bwd(dy, i64, Hi, Wi, base, acc, ld)
        bounded(got, ref, R.bf16_store_bound(ref, cnt, dxa, base if acc else None),
                f"max pool bf16 {Hi}x{Wi}->{Ho}x{Wo} few={few} dx acc={acc}")
        assert torch.equal(got[cnt == 0], ref[cnt == 0])


def test_adaptive_maxpool_bf16_nan():
    """7 -> 3: windows [0,3) [2,5) [4,7). A NaN in a window wins y and takes the gradient; of two NaNs in a window the
    later one in row-major order wins; a NaN on a shared pixel wins all four windows."""
    B, C, Hi, Ho, ld = 2, 8, 7, 3, 16
    x = R.bf_randn((B, C, Hi, Hi), 1220)
    x[0, 1, 0, 1] = NAN                         # window (0, 0) only
    x[0, 2, 5, 0] = x[0, 2, 6, 1] = NAN         # both in window (2, 0): (6, 1) is the later one
    x[0, 3, 0, 5] = x[0, 3, 0, 6] = NAN         # same row of window (0, 2)
    x[1, 4, 2, 2] = NAN                         # shared by four windows
    dy, base = ints((B, C, Ho, Ho), -3, 3, 1221, zeros=0.0), ints((B, C, Hi, Hi), -8, 8, 1222)
    y64, i64, dx64, _, cnt = R.maxpool_bwd64(x, dy, (Ho, Ho))
    assert int(i64[0, 1, 0, 0]) == 1 and int(i64[0, 2, 2, 0]) == 6 * Hi + 1 and int(i64[0, 3, 0, 2]) == 6
    assert i64[1, 4, :2, :2].flatten().tolist() == [2 * Hi + 2] * 4 and int(cnt[1, 4, 2, 2]) == 4
    assert int(y64.isnan().sum()) == 7 and float(dx64[0, 2, 5, 0]) == 0.0
    y, idx = _maxpool_fwd(x, Ho, Ho, ld)
    _same(y, y64, "y")
    assert torch.equal(idx, i64), "idx"
    for acc in (0, 1):
        got = _maxpool_bwd(dy, i64, Hi, Hi, base, acc, ld)
        assert_exact(got, dx64 + (base if acc else 0.0), f"max pool bf16 NaN dx acc={acc}")


# ---------------------------------------------------------------------------------------------------------------------
# the second trip of the grid-stride loops (the launchers cap the grid at 16384 blocks of 256 threads)
# ---------------------------------------------------------------------------------------------------------------------
CAP = 16384 * 256


def _i8(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8)


def test_sca_apply_fwd_bf16_second_grid_trip():
    """C = 8, a 2049 x 2049 plane: 4198401 channel groups, 4097 more than the capped grid's threads, so 4097 threads
    make a second trip. The exact layer's data (factor 1.5, 2 or 2.5 by channel, integer out): every y equals
    float64."""
    dev, L, st = _dev(), lib(), stream()
    B, C, H, W = 1, 8, 2049, 2049
    assert CAP < B * H * W * (C // 8) < 2 * CAP and (B * H * W * (C // 8)) % 256 != 0
    out = _i8((B, C, H, W), -4, 4, 1300)
    ca = ints((B, C), 0, 2, 1301, zeros=0.0) * 0.5
    oc = Canvas(out.shape, BF, dev, pitch=C, fill=GARB, data=out.to(BF))
    yc = Canvas(out.shape, BF, dev, pitch=C, fill=NAN)
    cad, sd = Flat((B, C), dev, data=ca), Flat((B, 1, H, W), dev, fill=0.0)
    gd = Flat((1,), dev, data=torch.tensor([2.0]))
    L.call("cn_sca_apply_fwd_bf16", oc.ptr, oc.pitch, cad.ptr, sd.ptr, gd.ptr, yc.ptr, yc.pitch, B, C, H * W, st)
    torch.cuda.synchronize()
    ref = out.double() * (1.5 + ca.view(B, C, 1, 1))
    assert float(ref.abs().max()) == 10.0
    assert_exact(yc.t, ref, "y")
    _canary(yc, "y")


@pytest.fixture(scope="module")
def big_pool():
    """2050 x 2050 -> 2049 x 2049 at C = 8: every window is 2 x 2 and overlaps its neighbours. Few-valued x, integer
    dy; the float64 reference is computed once and kept in narrow types (all values are exact in them)."""
    B, C, Hi, Ho = 1, 8, 2050, 2049
    x = _i8((B, C, Hi, Hi), -2, 2, 1310)
    dy = _i8((B, C, Ho, Ho), -3, 3, 1311)
    xr = (x.double() * 0.5).requires_grad_(True)
    y, idx = F.adaptive_max_pool2d(xr, (Ho, Ho), return_indices=True)
    (dx,) = torch.autograd.grad(y, xr, dy.double())
    assert float(dx.abs().max()) <= 12
    return dict(x=x, dy=dy, y2=(2 * y.detach()).to(torch.int8), idx=idx.to(I32), dx=dx.to(torch.int8), Hi=Hi, Ho=Ho)


def test_adaptive_maxpool_fwd_bf16_second_grid_trip(big_pool):
    """4198401 output groups: 4097 threads make a second trip. y and idx equal float64."""
    dev, L, st = _dev(), lib(), stream()
    p = big_pool
    B, C, Hi, Ho = 1, 8, p["Hi"], p["Ho"]
    assert CAP < B * Ho * Ho * (C // 8) < 2 * CAP
    xc = Canvas((B, C, Hi, Hi), BF, dev, pitch=C, fill=GARB, data=p["x"].to(BF) * 0.5)
    yc = Canvas((B, C, Ho, Ho), BF, dev, pitch=C, fill=NAN)
    idx = Flat((B, Ho, Ho, C), dev, fill=-7, dtype=I32)
    L.call("cn_adaptive_maxpool_fwd_bf16", xc.ptr, xc.pitch, yc.ptr, yc.pitch, idx.ptr, B, C, Hi, Hi, Ho, Ho, st)
    torch.cuda.synchronize()
    assert torch.equal((yc.t * 2).to(torch.int8).cpu(), p["y2"]) and bool((yc.t * 2 == (yc.t * 2).round()).all()), "y"
    assert torch.equal(idx.t.permute(0, 3, 1, 2).cpu(), p["idx"]), "idx"
    _canary(yc, "y")
    idx.assert_slack("idx")


def test_adaptive_maxpool_bwd_bf16_second_grid_trip(big_pool):
    """4202500 input groups: 8196 threads make a second trip. Integer dy, up to four windows per pixel: dx equals
    float64 autograd."""
    dev, L, st = _dev(), lib(), stream()
    p = big_pool
    B, C, Hi, Ho = 1, 8, p["Hi"], p["Ho"]
    assert CAP < B * Hi * Hi * (C // 8) < 2 * CAP
    dyc = Canvas((B, C, Ho, Ho), BF, dev, pitch=C, fill=GARB, data=p["dy"].to(BF))
    ix = Flat((B, Ho, Ho, C), dev, fill=-7, dtype=I32, data=p["idx"].permute(0, 2, 3, 1))
    dxc = Canvas((B, C, Hi, Hi), BF, dev, pitch=C, fill=NAN)
    L.call("cn_adaptive_maxpool_bwd_bf16", dyc.ptr, dyc.pitch, ix.ptr, dxc.ptr, dxc.pitch, B, C, Hi, Hi, Ho, Ho, 0, st)
    torch.cuda.synchronize()
    got = dxc.t.cpu()
    assert bool((got.float() == got.float().round()).all()) and torch.equal(got.to(torch.int8), p["dx"]), "dx"
    _canary(dxc, "dx")


# ---------------------------------------------------------------------------------------------------------------------
# engine.spatial_channel_attention on bf16 Vars: the routing of the four pool paths
# ---------------------------------------------------------------------------------------------------------------------
ROUTE = 1e-4  # the routing allowance of test_pointwise_exact_gpu.py::test_sca_engine_f32: fewer than 544 fp32 roundings


def _route_bound(ref, A, old=None):
    e = ROUTE * A
    if old is not None:
        e = e + U32 * (A + old.abs())
    return e + half_ulp_bf16(ref.abs() + e)


def _tie_free(shape, seed):
    """Random bf16 values with a unique maximum in every pixel's channels and in every plane: pixel l's channel l % C
    holds 8 + (l // C) / 16 (exact in bf16, above every N(0, 1) draw, distinct within its plane)."""
    B, C, H, W = shape
    x = R.bf_randn(shape, seed)
    l = torch.arange(H * W)
    x.view(B, C, H * W)[:, l % C, l] = (8.0 + (l // C).double() / 16).expand(B, H * W)
    assert torch.equal(rb(x), x) and H * W // C < 16
    return x


@pytest.fixture(scope="module", params=[(2, 24, 9, 11, False), (2, 24, 9, 11, True), (1, 96, 25, 25, False),
                                        (1, 96, 25, 25, True)],
                ids=lambda p: "x".join(map(str, p[:4])) + ("-few" if p[4] else "-tiefree"))
def sca_engine_case(request):
    """The module, inputs and float64 reference of one engine case, computed once for its routing variants."""
    from cultionet_amd.convolution import SpatialChannelAttention

    B, C, H, W, few = request.param
    torch.manual_seed(C)
    mod = SpatialChannelAttention(C, "SiLU")
    with torch.no_grad():
        mod.gamma.fill_(0.8)  # nonzero: the attention path carries gradient
    skip = R.bf_few((B, C, H, W), 1400 + C) if few else _tie_free((B, C, H, W), 1400 + C)
    out, dy = R.bf_randn((B, C, H, W), 1401 + C), R.bf_randn((B, C, H, W), 1402 + C)
    ties = (skip == skip.amax(1, keepdim=True)).sum(1) > 1
    plane_ties = (skip == skip.amax((2, 3), keepdim=True)).sum((2, 3)) > 1
    assert bool(ties.any() and plane_ties.any()) if few else not bool(ties.any() or plane_ties.any())
    o64 = out.clone().requires_grad_(True)
    y64, pw, leaves = R.sca_ref64(mod, skip, o64, paths=True)
    y64.backward(dy)
    paths = [l.grad for l in leaves]
    assert all(float(p.abs().max()) > 0 for p in paths)
    from cultionet_amd import engine as E

    mod = mod.to(_dev())
    return dict(mod=mod, store=E.ParamStore(mod), skip=skip, out=out, dy=dy, y=y64.detach(), dout=o64.grad,
                dskip=sum(paths), A=sum(p.abs() for p in paths), pgrad={n: v.grad for n, v in pw.items()},
                what=f"sca engine bf16 {B}x{C}x{H}x{W} few={few}")


def _engine(case, skip_req=True, out_req=True, parent=None):
    """engine.spatial_channel_attention under the tape. parent = (channels before, channels after, prefilled parent
    gradient [B, before + C + after, H, W]): skip is a channel slice of a wider bf16 Var."""
    from cultionet_amd import engine as E

    dev = _dev()
    mod, skip = case["mod"], case["skip"]
    B, C, H, W = skip.shape
    mk = lambda t: Canvas(t.shape, BF, dev, pitch=t.shape[1] + 8, fill=GARB, data=t).t
    store = case["store"]
    store.zero_grad()
    with E.using_store(store), E.recording(True) as tape:
        pv = None
        if parent is None:
            sv = E.Var(mk(skip), skip_req)
        else:
            before, after, pgrad = parent
            wide = R.bf_randn((B, before + C + after, H, W), 1410)
            wide[:, before:before + C] = skip
            pv = E.Var(mk(wide), True)
            pv.grad = mk(pgrad)
            sv = E.split_channels(pv, [before, C, after])[1]
        ov = E.Var(mk(case["out"]), out_req)
        yv = E.spatial_channel_attention(sv, ov, mod)
        assert yv.t.dtype == BF
        yv.grad = mk(case["dy"])
        tape.backward()
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.detach().double().cpu()
    grads = {n: cpu(store.grad_of(p)) for n, p in mod.named_parameters()}
    return cpu(yv.t), cpu(sv.grad), cpu(ov.grad), grads, (None if pv is None else cpu(pv.grad))


def _full(case):
    """The case's plain run (skip and out both take gradients), once."""
    if "full" not in case:
        case["full"] = _engine(case)
    return case["full"]


def _check_params(case, grads, tag, same_as_full=False):
    """fp32 parameter gradients: the routing allowance on the tensor's max |ref|, as the fp32 engine test.
    same_as_full: the variant runs the same kernels on the same inputs as the plain run, so gamma's gradient (sums in
    a fixed order) and the channel MLPs' weight gradients (one float atomic per image onto a zeroed buffer: with at most
    two images the sum does not depend on their order) must have the plain run's bits. The 3x3 conv's weight gradient
    adds one float atomic per block of rows in any order and keeps the allowance only."""
    if same_as_full:
        assert case["skip"].shape[0] <= 2
        full = _full(case)[3]
        for n in grads:
            if n == "gamma" or n.startswith("channel_attention."):
                assert torch.equal(grads[n], full[n]), f"{tag} {n}: differs from the plain run's bits"
    for n, ref in case["pgrad"].items():
        scale = float(ref.abs().max())
        err = float((grads[n] - ref).abs().max())
        print(f"BOUND {case['what']} {tag} {n}: worst err/bound {err / (ROUTE * scale):.3f}")
        assert err <= ROUTE * scale, f"{tag} {n}: max err {err:.3e} > {ROUTE * scale:.3e}"


def test_sca_engine_bf16_paths(sca_engine_case):
    """y, d out and d skip per element: 1e-4 of A plus the store's half bf16 ulp, where A is |y|, |d out|, and for
    d skip the sum of the four pool paths' absolute float64 gradients (pointwise_ref.sca_ref64(paths=True)): a path
    that is dropped, doubled or routed to the wrong tie is far outside."""
    c = sca_engine_case
    y, dskip, dout, grads, _ = _full(c)
    bounded(y, c["y"], _route_bound(c["y"], c["y"].abs()), c["what"] + " y")
    bounded(dout, c["dout"], _route_bound(c["dout"], c["dout"].abs()), c["what"] + " dout")
    bounded(dskip, c["dskip"], _route_bound(c["dskip"], c["A"]), c["what"] + " dskip")
    _check_params(c, grads, "full")


def test_sca_engine_bf16_skip_without_gradient(sca_engine_case):
    """skip.req = False: no skip gradient buffer appears; y and d out keep their bounds, gamma's and the MLPs'
    gradients the plain run's bits (see _check_params)."""
    c = sca_engine_case
    y, dskip, dout, grads, _ = _engine(c, skip_req=False)
    assert dskip is None
    bounded(y, c["y"], _route_bound(c["y"], c["y"].abs()), c["what"] + " skip.req=False y")
    bounded(dout, c["dout"], _route_bound(c["dout"], c["dout"].abs()), c["what"] + " skip.req=False dout")
    _check_params(c, grads, "skip.req=False", same_as_full=True)


def test_sca_engine_bf16_out_without_gradient(sca_engine_case):
    """out.req = False: no out gradient buffer appears; d skip keeps its bound, gamma's and the MLPs' gradients the
    plain run's bits (see _check_params)."""
    c = sca_engine_case
    y, dskip, dout, grads, _ = _engine(c, out_req=False)
    assert dout is None
    bounded(dskip, c["dskip"], _route_bound(c["dskip"], c["A"]), c["what"] + " out.req=False dskip")
    _check_params(c, grads, "out.req=False", same_as_full=True)


def test_sca_engine_bf16_skip_is_a_slice_of_a_wider_var(sca_engine_case):
    """skip = engine.split_channels(parent)[1], the parent's gradient already holding values: d skip is accumulated
    into its slice (one more fp32 add before the store), the other channels keep their bits."""
    c = sca_engine_case
    B, C, H, W = c["skip"].shape
    before, after = 8, 16
    old = R.bf_randn((B, before + C + after, H, W), 1420, 0.05)
    y, dslice, dout, grads, pgrad = _engine(c, parent=(before, after, old))
    sl = slice(before, before + C)
    ref = c["dskip"] + old[:, sl]
    bounded(pgrad[:, sl], ref, _route_bound(ref, c["A"], old[:, sl]), c["what"] + " slice dskip")
    assert torch.equal(dslice, pgrad[:, sl])
    assert torch.equal(pgrad[:, :before], old[:, :before]) and torch.equal(pgrad[:, sl.stop:], old[:, sl.stop:]), \
        "the parent's other channels changed"
    bounded(y, c["y"], _route_bound(c["y"], c["y"].abs()), c["what"] + " slice y")
    _check_params(c, grads, "slice")
