"""Pins tests/pointwise_ref.py on the CPU: the resize matrix against ATen's own fp32 F.interpolate (forward and adjoint)
within a few units of fp32 roundoff, the dyadic sizes and candidate counts the exact GPU layer relies on, the SCA and
final-combine references against the oracle's modules, and the tiling restatements against scalar loops. Run with -s to
read the distances."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R

U = R.U32

PRODUCTION = [(13, 14), (49, 50), (99, 100), (97, 100), (51, 100), (100, 51), (100, 60), (25, 100), (27, 28), (25, 28)]
# n_in, n_out, scale, candidates per interior input index (min, max)
DYADIC = [(5, 9, 0.5, 3, 3), (4, 5, 0.75, 2, 2), (9, 5, 2.0, 0, 1), (25, 97, 0.25, 7, 7), (37, 65, 0.5625, 3, 4),
          (49, 65, 0.75, 2, 3), (65, 33, 2.0, 0, 1), (49, 33, 1.5, 1, 1), (25, 33, 0.75, 2, 3)]


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float()


@pytest.mark.parametrize("n_in,n_out", PRODUCTION + [(d[0], d[1]) for d in DYADIC] + [(1, 4), (6, 1), (3, 1), (7, 5)])
def test_resize_matrix_rows_and_support(n_in, n_out):
    Rm = R.resize_matrix(n_in, n_out)
    assert Rm.shape == (n_out, n_in) and Rm.dtype == torch.float64
    assert bool((Rm >= 0).all()) and bool(((Rm != 0).sum(1) <= 2).all())
    assert float((Rm.sum(1) - 1).abs().max()) <= U  # h = fl(1 - l1): one rounding
    nz = (Rm != 0).nonzero()
    for o in range(n_out):  # the two taps are adjacent
        cols = nz[nz[:, 0] == o, 1]
        assert int(cols.max() - cols.min()) <= 1


@pytest.mark.parametrize("hi,wi,ho,wo", [(a, a, b, b) for a, b in PRODUCTION[:8]] + [(27, 25, 28, 28), (1, 6, 4, 1),
                                                                                       (3, 7, 1, 5)])
def test_resize_matrix_matches_aten_fp32(hi, wi, ho, wo):
    """ATen's fp32 forward and adjoint stay within a few u of the restated reference, measured per element against
    |R||x| (the issue's table: at most 3.4); a float64 F.interpolate is tens to thousands of u away, which is why the
    weights are restated in fp32."""
    x = _rand((2, 3, hi, wi), hi + wo).requires_grad_(True)
    dy = _rand((2, 3, ho, wo), ho + wi)
    y = F.interpolate(x, size=(ho, wo), mode="bilinear", align_corners=True)
    (dx,) = torch.autograd.grad(y, x, dy)
    y64 = R.resize_fwd(x.detach(), ho, wo)
    yabs = R.resize_fwd(x.detach().abs(), ho, wo)
    dx64 = R.resize_adj(dy, hi, wi)
    dxabs = R.resize_adj(dy.abs(), hi, wi)
    rf = float(((y.detach().double() - y64).abs() / (U * yabs).clamp_min(1e-300)).max())
    rb = float(((dx.double() - dx64).abs() / (U * dxabs).clamp_min(1e-300)).max())
    print(f"resize {hi}x{wi}->{ho}x{wo}: ATen fp32 fwd {rf:.2f} u, adjoint {rb:.2f} u")
    assert rf <= 6.0 and rb <= 6.0
    if min(hi, wi, ho, wo) > 8:
        y_d = F.interpolate(x.detach().double(), size=(ho, wo), mode="bilinear", align_corners=True)
        rd = float(((y_d - y64).abs() / (U * yabs).clamp_min(1e-300)).max())
        print(f"    float64 ATen fwd {rd:.0f} u")
        assert rd > 10.0


@pytest.mark.parametrize("n_in,n_out,scale,cmin,cmax", DYADIC)
def test_dyadic_sizes_give_dyadic_weights_and_stated_candidates(n_in, n_out, scale, cmin, cmax):
    assert (n_in - 1) / (n_out - 1) == scale
    Rm = R.resize_matrix(n_in, n_out)
    assert torch.equal(Rm * 32, (Rm * 32).round()), "weights are multiples of 1/32"
    assert torch.equal(Rm.sum(1), torch.ones(n_out, dtype=torch.float64))
    cand = R.candidates(n_in, n_out)
    inner = cand[1:-1]
    assert int(inner.min()) == cmin and int(inner.max()) == cmax, (int(inner.min()), int(inner.max()))
    assert int(cand.max()) == cmax


def test_candidate_counts_of_the_bounded_sizes():
    assert int(R.candidates(51, 100).max()) == 4  # the fourth candidate of resizes growing by almost 2x
    assert int(R.candidates(3, 64).max()) > 12    # the bf16 row kernel's fall-back
    for a, b in [(13, 14), (49, 50), (99, 100), (97, 100)]:
        assert int(R.candidates(a, b).max()) <= 3
    assert int(R.candidates(100, 51).max()) == 1 and int(R.candidates(100, 60).max()) == 2
    assert int(R.candidates(25, 100).max()) == 9  # beyond the near kernel's four slots


@pytest.mark.parametrize("B,C,H,W", [(2, 8, 5, 7), (1, 40, 9, 11)])
def test_sca_ref_matches_oracle_module_without_ties(B, C, H, W):
    from oracle import towerunet_oracle as O

    torch.manual_seed(C)
    mod = O.SpatialChannelAttention(C, "SiLU").double()
    with torch.no_grad():
        mod.gamma.fill_(0.8)
    skip = _rand((B, C, H, W), 1).double().requires_grad_(True)
    out = _rand((B, C, H, W), 2).double().requires_grad_(True)
    dy = _rand((B, C, H, W), 3).double()
    yo = out * mod(skip)
    go = torch.autograd.grad(yo, [skip, out] + [p for p in mod.parameters()], dy)
    s2, o2 = skip.detach().clone().requires_grad_(True), out.detach().clone().requires_grad_(True)
    y, pw = R.sca_ref64(mod, s2, o2)
    y.backward(dy)
    tol = 1e-12
    assert float((y - yo).detach().abs().max()) <= tol * float(yo.detach().abs().max())
    assert float((s2.grad - go[0]).abs().max()) <= tol * float(go[0].abs().max())
    assert float((o2.grad - go[1]).abs().max()) <= tol * float(go[1].abs().max())
    for (n, p), g in zip(mod.named_parameters(), go[2:]):
        assert float((pw[n].grad - g).abs().max()) <= tol * max(float(g.abs().max()), 1e-30), n


def test_sca_ref_tie_rules():
    """amax splits the channel-max gradient evenly; AdaptiveMaxPool2d(1) routes the H*W max to the first maximum."""
    x = torch.tensor([1.0, 2.0, 2.0, 0.0], dtype=torch.float64).view(1, 4, 1, 1).requires_grad_(True)
    x.amax(1).sum().backward()
    assert x.grad.flatten().tolist() == [0.0, 0.5, 0.5, 0.0]
    z = torch.tensor([1.0, 2.0, 2.0, 0.0], dtype=torch.float64).view(1, 1, 2, 2).requires_grad_(True)
    avg, mx, idx, cm, cx = R.sca_pools64(z)
    mx.sum().backward()
    assert z.grad.flatten().tolist() == [0.0, 1.0, 0.0, 0.0] and int(idx) == 1


@pytest.mark.parametrize("crisp,neg", [(1.0, False), (-3.0, True), (0.0, False), (3.0, False)])
def test_final_combine_ref_matches_oracle_module(crisp, neg):
    from oracle import towerunet_oracle as O

    fc = O.TowerUNetFinalCombine().double()
    order = [fc.dist_gamma1, fc.dist_gamma2, fc.dist_gamma3, fc.edge_gamma1, fc.edge_gamma2, fc.edge_gamma3,
             fc.crop_gamma1, fc.crop_gamma2, fc.crop_gamma3, fc.final_dist[0].weight, fc.final_edge[0].weight,
             fc.final_crop[0].weight, fc.final_dist[0].bias, fc.final_edge[0].bias, fc.final_crop[0].bias,
             fc.final_edge[1].gamma]
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in order[:15]:
            p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float64) * 0.5 + 0.75))
        if neg:
            order[4].mul_(-1.0)
        order[15].fill_(crisp)
    hs = [_rand((2, 3, 6, 5), 10 + i).double().requires_grad_(True) for i in range(3)]
    dys = [_rand((2, 1, 6, 5), 20 + i).double() for i in range(3)]
    outs = fc(*[torch.chunk(h, 3, dim=1) for h in hs])
    loss = sum((outs[k] * d).sum() for k, d in zip(("distance", "edge", "crop"), dys))
    go = torch.autograd.grad(loss, hs + order)
    h2 = [h.detach().clone().requires_grad_(True) for h in hs]
    p2 = [p.detach().clone().reshape(()).requires_grad_(True) for p in order]
    o2 = R.final_combine_ref(h2[0], h2[1], h2[2], p2, fc.final_edge[1].smooth)
    for a, k in zip(o2, ("distance", "edge", "crop")):
        assert float((a - outs[k]).detach().abs().max()) <= 1e-14
    g2 = torch.autograd.grad(sum((a * d).sum() for a, d in zip(o2, dys)), h2 + p2)
    for a, b in zip(g2, go):
        assert float((a - b.reshape(a.shape)).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1.0)


def _chips_scalar(scene, r0, c0, T, S, pad, mean, std, scale, lo, hi):
    f = np.float32
    P, H, W = scene.shape
    out = np.zeros((P, S, S), dtype=np.float32)
    for p in range(P):
        m = f(0) if mean is None else f(mean[p // T])
        inv = f(1) if std is None else f(1) / f(std[p // T])
        for y in range(S):
            for x in range(S):
                sy, sx = r0 - pad + y, c0 - pad + x
                v = f(scene[p, sy, sx]) if (0 <= sy < H and 0 <= sx < W) else f(0)
                v = f(v * f(scale))
                v = min(max(v, f(lo)), f(hi))
                out[p, y, x] = f(f(v - m) * inv)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.int16, np.uint16])
def test_window_chips_ref_matches_scalar_loops(dtype):
    rng = np.random.default_rng(3)
    H, W, T, S, pad = 11, 9, 2, 8, 2
    if dtype == np.float32:
        scene = rng.normal(2000, 3000, (4, H, W)).astype(dtype)
    elif dtype == np.uint16:
        scene = rng.integers(0, 65536, (4, H, W)).astype(dtype)
    else:
        scene = rng.integers(-20000, 20000, (4, H, W)).astype(dtype)
    wins = [(0, 0), (8, 4), (4, 8), (10, 8)]
    mean, std = np.array([0.21, 0.3], dtype=np.float32), np.array([0.11, 0.07], dtype=np.float32)
    for m, s in ((mean, std), (None, None)):
        got = R.window_chips_ref(scene, wins, T, S, pad, m, s, 1e-4, 0.0, 1.0)
        for n, (r0, c0) in enumerate(wins):
            want = _chips_scalar(scene, r0, c0, T, S, pad, m, s, 1e-4, 0.0, 1.0)
            assert np.array_equal(got[n].view(np.uint32), want.view(np.uint32))


def test_stitch_ref_matches_scalar_loops():
    rng = np.random.default_rng(4)
    S, pad, ws, H, W, scale = 8, 2, 4, 7, 6, 10000.0
    wins = [(0, 0), (0, 4), (4, 0), (4, 4)]
    maps = [rng.uniform(-0.2, 1.2, (4, S, S)).astype(np.float32) for _ in range(3)]
    maps[1][2, 3, 3] = np.nan
    got = R.stitch_ref(maps[0], maps[1], maps[2], wins, S, pad, ws, H, W, scale)
    want = np.zeros((3, H, W), dtype=np.uint16)
    f = np.float32
    for k in range(3):
        for n, (r0, c0) in enumerate(wins):
            for y in range(min(ws, H - r0)):
                for x in range(min(ws, W - c0)):
                    v = f(maps[k][n, pad + y, pad + x] * f(scale))
                    v = f(0) if np.isnan(v) else min(max(v, f(0)), f(scale))
                    want[k, r0 + y, c0 + x] = int(v)
    assert np.array_equal(got, want)
    assert got[1, 4 + 1, 0 + 1] == 0  # the NaN


@pytest.mark.parametrize("zscore", [True, False])
def test_prepare_chips_ref_distance_from_the_reference_arithmetic(zscore):
    """prepare_chips_ref (the kernel's arithmetic) against the reference's literal torch lines,
    (x / 10000).clip(1e-9, 1) and (. - mean) / std, over the full int16 range under 256 (mean, std) pairs.

    Bit equality with the reference is NOT the contract: the kernel multiplies by the rounded constant 1e-4 and by the
    rounded reciprocal of std, and about a quarter of all values differ from the reference in their last bits. The
    contract is the distance: with u = 2^-24 and v, m, s the clipped value, mean and std in float64,
        |kernel - reference| <= u (3 |v| + 6 |v - m|) / s        (3 u |v| without the z-score),
    from: the rounded 1e-4 and one product against one division (3 u |v| into v, carried through the subtraction),
    one subtraction on each side (2 u |v - m|), the rounded reciprocal and one product against one division
    (3 u |v - m|), and one more u |v - m| for the second-order terms."""
    C = 256
    x = np.broadcast_to(np.arange(-32768, 32768, dtype=np.int16), (1, C, 65536)).copy()
    rng = np.random.default_rng(12)
    mean = (rng.random(C) * 0.5).astype(np.float32) if zscore else None
    std = (rng.random(C) * 0.3 + 0.02).astype(np.float32) if zscore else None
    got = R.prepare_chips_ref(x, mean, std, 1.0 / 10000.0, 1e-9, 1.0)
    xt = torch.from_numpy(x)
    ref = (xt / 10_000.0).clip(1e-9, 1)
    assert ref.dtype == torch.float32
    v = np.clip(x.astype(np.float64) / 10000.0, 1e-9, 1.0)
    if zscore:
        ref = (ref - torch.from_numpy(mean).view(1, C, 1)) / torch.from_numpy(std).view(1, C, 1)
        m, s = mean.astype(np.float64).reshape(1, C, 1), std.astype(np.float64).reshape(1, C, 1)
        bound = U * (3 * np.abs(v) + 6 * np.abs(v - m)) / s
    else:
        bound = 3 * U * np.abs(v)
    ref = ref.numpy()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ratio = float((err / bound).max())
    differ = float((got.view(np.uint32) != ref.view(np.uint32)).mean())
    print(f"BOUND prepare_chips_ref vs reference arithmetic zscore={zscore}: worst err/bound {ratio:.3f} over {got.size} "
          f"values, {100 * differ:.1f} % differ in their bits")
    assert ratio <= 1.0
    if zscore:
        assert differ > 0.0  # the restatement is the kernel's arithmetic, not the reference's


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.int16, np.uint16])
def test_prepare_chips_ref_matches_scalar_loops(dtype):
    """Against a scalar loop of the kernel's statements, mean and std each on its own; NaN clips to lo."""
    f = np.float32
    rng = np.random.default_rng(13)
    if dtype == np.float32:
        x = rng.normal(2000, 6000, (2, 3, 7)).astype(dtype)
        x[0, 1, :5] = [np.nan, np.inf, -np.inf, 0.0, -0.0]
    elif dtype == np.uint16:
        x = rng.integers(0, 65536, (2, 3, 7)).astype(dtype)
    else:
        x = rng.integers(-32768, 32768, (2, 3, 7)).astype(dtype)
    mean, std = np.array([0.21, 0.3, 0.0], dtype=np.float32), np.array([0.11, 0.07, 3.0], dtype=np.float32)
    for m, s in ((mean, std), (mean, None), (None, std), (None, None)):
        got = R.prepare_chips_ref(x, m, s, 1e-4, 1e-9, 1.0)
        want = np.zeros(x.shape, dtype=np.float32)
        for b, c, l in np.ndindex(*x.shape):
            v = f(f(x[b, c, l]) * f(1e-4))
            v = f(1e-9) if np.isnan(v) else min(max(v, f(1e-9)), f(1.0))
            want[b, c, l] = f(f(v - (f(0) if m is None else m[c])) * (f(1) if s is None else f(f(1) / s[c])))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if dtype == np.float32:
        assert R.prepare_chips_ref(x, None, None, 1e-4, 1e-9, 1.0)[0, 1, 0] == f(1e-9)


def _writer_line(stack, scale=10_000.0):
    """callbacks.py:220 on the float32 numpy stack, then the cast of the uint16 raster it is written to."""
    return (stack * scale).clip(0, scale).astype(np.uint16)


def test_predictions_u16_ref_equals_the_reference_writer():
    """array_equal to the reference writer's numpy line on random probabilities around [0, 1], on every k / 10000 and
    on both fp32 neighbours of each; then the slicing: unequal pads, three different maps, three samples."""
    rng = np.random.default_rng(14)
    k = (np.arange(10001) / 10000.0).astype(np.float32)
    values = np.concatenate([rng.uniform(-0.1, 1.1, 1 << 20).astype(np.float32), k, np.nextafter(k, np.float32(-1)),
                             np.nextafter(k, np.float32(2)), np.array([-0.25, 1.5, 7.0, -0.0], dtype=np.float32)])
    n = values.size
    maps = [np.roll(values, s).reshape(1, 1, 1, n) for s in (0, 1, 2)]
    got = R.predictions_u16_ref(maps[0], maps[1], maps[2], 0, 0, 1, n, 10000.0)
    want = np.stack([_writer_line(m.reshape(1, 1, n)) for m in maps], 1)
    assert got.dtype == np.uint16 and got.shape == (1, 3, 1, n) and np.array_equal(got, want)
    assert (got == 10000).any() and (got == 0).any()
    B, H, W, pt, pl, h, w = 3, 17, 19, 3, 5, 12, 14
    maps = [R.count_neighbours(B * H * W, 15 + i).reshape(B, 1, H, W) for i in range(3)]
    got = R.predictions_u16_ref(maps[0], maps[1], maps[2], pt, pl, h, w, 10000.0)
    want = np.stack([_writer_line(m[:, 0, pt:pt + h, pl:pl + w]) for m in maps], 1)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, R.predictions_u16_ref(maps[0], maps[1], maps[2], pl, pt, h, w, 10000.0))
    nan = maps[1].copy()
    nan[2, 0, pt, pl] = np.nan
    assert R.predictions_u16_ref(maps[0], nan, maps[2], pt, pl, h, w, 10000.0)[2, 1, 0, 0] == 0  # as fmaxf


# ---------------------------------------------------------------------------------------------------------------------
# bf16 spatial-channel attention / max pool: the per-element bounds can fail
# ---------------------------------------------------------------------------------------------------------------------
from conv_exact_worker import rb  # noqa: E402


def _flagged(value64, ref, bound, touched, what, need=True):
    """A kernel computing `value64` perfectly (one rounding to bf16) must violate the bound at more than half of the
    elements the change touches."""
    n = int(touched.sum())
    if n == 0:
        assert not need, f"{what}: the mutant changes nothing"
        return None
    frac = float(((rb(value64) - ref).abs() > bound)[touched].double().mean())
    print(f"MUTANT {what}: {100 * frac:.1f} % of {n} touched elements flagged")
    assert frac > 0.5, f"{what}: only {100 * frac:.1f} % of {n} touched elements violate the bound"
    return frac


def _pool_bwd_emulate32(x, davg, dmx, dpool, old):
    """The kernel's order in fp32: davg * fl(1/L), + dm, + dpool0 / C, + dpool1 / n, + old."""
    f = torch.float32
    B, C, H, W = x.shape
    L = H * W
    cx = x.amax(1, keepdim=True)
    tie = x == cx
    n = tie.sum(1, keepdim=True).to(f)
    first = F.adaptive_max_pool2d(x, 1, return_indices=True)[1].view(B, C, 1)
    at = (torch.arange(L).view(1, 1, L) == first).view(B, C, H, W)
    invL = torch.tensor(1.0, dtype=f) / torch.tensor(float(L), dtype=f)
    o = davg.to(f).view(B, C, 1, 1) * invL
    o = o + torch.where(at, dmx.to(f).view(B, C, 1, 1), torch.zeros((), dtype=f))
    o = o + (dpool[:, :1].to(f) / torch.tensor(float(C), dtype=f))
    o = o + torch.where(tie, dpool[:, 1:].to(f) / n, torch.zeros((), dtype=f))
    if old is not None:
        o = o + old.to(f)
    assert o.dtype == f
    return o.double()


@pytest.mark.parametrize("B,C,H,W,ld,few,acc", R.SCA_POOL_BWD_BOUNDED)
def test_sca_pool_bwd_bf16_bound_passes_the_kernel_and_fails_mutants(B, C, H, W, ld, few, acc):
    """D = 7 (+ the accumulate's add): a perfect kernel (float64 rounded once to bf16) and an fp32 emulation of the
    kernel's order pass at every element; leaving out any of the four terms, giving the channel-max gradient to the
    first tied channel only, giving the H*W max to the last maximum, or ignoring `accumulate`, fails at more than half
    of the elements it changes."""
    x, davg, dmx, dpool, base = R.sca_pool_bwd_inputs(B, C, H, W, few, 900 + C + H)
    old = base if acc else None
    g, A = R.sca_pool_bwd_terms64(x, davg, dmx, dpool)
    ref = sum(g) + (base if acc else 0.0)
    bound = R.sca_pool_bwd_bound(ref, A, old)
    what = f"pool bwd {B}x{C}x{H}x{W} few={few} acc={acc}"
    assert bool(((rb(ref) - ref).abs() <= bound).all()), "a perfect kernel fails the bound"
    emu = rb(_pool_bwd_emulate32(x, davg, dmx, dpool, old))
    ratio = float(((emu - ref).abs() / bound).max())
    print(f"BOUND {what} fp32 emulation: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0
    for k, name in enumerate(("H*W average", "H*W max", "channel mean", "channel max")):
        _flagged(ref - g[k], ref, bound, g[k] != 0, f"{what} without the {name}")
    if acc:
        _flagged(ref - base, ref, bound, base != 0, f"{what} ignoring accumulate")
    if not few:
        return  # random x ties by accident at a handful of elements at most: the tie rules are judged on few-valued x
    # channel max to the first tied channel only
    tie = x == x.amax(1, keepdim=True)
    firstc = tie & (tie.cumsum(1) == 1)
    m = ref - g[3] + torch.where(firstc, dpool[:, 1:].expand_as(x), torch.zeros(()).double())
    _flagged(m, ref, bound, m != ref, f"{what} channel max to the first tie")
    # H*W max to the last maximum
    xf = x.flatten(2)
    last = (H * W - 1) - xf.flip(2).argmax(2)
    assert bool((xf.gather(2, last.unsqueeze(2)).squeeze(2) == xf.amax(2)).all())
    glast = torch.zeros_like(xf).scatter_(2, last.unsqueeze(2), dmx.unsqueeze(2)).view_as(x)
    m = ref - g[1] + glast
    _flagged(m, ref, bound, m != ref, f"{what} H*W max to the last maximum")


@pytest.mark.parametrize("B,C,H,W", R.SCA_BF16_POW2)
def test_sca_pool_bwd_bf16_exact_inputs(B, C, H, W):
    """The exact layer's data: 1, 2, 4 or 8 channels at every pixel's maximum (all four occur), ties in the H*W max,
    every float64 dx an integer of at most 256, and the fp32 emulation of the kernel equal to it."""
    x, davg, dmx, dpool, base = R.sca_pool_bwd_exact_inputs(B, C, H, W, 950 + C)
    n = (x == x.amax(1, keepdim=True)).sum(1)
    assert sorted(n.unique().tolist()) == [1, 2, 4, 8]
    assert bool((R.sca_pools64(x)[2] > 0).any()) and bool(((x == x.amax((2, 3), keepdim=True)).sum((2, 3)) > 1).any())
    g, A = R.sca_pool_bwd_terms64(x, davg, dmx, dpool)
    for old in (None, base):
        ref = sum(g) + (0.0 if old is None else old)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= 256 and torch.equal(rb(ref), ref)
        assert torch.equal(_pool_bwd_emulate32(x, davg, dmx, dpool, old), ref)


def _occurrence_rank(idx):
    """Per output of [B,C,Ho,Wo] indices: how many earlier outputs (row-major) of the plane chose the same pixel."""
    B, C = idx.shape[:2]
    flat = idx.flatten(2)
    n = flat.shape[2]
    key = flat * n + torch.arange(n).view(1, 1, n)          # sort by pixel, then by output position
    order = key.argsort(2)
    sp = flat.gather(2, order)
    pos = torch.arange(n).view(1, 1, n).expand(B, C, n)
    start = torch.where(torch.cat([torch.ones(B, C, 1, dtype=torch.bool), sp[:, :, 1:] != sp[:, :, :-1]], 2), pos, 0)
    rank_sorted = pos - start.cummax(2)[0]
    return torch.zeros_like(flat).scatter_(2, order, rank_sorted).view_as(idx)


@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo,ld", R.MAXPOOL_BF16_CASES)
@pytest.mark.parametrize("acc", [0, 1])
def test_maxpool_bwd_bf16_bound_passes_the_kernel_and_fails_the_mutant(B, C, Hi, Wi, Ho, Wo, ld, acc):
    """D = windows per pixel + accumulate on sum |dy| + |old|. A perfect kernel passes; a kernel that drops the
    second window of a pixel that is the first maximum of several fails at more than half of those pixels."""
    x = R.maxpool_inputs(B, C, Hi, Wi, Ho, Wo, 960)
    dy, base = R.bf_randn((B, C, Ho, Wo), 961), R.bf_randn((B, C, Hi, Wi), 962, 0.05)
    y, idx, dx, dxa, cnt = R.maxpool_bwd64(x, dy, (Ho, Wo))
    ref = dx + (base if acc else 0.0)
    bound = R.bf16_store_bound(ref, cnt, dxa) if not acc else R.bf16_store_bound(ref, cnt, dxa, base)
    assert bool(((rb(ref) - ref).abs() <= bound).all())
    overlap = Hi % Ho != 0
    if overlap:
        assert bool((cnt == 2).any()) and bool((cnt == 4).any())
    rank = _occurrence_rank(idx)
    keep = torch.where(rank == 1, torch.zeros_like(dy), dy)
    m = torch.zeros(B, C, Hi * Wi, dtype=torch.float64).scatter_add_(2, idx.flatten(2), keep.flatten(2)).view_as(x)
    assert torch.equal(torch.zeros(B, C, Hi * Wi, dtype=torch.float64).scatter_add_(2, idx.flatten(2), dy.flatten(2))
                       .view_as(x), dx)
    m = m + (base if acc else 0.0)
    _flagged(m, ref, bound, m != ref, f"max pool bwd {Hi}x{Wi}->{Ho}x{Wo} acc={acc} second window dropped",
             need=overlap)


@pytest.mark.parametrize("B,C,H,W,ld", R.SCA_BF16_SHAPES)
@pytest.mark.parametrize("acc", [0, 1])
def test_sca_apply_dout_bf16_bound_passes_the_kernel_and_fails_the_mutant(B, C, H, W, ld, acc):
    """dout = dy (1 + g (ca + sigmoid(sconv))) [+ old]: a perfect kernel passes; one without the sigmoid term fails."""
    dy, base = R.bf_randn((B, C, H, W), 970), R.bf_randn((B, C, H, W), 971, 0.1)
    ca, sconv = torch.sigmoid(R.f32_randn((B, C), 972)).float().double(), R.f32_randn((B, 1, H, W), 973, 2.0)
    gamma = float(torch.tensor(0.9).float())
    g, sa, inner, e_inner, att, mag, e_att = R.sca_att64(ca, sconv, gamma)
    old = base if acc else None
    ref, bound = R.sca_gate_bound(dy, att, mag, e_att, old)
    assert bool(((rb(ref) - ref).abs() <= bound).all())
    m = dy * (1 + g * ca.view(B, C, 1, 1)) + (base if acc else 0.0)
    _flagged(m, ref, bound, m != ref, f"apply dout {B}x{C}x{H}x{W} acc={acc} without sigmoid(sconv)")


def test_sca_ref_paths_sum_to_the_skip_gradient():
    """sca_ref64(paths=True): the four paths' gradients add up to the default form's d skip, y is unchanged."""
    from oracle import towerunet_oracle as O

    torch.manual_seed(3)
    mod = O.SpatialChannelAttention(16, "SiLU").double()
    with torch.no_grad():
        mod.gamma.fill_(0.8)
    skip, out, dy = (_rand((2, 16, 5, 7), s).double() for s in (1, 2, 3))
    s1 = skip.clone().requires_grad_(True)
    y1, pw1 = R.sca_ref64(mod, s1, out)
    y1.backward(dy)
    y2, pw2, leaves = R.sca_ref64(mod, skip, out, paths=True)
    y2.backward(dy)
    assert torch.equal(y1, y2) and len(leaves) == 4 and all(float(l.grad.abs().max()) > 0 for l in leaves)
    tot = sum(l.grad for l in leaves)
    assert float((tot - s1.grad).abs().max()) <= 1e-14 * float(s1.grad.abs().max())
    for n in pw1:
        assert torch.equal(pw1[n].grad, pw2[n].grad) or float((pw1[n].grad - pw2[n].grad).abs().max()) <= 1e-14
