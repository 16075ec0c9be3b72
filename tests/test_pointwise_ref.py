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
