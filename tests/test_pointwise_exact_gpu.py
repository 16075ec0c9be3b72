"""Bilinear resize (fp32 and bf16), the resized ConvTranspose taps pass, fp32 spatial-channel attention, the fp32
adaptive max pool, the fused final-combine head and the predict tiling kernels, through the C ABI, against the float64 /
bit-exact references of tests/pointwise_ref.py. Two layers, as tests/test_conv_exact_gpu.py defines them:

* exact: small-integer data arranged so that every intermediate is representable (the premise is asserted); results
  must EQUAL float64 (bf16 results: float64 rounded to nearest even);
* bounded: random data, per-element bound D * 2^-24 * (the same op on absolute values), D = the fp32 roundings on the
  way to one output, counted from the kernel in each docstring; sigmoid / SiLU cost (|v| + 8) u as stated in
  test_fused_bf16_random_bound; bf16 outputs add half a bf16 ulp. No floors, nothing fitted to what the GPU returns.

Outputs live in NaN- (or sentinel-) filled buffers with strides larger than the tensor and slack behind them, which must
survive; inputs sit in buffers whose gaps hold garbage no result may pick up. Run with -s to read the err/bound ratios.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from conv_exact_worker import (BF, F32, GARB, RED, U32, Canvas, Flat, assert_exact, bounded, half_ulp_bf16, ints, lib,
                               premise, rb, stream, term_bound)
from conv_exact_worker import act_err as _act_err, canary as _canary, dev as _dev, same as _same

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _randn(shape, seed, scale=1.0):
    """fp32-representable N(0, scale^2) values as float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g, dtype=torch.float64) * scale).float().double()


def _few(shape, seed):
    """Integers from five values (-2..2): ties everywhere."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, tuple(shape), generator=g, dtype=torch.int64).double()


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize, fp32
# ---------------------------------------------------------------------------------------------------------------------

def _near_kernel(B, C, Hi, Wi, Ho, Wo):
    """The launcher's choice of cn_bilinear_bwd_near_kernel, restated."""
    return 2 * Hi > Ho and 2 * Wi > Wo and B * C * Hi * Wi >= 1 << 16


def _on_grid(img, Hp, Wp, fill):
    B, C, Hi, Wi = img.shape
    full = torch.full((B, C, Hp, Wp), fill, dtype=torch.float64)
    full[:, :, :Hi, :Wi] = img
    return full


def _cand_map(Hi, Wi, Ho, Wo):
    """Per input pixel: the number of (output row, output column) pairs that read it."""
    return torch.outer(R.candidates(Hi, Ho), R.candidates(Wi, Wo)).double()


def _bilinear_f32(B, C, Hi, Wi, Ho, Wo, exact, grid=(0, 0), seed=0):
    """cn_bilinear_fwd_f32 / cn_bilinear_bwd_f32 (accumulate 0 and 1) on the stored grid `grid` (0, 0: dense).

    Roundings, forward: hx*a, + lx*b, * hy, + the other row = 4 on the way to the output (fewer where the compiler
    fuses), the weights being the reference's own fp32 numbers: D = 4. Adjoint: an input pixel sums its N = ny*nx
    candidates; per term the axis weight (two taps on one index at a clamped border: 1 add per axis = 2), wy*wx (1),
    * dy (1), then at most N adds: D = N + 4, + 1 for the accumulate."""
    dev, L, st = _dev(), lib(), stream()
    Hp, Wp = (grid[0] or Hi), (grid[1] or Wi)
    what = f"bilinear f32 {B}x{C} {Hi}x{Wi}->{Ho}x{Wo} grid {Hp}x{Wp}"
    if exact:
        x, dy, base = ints((B, C, Hi, Wi), -4, 4, seed + 1), ints((B, C, Ho, Wo), -3, 3, seed + 2), \
            ints((B, C, Hp, Wp), -8, 8, seed + 3)
        for a, b in ((Hi, Ho), (Wi, Wo)):
            Rm = R.resize_matrix(a, b)
            assert torch.equal(Rm * 32, (Rm * 32).round()), f"{what}: weights are not multiples of 1/32"
        # every product is a multiple of 1/1024 and every partial sum stays below 2^24 / 1024
        premise(what, 1024 * float(R.resize_fwd(x.abs(), Ho, Wo).max()))
        premise(what + " adjoint", 1024 * (float(R.resize_adj(dy.abs(), Hi, Wi).max()) + 8))
    else:
        x, dy, base = _randn((B, C, Hi, Wi), seed + 1), _randn((B, C, Ho, Wo), seed + 2), _randn((B, C, Hp, Wp), seed + 3)
    y64, dx64 = R.resize_fwd(x, Ho, Wo), R.resize_adj(dy, Hi, Wi)
    xc = Canvas((B, C, Hp, Wp), F32, dev, pitch=C * Hp * Wp + 5, fill=NAN, data=_on_grid(x, Hp, Wp, NAN))
    yc = Canvas((B, C, Ho, Wo), F32, dev, pitch=C * Ho * Wo + 3, fill=NAN)
    L.call("cn_bilinear_fwd_f32", xc.ptr, xc.pitch, yc.ptr, yc.pitch, B, C, Hi, Wi, Ho, Wo, grid[0], grid[1], st)
    torch.cuda.synchronize()
    if exact:
        assert_exact(yc.t, y64, what + " y")
    else:
        bounded(yc.t, y64, 4 * U32 * R.resize_fwd(x.abs(), Ho, Wo), what + " y")
    _canary(yc, what + " y")
    dyc = Canvas((B, C, Ho, Wo), F32, dev, pitch=C * Ho * Wo + 7, fill=GARB, data=dy)
    nmap = _cand_map(Hi, Wi, Ho, Wo)
    for acc in (0, 1):
        dxc = Canvas((B, C, Hp, Wp), F32, dev, pitch=C * Hp * Wp + 9, fill=NAN, data=base if acc else None)
        L.call("cn_bilinear_bwd_f32", dyc.ptr, dyc.pitch, dxc.ptr, dxc.pitch, B, C, Hi, Wi, Ho, Wo, grid[0], grid[1],
               acc, st)
        torch.cuda.synchronize()
        old = base if acc else torch.zeros_like(base)
        ref = old.clone()  # the padding of the stored grid: zeros, or left alone when accumulating
        ref[:, :, :Hi, :Wi] += dx64
        if exact:
            assert_exact(dxc.t, ref, f"{what} dx acc={acc}")
        else:
            bnd = torch.zeros_like(ref)
            bnd[:, :, :Hi, :Wi] = (nmap + 4 + acc) * U32 * (R.resize_adj(dy.abs(), Hi, Wi) + old[:, :, :Hi, :Wi].abs())
            bounded(dxc.t, ref, bnd, f"{what} dx acc={acc}")
        _canary(dxc, f"{what} dx acc={acc}")


# Hi, Wi, Ho, Wo, (B, C) reaching the near-1:1 kernel (or None), largest candidate count per axis
DYADIC = [
    (5, 5, 9, 9, None, 3),
    (4, 4, 5, 5, None, 2),
    (9, 9, 5, 5, None, 1),                # pixels nobody reads
    (25, 25, 97, 97, None, 7),            # the general kernel's wide path
    (37, 37, 65, 65, (3, 17), 4),         # the near kernel's predicated tail
    (49, 49, 65, 65, (2, 17), 3),
    (65, 65, 33, 33, (2, 17), 1),         # "no output reads this pixel"
    (49, 49, 33, 33, (2, 17), 1),
    (1, 6, 4, 1, None, 4),
    (3, 7, 1, 5, None, 1),                # scale 0 on one axis
]


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,big,cmax", DYADIC)
def test_bilinear_f32_exact(Hi, Wi, Ho, Wo, big, cmax):
    """Dyadic scales: all weights are multiples of 1/32, integer data keeps every sum exact. Each size below the
    near-kernel threshold (general kernel) and, where listed, above it with a ragged last 16-channel chunk."""
    cy, cx = R.candidates(Hi, Ho), R.candidates(Wi, Wo)
    assert max(int(cy.max()), int(cx.max())) == cmax, "the case no longer reaches its candidate count"
    if (Hi, Ho) in ((9, 5), (65, 33)):
        assert int(cy.min()) == 0 and int(cx.min()) == 0
    if (Hi, Ho) == (25, 97):
        assert 2 * Hi <= Ho and int(2 * (Ho - 1) / (Hi - 1)) + 2 >= 8  # general kernel, candidate window >= 8 wide
    assert not _near_kernel(2, 3, Hi, Wi, Ho, Wo)
    _bilinear_f32(2, 3, Hi, Wi, Ho, Wo, exact=True, seed=Hi + Wo)
    if big is not None:
        assert _near_kernel(big[0], big[1], Hi, Wi, Ho, Wo) and big[1] % 16 != 0
        _bilinear_f32(big[0], big[1], Hi, Wi, Ho, Wo, exact=True, seed=Hi + Wo + 50)


@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo", [(2, 3, 5, 5, 9, 9), (2, 17, 49, 49, 65, 65), (3, 17, 37, 37, 65, 65)])
def test_bilinear_f32_stored_grid_exact(B, C, Hi, Wi, Ho, Wo):
    """Hp > Hi, Wp > Wi: the forward must not read the (NaN) padding; the adjoint writes it as zeros, and leaves it
    alone when accumulating. Both adjoint kernels."""
    _bilinear_f32(B, C, Hi, Wi, Ho, Wo, exact=True, grid=(Hi + 2, Wi + 3), seed=77)


def test_bilinear_f32_small_stored_grid_is_an_error():
    L, st = lib(), stream()
    t = torch.zeros(4096, device=_dev())
    for name, tail in (("cn_bilinear_fwd_f32", ()), ("cn_bilinear_bwd_f32", (0,))):
        for Hp, Wp in ((4, 5), (5, 4)):
            with pytest.raises(L.HipKernelError):
                L.call(name, t.data_ptr(), 512, t.data_ptr() + 8192, 512, 1, 1, 5, 5, 9, 9, Hp, Wp, *tail, st)
    torch.cuda.synchronize()


# production resizes: B, C (general kernel), B, C reaching the near kernel (or None)
PRODUCTION = [
    (13, 13, 14, 14, None), (49, 49, 50, 50, (2, 17)), (99, 99, 100, 100, (1, 7)), (97, 97, 100, 100, (1, 7)),
    (27, 25, 28, 28, (6, 17)), (51, 51, 100, 100, (2, 17)), (100, 100, 51, 51, (1, 7)), (100, 100, 60, 60, (1, 7)),
    (25, 25, 100, 100, None),
]


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,big", PRODUCTION)
def test_bilinear_f32_random_bound(Hi, Wi, Ho, Wo, big):
    """Random data at the production sizes, forward 4 u, adjoint (N + 4 + accumulate) u per element (see
    _bilinear_f32); 51 -> 100 has four candidates per axis, 25 -> 100 nine."""
    if (Hi, Ho) == (51, 100):
        assert int(R.candidates(51, 100).max()) == 4
    _bilinear_f32(2, 3, Hi, Wi, Ho, Wo, exact=False, seed=Hi + Wo)
    if big is not None:
        assert _near_kernel(big[0], big[1], Hi, Wi, Ho, Wo)
        _bilinear_f32(big[0], big[1], Hi, Wi, Ho, Wo, exact=False, seed=Hi + Wo + 50)


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize, bf16 NHWC
# ---------------------------------------------------------------------------------------------------------------------

def _bilinear_bf16(B, C, Hi, Wi, Ho, Wo, exact, seed=0):
    """cn_bilinear_fwd_bf16 / cn_bilinear_bwd_bf16: the fp32 expressions of the fp32 kernels on bf16 operands (D = 4
    forward, N + 4 (+ 1 accumulating) adjoint, as _bilinear_f32), then ONE rounding to bf16 (the accumulate adds the
    old value in fp32 first)."""
    dev, L, st = _dev(), lib(), stream()
    what = f"bilinear bf16 {B}x{C} {Hi}x{Wi}->{Ho}x{Wo}"
    if exact:
        x, dy, base = ints((B, C, Hi, Wi), -4, 4, seed + 1), ints((B, C, Ho, Wo), -3, 3, seed + 2), \
            ints((B, C, Hi, Wi), -8, 8, seed + 3)
        for a, b in ((Hi, Ho), (Wi, Wo)):
            Rm = R.resize_matrix(a, b)
            assert torch.equal(Rm * 32, (Rm * 32).round()), f"{what}: weights are not multiples of 1/32"
        premise(what, 1024 * float(R.resize_fwd(x.abs(), Ho, Wo).max()))
        premise(what + " adjoint", 1024 * (float(R.resize_adj(dy.abs(), Hi, Wi).max()) + 8))
    else:
        x, dy, base = rb(_randn((B, C, Hi, Wi), seed + 1)), rb(_randn((B, C, Ho, Wo), seed + 2)), \
            rb(_randn((B, C, Hi, Wi), seed + 3))
    y64, dx64 = R.resize_fwd(x, Ho, Wo), R.resize_adj(dy, Hi, Wi)
    xc = Canvas(x.shape, BF, dev, pitch=C + 8, fill=GARB, data=x)
    yc = Canvas(y64.shape, BF, dev, pitch=C + 24, fill=NAN)
    L.call("cn_bilinear_fwd_bf16", xc.ptr, xc.pitch, yc.ptr, yc.pitch, B, C, Hi, Wi, Ho, Wo, st)
    torch.cuda.synchronize()
    if exact:
        assert_exact(yc.t, rb(y64), what + " y")
    else:
        e = 4 * U32 * R.resize_fwd(x.abs(), Ho, Wo)
        bounded(yc.t, y64, e + half_ulp_bf16(y64.abs() + e), what + " y")
    _canary(yc, what + " y")
    dyc = Canvas(dy.shape, BF, dev, pitch=C + 16, fill=GARB, data=dy)
    nmap = _cand_map(Hi, Wi, Ho, Wo)
    for acc in (0, 1):
        dxc = Canvas(x.shape, BF, dev, pitch=C + 8, fill=NAN, data=base if acc else None)
        L.call("cn_bilinear_bwd_bf16", dyc.ptr, dyc.pitch, dxc.ptr, dxc.pitch, B, C, Hi, Wi, Ho, Wo, acc, st)
        torch.cuda.synchronize()
        old = base if acc else torch.zeros_like(base)
        ref = dx64 + old
        if exact:
            assert_exact(dxc.t, rb(ref), f"{what} dx acc={acc}")
        else:
            e = (nmap + 4 + acc) * U32 * (R.resize_adj(dy.abs(), Hi, Wi) + old.abs())
            bounded(dxc.t, ref, e + half_ulp_bf16(ref.abs() + e), f"{what} dx acc={acc}")
        _canary(dxc, f"{what} dx acc={acc}")


@pytest.mark.parametrize("Hi,Wi,Ho,Wo,big,cmax", DYADIC)
def test_bilinear_bf16_exact(Hi, Wi, Ho, Wo, big, cmax):
    assert max(int(R.candidates(Hi, Ho).max()), int(R.candidates(Wi, Wo).max())) == cmax
    _bilinear_bf16(2, 8, Hi, Wi, Ho, Wo, exact=True, seed=Hi + Wo)
    if big is not None:
        _bilinear_bf16(1, 24, Hi, Wi, Ho, Wo, exact=True, seed=Hi + Wo + 50)


# the case list of test_bf16_kernels_gpu.py::test_bilinear_bf16: the row kernels and their element-wise fall-backs
# (Wi > 256; more than 12 candidates per axis at 3 -> 64)
@pytest.mark.parametrize("case", [(2, 16, 13, 13, 14, 14), (1, 32, 49, 49, 50, 50), (2, 8, 97, 97, 100, 100),
                                  (1, 8, 25, 25, 25, 25), (2, 16, 7, 9, 20, 23), (1, 8, 40, 40, 13, 17),
                                  (2, 32, 25, 25, 100, 100), (1, 16, 13, 13, 100, 100), (1, 8, 100, 100, 25, 25),
                                  (1, 8, 5, 300, 9, 310), (1, 8, 1, 6, 4, 1), (1, 8, 3, 3, 64, 64),
                                  (1, 8, 4, 260, 6, 500), (1, 16, 51, 51, 100, 100)])
def test_bilinear_bf16_random_bound(case):
    B, C, Hi, Wi, Ho, Wo = case
    if (Hi, Ho) == (3, 64):
        assert int(R.candidates(3, 64).max()) > 12
    _bilinear_bf16(B, C, Hi, Wi, Ho, Wo, exact=False, seed=Hi + Wo)


def _engine_tape(fn, x, dy, bf16):
    """fn(Var) under the tape on an fp32 NCHW or bf16 NHWC Var; returns y, dx (CPU float64)."""
    from cultionet_amd import engine as E

    dev = _dev()
    mk = (lambda t: Canvas(t.shape, BF, dev, data=t).t) if bf16 else (lambda t: t.float().to(dev).contiguous())
    with E.recording(True) as tape:
        xv = E.Var(mk(x), True)
        yv = fn(xv)
        yv.grad = mk(dy)
        tape.backward()
    torch.cuda.synchronize()
    assert yv.t.dtype == (BF if bf16 else F32)
    return yv.t.detach().double().cpu(), xv.grad.detach().double().cpu()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("B,C,Hi,Ho", [(1, 8, 5, 9), (2, 24, 49, 65)])
def test_resize_bilinear_engine_exact(B, C, Hi, Ho, bf16):
    """engine.resize_bilinear picks the fp32 or the bf16 kernels by the Var's type (and, at [2, 24, 49, 49], the fp32
    near-1:1 adjoint): dyadic sizes, integer data, results equal float64 (rounded to bf16 for bf16 Vars)."""
    from cultionet_amd import engine as E

    assert _near_kernel(B, C, Hi, Hi, Ho, Ho) == (Hi == 49)
    x, dy = ints((B, C, Hi, Hi), -4, 4, 380), ints((B, C, Ho, Ho), -3, 3, 381)
    premise("resize engine", 1024 * float(R.resize_adj(dy.abs(), Hi, Hi).max()))
    y, dx = _engine_tape(lambda v: E.resize_bilinear(v, (Ho, Ho)), x, dy, bf16)
    rnd = rb if bf16 else (lambda t: t)
    assert_exact(y, rnd(R.resize_fwd(x, Ho, Ho)), "y")
    assert_exact(dx, rnd(R.resize_adj(dy, Hi, Hi)), "dx")


# ---------------------------------------------------------------------------------------------------------------------
# ConvTranspose taps pass with a resize behind it
# ---------------------------------------------------------------------------------------------------------------------
K, S4, PAD = 3, 4, 1  # final_c's ConvTranspose2d(k 3, stride 4, padding 1)


def _tap_index(Hc, Hy):
    """(ky, a, p) of every tap of one axis that lands inside the natural output: p = 4 a - 1 + ky."""
    return [(ky, a, S4 * a - PAD + ky) for ky in range(K) for a in range(Hc) if 0 <= S4 * a - PAD + ky < Hy]


def _taps_scatter(P, bias, C, Hc, Wc):
    """bias + scatter(P): [B][C][Hy][Wy] float64."""
    B = P.shape[0]
    Hy, Wy = (Hc - 1) * S4 - 2 * PAD + K, (Wc - 1) * S4 - 2 * PAD + K
    Y = bias.view(1, C, 1, 1).expand(B, C, Hy, Wy).clone()
    P6 = P.view(B, C, K, K, Hc, Wc)
    for ky, a, p in _tap_index(Hc, Hy):
        for kx, b, q in _tap_index(Wc, Wy):
            Y[:, :, p, q] += P6[:, :, ky, kx, a, b]
    return Y


def _taps_gather(G, C, Hc, Wc):
    """The adjoint of the scatter: dP [B][C*K*K][Hc][Wc] (taps outside the natural output get 0)."""
    B, _, Hy, Wy = G.shape
    dP = torch.zeros(B, C, K, K, Hc, Wc, dtype=torch.float64)
    for ky, a, p in _tap_index(Hc, Hy):
        for kx, b, q in _tap_index(Wc, Wy):
            dP[:, :, ky, kx, a, b] = G[:, :, p, q]
    return dP.view(B, C * K * K, Hc, Wc)


def _taps(B, C, Hc, Wc, Ho, Wo, exact, seed):
    """cn_convt_taps_fwd_f32 / cn_convt_taps_bwd_f32 with (Ho, Wo) != the natural size. Forward: P + bias (1), then
    the four roundings of the bilinear forward: D = 5. Adjoint: dP = resize_matrix^T dz gathered at the tap
    positions, the weights and sums of the bilinear adjoint: D = N + 4 with N = ny*nx candidates of the tap's pixel."""
    dev, L, st = _dev(), lib(), stream()
    Hy, Wy = (Hc - 1) * S4 - 2 * PAD + K, (Wc - 1) * S4 - 2 * PAD + K
    what = f"taps {B}x{C} {Hc}x{Wc} natural {Hy}x{Wy} -> {Ho}x{Wo}"
    if exact:
        P, bias, dz = ints((B, C * K * K, Hc, Wc), -4, 4, seed), ints((C,), -8, 8, seed + 1), \
            ints((B, C, Ho, Wo), -3, 3, seed + 2)
        for a, b in ((Hy, Ho), (Wy, Wo)):
            Rm = R.resize_matrix(a, b)
            assert torch.equal(Rm * 32, (Rm * 32).round()), f"{what}: weights are not multiples of 1/32"
        premise(what, 1024 * 12.0)
        premise(what + " adjoint", 1024 * float(R.resize_adj(dz.abs(), Hy, Wy).max()))
    else:
        P, bias, dz = _randn((B, C * K * K, Hc, Wc), seed), _randn((C,), seed + 1), _randn((B, C, Ho, Wo), seed + 2)
    z64 = R.resize_fwd(_taps_scatter(P, bias, C, Hc, Wc), Ho, Wo)
    dP64 = _taps_gather(R.resize_adj(dz, Hy, Wy), C, Hc, Wc)
    per = C * K * K * Hc * Wc
    pc = Flat((B, per + 6), dev, fill=GARB)
    pc.t[:, :per].copy_(P.reshape(B, per).float())
    bd = bias.float().to(dev)
    zc = Canvas((B, C, Ho, Wo), F32, dev, pitch=C * Ho * Wo + 3, fill=NAN)
    L.call("cn_convt_taps_fwd_f32", pc.ptr, per + 6, bd.data_ptr(), zc.ptr, zc.pitch, B, C, Hc, Wc, K, S4, PAD, Ho, Wo,
           st)
    torch.cuda.synchronize()
    if exact:
        assert_exact(zc.t, z64, what + " z")
    else:
        zabs = R.resize_fwd(_taps_scatter(P.abs(), bias.abs(), C, Hc, Wc), Ho, Wo)
        bounded(zc.t, z64, 5 * U32 * zabs, what + " z")
    _canary(zc, what + " z")
    dzc = Canvas((B, C, Ho, Wo), F32, dev, pitch=C * Ho * Wo + 5, fill=GARB, data=dz)
    dpc = Canvas((B, C * K * K, Hc, Wc), F32, dev, pitch=per + 7, fill=NAN)
    L.call("cn_convt_taps_bwd_f32", dzc.ptr, dzc.pitch, dpc.ptr, dpc.pitch, B, C, Hc, Wc, K, S4, PAD, Ho, Wo, st)
    torch.cuda.synchronize()
    if exact:
        assert_exact(dpc.t, dP64, what + " dP")
    else:
        n = _cand_map(Hy, Wy, Ho, Wo).expand(B, C, Hy, Wy)
        bnd = _taps_gather((n + 4) * U32 * R.resize_adj(dz.abs(), Hy, Wy), C, Hc, Wc)
        bounded(dpc.t, dP64, bnd, what + " dP")
    _canary(dpc, what + " dP")


@pytest.mark.parametrize("B,C,Hc,Wc,size", [(2, 17, 7, 7, 33), (1, 3, 7, 4, 33)])
def test_convt_taps_resized_exact(B, C, Hc, Wc, size):
    """Natural size 25 (Hc = 7) resized to 33: scale 24/32, dyadic weights; forward and adjoint equal float64."""
    if Wc == 7:
        assert ((Hc - 1) * S4 - 2 * PAD + K - 1) / (size - 1) == 0.75
    Wo = size if Wc == 7 else 17  # natural width 13 -> 17: scale 12/16
    _taps(B, C, Hc, Wc, size, Wo, exact=True, seed=300 + C)


@pytest.mark.parametrize("B,C,Hc,Wc,size", [(1, 5, 25, 25, 100), (2, 17, 7, 7, 30)])
def test_convt_taps_resized_random_bound(B, C, Hc, Wc, size):
    _taps(B, C, Hc, Wc, size, size, exact=False, seed=320 + C)


def test_convt_taps_adjoint_refuses_2x_resizes():
    """An input pixel has at most four candidates per axis only below 2x: 25 -> 50 and beyond is an argument error."""
    L, st = lib(), stream()
    t = torch.zeros(1 << 16, device=_dev())
    for Ho, Wo in ((50, 33), (33, 50), (64, 64)):
        with pytest.raises(L.HipKernelError):
            L.call("cn_convt_taps_bwd_f32", t.data_ptr(), 0, t.data_ptr(), 0, 1, 1, 7, 7, K, S4, PAD, Ho, Wo, st)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 spatial-channel attention: pools
# ---------------------------------------------------------------------------------------------------------------------

def _sca_pool_fwd(x, dev, pad=11):
    B, C, H, W = x.shape
    Lp = H * W
    xc = Canvas(x.shape, F32, dev, pitch=C * Lp + pad, fill=GARB, data=x)
    avg, mx, pooled = Flat((B, C), dev), Flat((B, C), dev), Flat((B, 2, H, W), dev)
    idx = Flat((B, C), dev, fill=-7, dtype=torch.int32)
    cnt = Flat((B, H, W), dev, fill=-7, dtype=torch.int32)
    lib().call("cn_sca_pool_fwd_f32", xc.ptr, xc.pitch, B, C, Lp, avg.ptr, mx.ptr, idx.ptr, pooled.ptr, cnt.ptr, stream())
    torch.cuda.synchronize()
    for f, n in ((avg, "avg"), (mx, "mx"), (pooled, "pooled"), (idx, "idx"), (cnt, "ccnt")):
        f.assert_slack(n)
    return xc, avg, mx, idx, pooled, cnt


@pytest.mark.parametrize("B,C,H,W", [(2, 6, 3, 5), (2, 5, 25, 25), (1, 7, 33, 33)])
def test_sca_pool_fwd_f32_few_valued(B, C, H, W):
    """Five-valued integer data: ties in both maxima. The sums are exact integers, so avg and the channel mean differ
    from float64 by their one division (D = 1); max, idx (first maximum, as nn.AdaptiveMaxPool2d), the channel max and
    the tie count are equal."""
    x = _few((B, C, H, W), 400 + H)
    premise("sca pool sums", 2.0 * max(C, H * W))
    _, avg, mx, idx, pooled, cnt = _sca_pool_fwd(x, _dev())
    ravg, rmx, ridx, rcm, rcx = R.sca_pools64(x)
    bounded(avg.t, ravg, U32 * ravg.abs(), "avg")
    bounded(pooled.t[:, 0], rcm, U32 * rcm.abs(), "channel mean")
    assert_exact(mx.t, rmx, "mx")
    assert torch.equal(idx.t.cpu().long(), ridx), "idx (first maximum)"
    assert_exact(pooled.t[:, 1], rcx, "channel max")
    ties = (x == rcx.unsqueeze(1)).sum(1)
    assert torch.equal(cnt.t.cpu().long(), ties), "tie count"
    assert bool((ties > 1).any()) and bool((ridx > 0).any())  # ties really occurred, in both maxima


@pytest.mark.parametrize("B,C,H,W", [(2, 40, 9, 11), (1, 3, 33, 33)])
def test_sca_pool_fwd_f32_random_bound(B, C, H, W):
    """avg: a thread adds ceil(L / 256) values, cn_block_sum adds 9 levels, one division: D = ceil(L/256) + 10.
    Channel mean: C sequential adds and the division: D = C + 1. The maxima are exact."""
    x = _randn((B, C, H, W), 410 + H)
    _, avg, mx, idx, pooled, cnt = _sca_pool_fwd(x, _dev())
    ravg, rmx, ridx, rcm, rcx = R.sca_pools64(x)
    Lp = H * W
    bounded(avg.t, ravg, (math.ceil(Lp / 256) + RED + 1) * U32 * x.abs().mean((2, 3)), "avg")
    bounded(pooled.t[:, 0], rcm, (C + 1) * U32 * x.abs().mean(1), "channel mean")
    assert_exact(mx.t, rmx, "mx")
    assert torch.equal(idx.t.cpu().long(), ridx)
    assert_exact(pooled.t[:, 1], rcx, "channel max")
    assert bool((cnt.t == 1).all())


def test_sca_pool_fwd_f32_nan_and_minus_inf():
    """A NaN wins both maxima (ATen, and the bf16 kernels) and keeps its index; a plane of -inf has its first pixel
    as the maximum."""
    B, C, H, W = 2, 4, 17, 19  # L = 323: the planted values sit in a thread's second iteration
    x = _randn((B, C, H, W), 420)
    x[0, 1, 16, 5] = NAN
    x[1, 2] = -math.inf
    _, avg, mx, idx, pooled, cnt = _sca_pool_fwd(x, _dev())
    ravg, rmx, ridx, rcm, rcx = R.sca_pools64(x)
    assert math.isnan(float(rmx[0, 1])) and int(ridx[0, 1]) == 16 * W + 5 and math.isnan(float(rcx[0, 16, 5]))
    _same(mx.t, rmx, "mx")
    assert torch.equal(idx.t.cpu().long(), ridx), "idx"
    _same(pooled.t[:, 1], rcx, "channel max")
    got_avg, got_cm = avg.t.cpu().double(), pooled.t[:, 0].cpu().double()
    assert math.isnan(float(got_avg[0, 1])) and float(got_avg[1, 2]) == -math.inf
    assert math.isnan(float(got_cm[0, 16, 5])) and bool((got_cm[1] == -math.inf).all())
    fin = ravg.isfinite()
    assert bool(((got_avg - ravg).abs()[fin] <= (2 + RED + 1) * U32 * x.abs().mean((2, 3))[fin]).all())
    # an all -inf pixel: every channel ties at the maximum
    x2 = _randn((1, 3, 2, 3), 421)
    x2[0, :, 1, 1] = -math.inf
    _, _, _, _, pooled2, cnt2 = _sca_pool_fwd(x2, _dev())
    assert float(pooled2.t[0, 1, 1, 1]) == -math.inf and int(cnt2.t[0, 1, 1]) == 3


def _sca_pool_bwd(x, davg, dmx, dpool, base, accumulate):
    """cn_sca_pool_bwd_f32 after its own forward; returns dx [B,C,H,W] (CPU float64)."""
    dev = _dev()
    B, C, H, W = x.shape
    xc, avg, mx, idx, pooled, cnt = _sca_pool_fwd(x, dev)
    g = [t.float().to(dev).contiguous() for t in (davg, dmx, dpool)]
    dxc = Canvas(x.shape, F32, dev, pitch=C * H * W + 13, fill=NAN, data=base if accumulate else None)
    lib().call("cn_sca_pool_bwd_f32", xc.ptr, xc.pitch, g[0].data_ptr(), g[1].data_ptr(), idx.ptr, pooled.ptr,
               g[2].data_ptr(), cnt.ptr, dxc.ptr, dxc.pitch, B, C, H * W, accumulate, stream())
    torch.cuda.synchronize()
    _canary(dxc, "sca pool dx")
    return dxc.t.cpu().double()


def _sca_pool_bwd_ref(x, davg, dmx, dpool):
    """float64 autograd of the four pools (and the same on absolute values, term by term, for the bound)."""
    grads, asum = R.sca_pool_bwd_terms64(x, davg, dmx, dpool)
    return sum(grads), asum


@pytest.mark.parametrize("B,C,H,W", [(2, 6, 3, 5), (2, 5, 25, 25), (1, 7, 33, 33)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_sca_pool_bwd_f32_exact(B, C, H, W, accumulate):
    """Five-valued x (ties), gradients chosen so that every division is exact: davg a multiple of L, the channel-mean
    gradient a multiple of C, the channel-max gradient a multiple of lcm(1..C) -- the even split among tied channels
    (torch.amax) then stays an integer. dx equals float64 autograd."""
    Lp = H * W
    x = _few((B, C, H, W), 430 + H)
    lcm = math.lcm(*range(1, C + 1))
    davg, dmx = ints((B, C), -3, 3, 431) * Lp, ints((B, C), -3, 3, 432)
    dpool = torch.stack([ints((B, H, W), -3, 3, 433) * C, ints((B, H, W), -3, 3, 434, zeros=0.0) * lcm], 1)
    base = ints((B, C, H, W), -8, 8, 435)
    premise("sca pool bwd", 3 + 3 + 3 + 3 * lcm + 8)
    ref, _ = _sca_pool_bwd_ref(x, davg, dmx, dpool)
    assert bool(((x == x.amax(1, keepdim=True)).sum(1) > 1).any())
    assert torch.equal(ref, ref.round()), "the reference gradient is an integer"
    got = _sca_pool_bwd(x, davg, dmx, dpool, base, accumulate)
    assert_exact(got, ref + (base if accumulate else 0), "dx")


@pytest.mark.parametrize("few", [True, False])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_sca_pool_bwd_f32_random_bound(few, accumulate):
    """Random gradients: three divisions (1 each) and three adds on the way to dx, one more when accumulating:
    D = 4 (+ 1) on the sum of the absolute terms."""
    B, C, H, W = 2, 6, 25, 25
    x = _few((B, C, H, W), 440) if few else _randn((B, C, H, W), 440)
    davg, dmx, dpool = _randn((B, C), 441, 4.0), _randn((B, C), 442, 4.0), _randn((B, 2, H, W), 443)
    base = _randn((B, C, H, W), 444)
    ref, aref = _sca_pool_bwd_ref(x, davg, dmx, dpool)
    got = _sca_pool_bwd(x, davg, dmx, dpool, base, accumulate)
    old = base if accumulate else torch.zeros_like(base)
    bounded(got, ref + old, (4 + accumulate) * U32 * (aref + old.abs()), f"sca pool dx few={few} acc={accumulate}")


# ---------------------------------------------------------------------------------------------------------------------
# fp32 spatial-channel attention: channel MLPs
# ---------------------------------------------------------------------------------------------------------------------

def _mlp_inputs(B, C, seed):
    Ch = C // 2
    w = lambda shape, fan, s: _randn(shape, s, fan ** -0.5)
    return dict(va=_randn((B, C), seed), vm=_randn((B, C), seed + 1).abs(), w1a=w((Ch, C), C, seed + 2),
                w2a=w((C, Ch), Ch, seed + 3), w1m=w((Ch, C), C, seed + 4), w2m=w((C, Ch), Ch, seed + 5))


def _mlp_fwd64(p):
    """hpre_a, hpre_m, ca in float64 with their error bounds: C fused multiply-adds per first-layer output ((C + 4) u
    on |W1||v|), SiLU, Ch per second-layer sum and the add of the two branches ((Ch + 4) u), sigmoid."""
    C, Ch = p["va"].shape[1], p["w1a"].shape[0]
    out = {}
    z, e_z = 0.0, 0.0
    for br, v, w1, w2 in (("a", p["va"], p["w1a"], p["w2a"]), ("m", p["vm"], p["w1m"], p["w2m"])):
        h = v @ w1.t()
        e_h = (C + 4) * U32 * (v.abs() @ w1.abs().t())
        a = F.silu(h)
        e_a = _act_err(h, e_h, a)
        z = z + a @ w2.t()
        e_z = e_z + (Ch + 4) * U32 * ((a.abs() + e_a) @ w2.abs().t()) + e_a @ w2.abs().t()
        out["h" + br], out["e_h" + br] = h, e_h
    ca = torch.sigmoid(z)
    out["ca"], out["e_ca"] = ca, 0.25 * e_z + (z.abs() + e_z + 8) * U32 * ca
    return out


@pytest.mark.parametrize("C", [40, 128, 320, 520])
def test_sca_mlp_fwd_f32_random_bound(C):
    """C = 520 gives Ch = 260: both strided loops of the kernel (c += 256, j += 256) iterate twice (three times)."""
    dev, L, st = _dev(), lib(), stream()
    B, Ch = 3, C // 2
    p = _mlp_inputs(B, C, 450 + C)
    r = _mlp_fwd64(p)
    d = {k: v.float().to(dev).contiguous() for k, v in p.items()}
    ha, hm, ca = Flat((B, Ch), dev), Flat((B, Ch), dev), Flat((B, C), dev)
    L.call("cn_sca_mlp_fwd_f32", d["va"].data_ptr(), d["vm"].data_ptr(), d["w1a"].data_ptr(), d["w2a"].data_ptr(),
           d["w1m"].data_ptr(), d["w2m"].data_ptr(), ha.ptr, hm.ptr, ca.ptr, B, C, Ch, st)
    torch.cuda.synchronize()
    bounded(ha.t, r["ha"], r["e_ha"], f"mlp hpre_a C={C}")
    bounded(hm.t, r["hm"], r["e_hm"], f"mlp hpre_m C={C}")
    bounded(ca.t, r["ca"], r["e_ca"], f"mlp ca C={C}")
    for f, n in ((ha, "hpre_a"), (hm, "hpre_m"), (ca, "ca")):
        f.assert_slack(n)


def _silu_grad64(h):
    s = torch.sigmoid(h)
    return s * (1 + h * (1 - s))


@pytest.mark.parametrize("C", [40, 128, 320, 520])
def test_sca_mlp_bwd_f32_random_bound(C):
    """cn_sca_mlp_bwd_f32 on the float64 forward's hpre / ca rounded to fp32, against float64 autograd.

    d pre = d ca * a * (1 - a): 3 roundings, and the rounding of the stored a (u a) moves it by at most u |d ca| a.
    h = SiLU(hpre): the activation term, plus 1.1 u |hpre| for the stored hpre's rounding; SiLU' = s (1 + x (1 - s)):
    the sigmoid's (|x| + 8) u s carried through |d/ds| <= 1 + 3 |x|, four more roundings, and |SiLU''| <= 1/2 times
    u |hpre| for the stored value.
    dW2 = sum_b d pre h (one product, B atomic adds onto the prefill: B + 1 roundings), dh = W2^T d pre (C + 4),
    dh *= SiLU' (1), dW1 = sum_b dh v (B + 1), dv = W1^T dh (Ch + 4)."""
    dev, L, st = _dev(), lib(), stream()
    B, Ch = 3, C // 2
    p = _mlp_inputs(B, C, 470 + C)
    r = _mlp_fwd64(p)
    dca = _randn((B, C), 480 + C)
    names = ("w1a", "w2a", "w1m", "w2m")
    pre = {k: _randn(p[k].shape, 490 + i) for i, k in enumerate(names)}  # prefill of the accumulated gradients
    h32 = {"a": r["ha"].float().double(), "m": r["hm"].float().double()}
    ca32 = r["ca"].float().double()
    # float64 autograd
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    mlp = lambda v, w1, w2: F.silu(v @ w1.t()) @ w2.t()
    ca64 = torch.sigmoid(mlp(leaves["va"], leaves["w1a"], leaves["w2a"]) + mlp(leaves["vm"], leaves["w1m"], leaves["w2m"]))
    keys = ("w1a", "w2a", "w1m", "w2m", "va", "vm")
    g64 = dict(zip(keys, torch.autograd.grad((ca64 * dca).sum(), [leaves[k] for k in keys])))
    # bounds
    dpre = dca * ca32 * (1 - ca32)
    e_dpre = 3 * U32 * dpre.abs() + U32 * dca.abs() * ca32
    bnd = {}
    for br, v, w1, w2 in (("a", p["va"], p["w1a"], p["w2a"]), ("m", p["vm"], p["w1m"], p["w2m"])):
        h = h32[br]
        a = F.silu(h)
        e_a = (h.abs() + 8) * U32 * a.abs() + 1.1 * U32 * h.abs()
        s = torch.sigmoid(h)
        gr = _silu_grad64(h)
        e_gr = (1 + 3 * h.abs()) * (h.abs() + 8) * U32 * s + 4 * U32 * s * (1 + h.abs()) + 0.5 * U32 * h.abs()
        t2 = dpre.abs().t() @ a.abs()                                             # [C][Ch] sum_b |d pre| |h|
        bnd["w2" + br] = e_dpre.t() @ a.abs() + dpre.abs().t() @ e_a + (B + 2) * U32 * (t2 + pre["w2" + br].abs())
        dh_ = dpre @ w2                                                           # [B][Ch]
        e_dh_ = (C + 4) * U32 * (dpre.abs() @ w2.abs()) + e_dpre @ w2.abs()
        dh = dh_ * gr
        e_dh = gr.abs() * e_dh_ + dh_.abs() * e_gr + e_dh_ * e_gr + U32 * dh.abs()
        t1 = dh.abs().t() @ v.abs()                                               # [Ch][C]
        bnd["w1" + br] = e_dh.t() @ v.abs() + (B + 2) * U32 * (t1 + pre["w1" + br].abs())
        bnd["v" + br] = (Ch + 4) * U32 * ((dh.abs() + e_dh) @ w1.abs()) + e_dh @ w1.abs()
    d = {k: v.float().to(dev).contiguous() for k, v in p.items()}
    dv = {"ha": h32["a"], "hm": h32["m"], "ca": ca32, "dca": dca}
    dv = {k: v.float().to(dev).contiguous() for k, v in dv.items()}
    gw = {k: Flat(p[k].shape, dev, data=pre[k]) for k in names}
    davg, dmx = Flat((B, C), dev), Flat((B, C), dev)
    L.call("cn_sca_mlp_bwd_f32", d["va"].data_ptr(), d["vm"].data_ptr(), d["w1a"].data_ptr(), d["w2a"].data_ptr(),
           d["w1m"].data_ptr(), d["w2m"].data_ptr(), dv["ha"].data_ptr(), dv["hm"].data_ptr(), dv["ca"].data_ptr(),
           dv["dca"].data_ptr(), gw["w1a"].ptr, gw["w2a"].ptr, gw["w1m"].ptr, gw["w2m"].ptr, davg.ptr, dmx.ptr, B, C, Ch,
           st)
    torch.cuda.synchronize()
    for k in names:
        bounded(gw[k].t, g64[k] + pre[k].float().double(), bnd[k], f"mlp d{k} C={C}")
        gw[k].assert_slack(k)
    bounded(davg.t, g64["va"], bnd["va"], f"mlp davg C={C}")
    bounded(dmx.t, g64["vm"], bnd["vm"], f"mlp dmx C={C}")
    davg.assert_slack("davg")
    dmx.assert_slack("dmx")


def test_sca_mlp_f32_refuses_more_than_1024_channels():
    L, st = lib(), stream()
    C, Ch = 1040, 520
    t = torch.zeros(C * Ch, device=_dev())
    a = [t.data_ptr()] * 9
    with pytest.raises(L.HipKernelError):
        L.call("cn_sca_mlp_fwd_f32", *a, 1, C, Ch, st)
    with pytest.raises(L.HipKernelError):
        L.call("cn_sca_mlp_bwd_f32", *([t.data_ptr()] * 16), 1, C, Ch, st)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 spatial-channel attention: apply
# ---------------------------------------------------------------------------------------------------------------------

_att64 = R.sca_att64


@pytest.mark.parametrize("B,C,H,W,gamma", [(2, 5, 25, 25, 0.9), (1, 3, 33, 33, -0.7), (2, 6, 3, 5, 0.9)])
def test_sca_apply_f32_random_bound(B, C, H, W, gamma):
    """y = out * att: one more product. Backward: d out = dy * att (+ old: 1); d ca = g sum_l dy out: a product, a
    thread's ceil(L / 256) adds, cn_block_sum's 9, the product with g: D = ceil(L/256) + 11; d sconv = g sa (1 - sa)
    sum_c dy out: C fused multiply-adds, then 1 - sa and three products, D = C + 4 on sum |dy out|, the sigmoid's error
    through |d/ds s(1-s)| <= 1; d gamma = prefill + sum_{b,c} 0.5 sum_l dy out (a + sa): per term two products and
    the error of a + sa, the block's sums as for d ca, cn_sca_sum_kernel's ceil(BC / 256) + 9 adds and the add onto
    the prefill."""
    dev, L, st = _dev(), lib(), stream()
    Lp = H * W
    out, dy = _randn((B, C, H, W), 500), _randn((B, C, H, W), 501)
    ca, sconv = torch.sigmoid(_randn((B, C), 502)).float().double(), _randn((B, 1, H, W), 503, 2.0)
    base = _randn((B, C, H, W), 504)
    g, sa, inner, e_inner, att, mag, e_att = _att64(ca, sconv, gamma)
    oc = Canvas(out.shape, F32, dev, pitch=C * Lp + 7, fill=GARB, data=out)
    dyc = Canvas(dy.shape, F32, dev, pitch=C * Lp + 9, fill=GARB, data=dy)
    yc = Canvas(out.shape, F32, dev, pitch=C * Lp + 5, fill=NAN)
    cad, sd = ca.float().to(dev), sconv.float().to(dev).contiguous()
    gd = torch.tensor([gamma], dtype=torch.float64).float().to(dev)
    gamma = float(gd.double().cpu())
    g, sa, inner, e_inner, att, mag, e_att = _att64(ca, sconv, gamma)
    L.call("cn_sca_apply_fwd_f32", oc.ptr, oc.pitch, cad.data_ptr(), sd.data_ptr(), gd.data_ptr(), yc.ptr, yc.pitch, B, C,
           Lp, st)
    torch.cuda.synchronize()
    bounded(yc.t, out * att, out.abs() * e_att + U32 * out.abs() * (mag + e_att), "sca apply y")
    _canary(yc, "sca apply y")
    t = dy * out
    n_l = math.ceil(Lp / 256) + RED
    ref_dca = g * t.sum((2, 3))
    b_dca = (n_l + 2) * U32 * abs(g) * t.abs().sum((2, 3))
    ssum = t.sum(1, keepdim=True)
    ref_ds = g * sa * (1 - sa) * ssum
    b_ds = abs(g) * ((C + 4) * U32 * sa * (1 - sa) * t.abs().sum(1, keepdim=True) + (sconv.abs() + 8) * U32 * sa * ssum.abs())
    ref_dg = 0.5 * (t * inner).sum()
    n_bc = math.ceil(B * C / 256) + RED
    b_dg = 0.5 * float((t.abs() * e_inner).sum()) + (n_l + n_bc + 4) * U32 * (0.5 * float((t.abs() * inner).sum()) + 0.25)
    scratch = Flat((B * C,), dev)
    for acc, with_dout in ((0, True), (1, True), (0, False)):
        doc = Canvas(out.shape, F32, dev, pitch=C * Lp + 3, fill=NAN, data=base if acc else None)
        dca, ds = Flat((B, C), dev), Flat((B, 1, H, W), dev)
        dg = Flat((1,), dev, data=torch.tensor([0.25]))
        L.call("cn_sca_apply_bwd_f32", dyc.ptr, dyc.pitch, oc.ptr, oc.pitch, cad.data_ptr(), sd.data_ptr(), gd.data_ptr(),
               doc.ptr if with_dout else None, doc.pitch if with_dout else 0, acc, dca.ptr, ds.ptr, dg.ptr, scratch.ptr, B,
               C, Lp, st)
        torch.cuda.synchronize()
        tag = f"acc={acc} dout={with_dout}"
        if with_dout:
            old = base if acc else torch.zeros_like(base)
            bounded(doc.t, dy * att + old, dy.abs() * e_att + (1 + acc) * U32 * (dy.abs() * (mag + e_att) + old.abs()),
                    "sca apply dout " + tag)
        else:
            assert bool(doc.buf.isnan().all()), "dout is nullable: nothing may be written"
        _canary(doc, "dout")
        bounded(dca.t, ref_dca, b_dca, "sca apply dca " + tag)
        bounded(ds.t, ref_ds, b_ds, "sca apply dsconv " + tag)
        bounded(dg.t, (ref_dg + 0.25).view(1), torch.full((1,), b_dg, dtype=torch.float64), "sca apply dgamma " + tag)
        for f, n in ((dca, "dca"), (ds, "dsconv"), (dg, "dgamma"), (scratch, "scratch")):
            f.assert_slack(n)


@pytest.mark.parametrize("B,C,H,W", [(2, 5, 25, 25), (1, 3, 33, 33)])
def test_sca_apply_bwd_f32_exact_sums_and_reproducible(B, C, H, W):
    """Integer dy and out: the sum behind d ca is exact, and with gamma = 0.5 (g = 1/4) so is d ca. Two identical
    calls give identical bits in every output."""
    dev, L, st = _dev(), lib(), stream()
    Lp = H * W
    out, dy = ints((B, C, H, W), -4, 4, 510), ints((B, C, H, W), -3, 3, 511)
    premise("sca apply dca", term_bound(out, dy, Lp))
    ca, sconv = torch.sigmoid(_randn((B, C), 512)).float(), _randn((B, 1, H, W), 513, 2.0).float()
    oc = Canvas(out.shape, F32, dev, pitch=C * Lp + 7, fill=GARB, data=out)
    dyc = Canvas(dy.shape, F32, dev, pitch=C * Lp + 9, fill=GARB, data=dy)
    cad, sd, gd = ca.to(dev), sconv.to(dev).contiguous(), torch.tensor([0.5], device=dev)
    runs = []
    for _ in range(2):
        doc = Canvas(out.shape, F32, dev, pitch=C * Lp + 3, fill=NAN)
        dca, ds, dg, scratch = Flat((B, C), dev), Flat((B, 1, H, W), dev), Flat((1,), dev, fill=0.0), Flat((B * C,), dev)
        L.call("cn_sca_apply_bwd_f32", dyc.ptr, dyc.pitch, oc.ptr, oc.pitch, cad.data_ptr(), sd.data_ptr(), gd.data_ptr(),
               doc.ptr, doc.pitch, 0, dca.ptr, ds.ptr, dg.ptr, scratch.ptr, B, C, Lp, st)
        torch.cuda.synchronize()
        runs.append((doc.t.clone(), dca.t.clone(), ds.t.clone(), dg.t.clone()))
    assert_exact(runs[0][1], 0.25 * (dy * out).sum((2, 3)), "dca")
    for a, b in zip(*runs):
        assert torch.equal(a, b), "not bit-reproducible"


# ---------------------------------------------------------------------------------------------------------------------
# fp32 spatial-channel attention: the engine
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C,H,W", [(2, 40, 9, 11), (1, 320, 5, 7)])
@pytest.mark.parametrize("few", [False, True])
def test_sca_engine_f32(B, C, H, W, few):
    """engine.spatial_channel_attention on fp32 Vars: y, d skip, d out and every parameter gradient against the
    float64 reference (tests/pointwise_ref.py), tie-free and five-valued (the channel-max gradient split evenly).
    The kernels have their per-element bounds above; this test is about the routing between them, and uses the
    tolerance of its bf16 mirror for fp32 results, 1e-4 of the tensor's max |ref|: the longest chain to any output is
    below C + C/2 + 64 <= 544 roundings, 3.3e-5 relative, while a gradient routed to one of two tied channels is off
    by half of it."""
    from cultionet_amd import engine as E
    from cultionet_amd.convolution import SpatialChannelAttention

    dev = _dev()
    torch.manual_seed(C)
    mod = SpatialChannelAttention(C, "SiLU")
    with torch.no_grad():
        mod.gamma.fill_(0.8)
    skip = _few((B, C, H, W), 520 + C) * 0.5 if few else _randn((B, C, H, W), 520 + C)
    out, dy = _randn((B, C, H, W), 521 + C), _randn((B, C, H, W), 522 + C)
    if few:
        assert bool(((skip == skip.amax(1, keepdim=True)).sum(1) > 1).any())
    s64, o64 = skip.clone().requires_grad_(True), out.clone().requires_grad_(True)
    y64, pw = R.sca_ref64(mod, s64, o64)
    y64.backward(dy)
    mod = mod.to(dev)
    store = E.ParamStore(mod)
    store.zero_grad()
    with E.using_store(store), E.recording(True) as tape:
        sv, ov = E.Var(skip.float().to(dev), True), E.Var(out.float().to(dev), True)
        yv = E.spatial_channel_attention(sv, ov, mod)
        yv.grad = dy.float().to(dev)
        tape.backward()
    torch.cuda.synchronize()

    def close(got, ref, what):
        got, ref = got.detach().double().cpu(), ref.detach()
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print(f"BOUND sca engine {what}: worst err/bound {err / (1e-4 * scale):.3f}")
        assert err <= 1e-4 * scale, f"{what}: max err {err:.3e} > {1e-4 * scale:.3e}"

    close(yv.t, y64, "y")
    close(ov.grad, o64.grad, "dout")
    close(sv.grad, s64.grad, "dskip")
    for n, p in mod.named_parameters():
        close(store.grad_of(p), pw[n].grad, n)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 adaptive max pool
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo", [(2, 3, 28, 28, 14, 14), (2, 3, 25, 25, 12, 12), (3, 2, 7, 7, 3, 3),
                                             (2, 3, 13, 9, 6, 4)])
@pytest.mark.parametrize("kind", ["few", "random", "special"])
def test_adaptive_maxpool_f32_exact(B, C, Hi, Wi, Ho, Wo, kind):
    """y and idx equal F.adaptive_max_pool2d in float64 (first maximum of a window; a NaN wins; an all -inf window
    keeps its first pixel), idx=None gives the same y, and the backward with integer dy equals autograd with
    accumulate 0 and 1, all on padded batch strides."""
    dev, L, st = _dev(), lib(), stream()
    x = _few((B, C, Hi, Wi), 600 + Hi) if kind == "few" else _randn((B, C, Hi, Wi), 600 + Hi)
    if kind == "special":
        x[0, 1, Hi // 2, Wi // 2] = NAN
        x[1, 0, : Hi // 2 + 1, : Wi // 2 + 1] = -math.inf
    xr = x.clone().requires_grad_(True)
    y64, i64 = F.adaptive_max_pool2d(xr, (Ho, Wo), return_indices=True)
    dy = ints((B, C, Ho, Wo), -3, 3, 601, zeros=0.0)
    (dx64,) = torch.autograd.grad(y64, xr, dy)
    if kind == "special":
        assert bool(y64.isnan().any()) and bool((y64 == -math.inf).any())
    xc = Canvas(x.shape, F32, dev, pitch=C * Hi * Wi + 5, fill=GARB, data=x)
    yc = Canvas(y64.shape, F32, dev, pitch=C * Ho * Wo + 3, fill=NAN if kind != "special" else 12345.0)
    idx = Flat((B, C, Ho, Wo), dev, fill=-7, dtype=torch.int32)
    L.call("cn_adaptive_maxpool_fwd_f32", xc.ptr, xc.pitch, yc.ptr, yc.pitch, idx.ptr, B, C, Hi, Wi, Ho, Wo, st)
    y2 = Canvas(y64.shape, F32, dev, pitch=C * Ho * Wo + 3, fill=12345.0)
    L.call("cn_adaptive_maxpool_fwd_f32", xc.ptr, xc.pitch, y2.ptr, y2.pitch, None, B, C, Hi, Wi, Ho, Wo, st)
    torch.cuda.synchronize()
    _same(yc.t, y64.detach(), "y")
    _same(y2.t, y64.detach(), "y (no idx)")
    assert torch.equal(idx.t.cpu().long(), i64), "idx (first maximum of the window)"
    _canary(yc, "y")
    _canary(y2, "y (no idx)")
    idx.assert_slack("idx")
    if kind == "few":
        first = F.adaptive_max_pool2d(-torch.arange(Hi * Wi, dtype=torch.float64).view(1, 1, Hi, Wi), (Ho, Wo))
        assert bool((i64 != (-first).long()).any())  # a maximum that is not the window's first pixel ...
        assert bool(((x.flatten(2).gather(2, i64.flatten(2)) == y64.detach().flatten(2)).all()))
    dyc = Canvas(dy.shape, F32, dev, pitch=C * Ho * Wo + 7, fill=GARB, data=dy)
    base = ints((B, C, Hi, Wi), -8, 8, 602)
    for acc in (0, 1):
        dxc = Canvas(x.shape, F32, dev, pitch=C * Hi * Wi + 9, fill=NAN, data=base if acc else None)
        L.call("cn_adaptive_maxpool_bwd_f32", dyc.ptr, dyc.pitch, idx.ptr, dxc.ptr, dxc.pitch, B, C, Hi, Wi, Ho, Wo, acc,
               st)
        torch.cuda.synchronize()
        assert_exact(dxc.t, dx64 + (base if acc else 0), f"dx acc={acc}")
        _canary(dxc, "dx")


def test_adaptive_maxpool_engine_f32_exact():
    """engine.adaptive_max_pool2d on an fp32 Var under the tape (25 -> 12, overlapping windows, five-valued data) and
    with the tape off."""
    from cultionet_amd import engine as E

    B, C, Hi, Ho = 2, 5, 25, 12
    x, dy = _few((B, C, Hi, Hi), 610), ints((B, C, Ho, Ho), -3, 3, 611, zeros=0.0)
    xr = x.clone().requires_grad_(True)
    y64 = F.adaptive_max_pool2d(xr, (Ho, Ho))
    (dx64,) = torch.autograd.grad(y64, xr, dy)
    y, dx = _engine_tape(lambda v: E.adaptive_max_pool2d(v, (Ho, Ho)), x, dy, False)
    with E.recording(False):
        ye = E.adaptive_max_pool2d(E.Var(x.float().to(_dev())), (Ho, Ho))
    torch.cuda.synchronize()
    assert_exact(y, y64.detach(), "y")
    assert_exact(ye.t, y64.detach(), "y (tape off)")
    assert_exact(dx, dx64, "dx")


# ---------------------------------------------------------------------------------------------------------------------
# TowerUNetFinalCombine + SigmoidCrisp
# ---------------------------------------------------------------------------------------------------------------------
SMOOTH = float(np.float32(1e-2))  # the kernel receives the fp32 value


def _ptr16(t):
    return (ctypes.c_void_p * 16)(*[t.data_ptr() + 4 * k for k in range(16)])


def _fc_params(seed, crisp, negative):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(16, generator=g, dtype=torch.float64) * 0.5 + 0.75  # tower gammas, weights, biases in [0.75, 1.25]
    p[12:15] -= 1.0
    if negative:
        p[4] = -p[4]
    p[15] = crisp
    return p.float().double()


def _fc_forward_bounds(h, p):
    """Per task k: s, e_s, z (the sigmoid's argument), e_z, and for the edge task the linear part, with
    s = sum_t (1/gamma_t) h_t: a reciprocal, a product and two adds: 4 u on sum |h_t / gamma_t|;
    z = w s + b: 2 u (|w s| + |b|); edge: z *= crisp, crisp = 1 / (smooth + sigmoid(gamma_c)) within (|gamma_c| + 10) u
    relative (the sigmoid's (|gamma_c| + 8) u, the add, the reciprocal), and the product."""
    sg = torch.sigmoid(p[15])
    crisp = 1.0 / (SMOOTH + sg)
    r_crisp = (p[15].abs() + 10) * U32
    res = []
    for k in range(3):
        terms = [h[t][:, k:k + 1] / p[3 * k + t] for t in range(3)]
        s, sabs = sum(terms), sum(t.abs() for t in terms)
        e_s = 4 * U32 * sabs
        zlin = p[9 + k] * s + p[12 + k]
        e_zlin = p[9 + k].abs() * e_s + 2 * U32 * ((p[9 + k] * s).abs() + p[12 + k].abs())
        z, e_z = zlin, e_zlin
        if k == 1:
            z = zlin * crisp
            e_z = crisp * e_zlin + (r_crisp + U32) * (zlin.abs() + e_zlin) * crisp
        res.append(dict(s=s, e_s=e_s, zlin=zlin, e_zlin=e_zlin, z=z, e_z=e_z))
    return res, sg, crisp, r_crisp


@pytest.mark.parametrize("B,H,W", [(2, 20, 20), (3, 149, 149)])
@pytest.mark.parametrize("crisp,negative", [(1.0, False), (-3.0, True), (0.0, False), (3.0, True)])
def test_final_combine_f32_random_bound(B, H, W, crisp, negative):
    """Forward and backward against float64 autograd. B*HW = 66603 > 256*256 makes the backward's grid-stride loop
    iterate (twice for some threads, ragged).

    Forward: out = sigmoid(z): 0.25 e_z + (|z| + 8) u out.
    Backward (out given as the float64 value rounded to fp32, which moves o (1 - o) by at most u o):
      dz = d out * o * (1 - o): 3 u |dz| + u |d out| o; edge: dz *= crisp (crisp's error + 1);
      dh_t = dz w / gamma_t: three more roundings (the product with w, the reciprocal, the product).
    Parameter gradients: sums over the n = B*HW pixels into prefilled values: a thread adds ceil(n / (256 nb)) terms
    (nb = min(256, ceil(n / 256)) blocks), cn_block_sum 9, then nb atomic adds: R = ceil(n / (256 nb)) + 9 + nb + 1
    roundings (272 at n = 66603) on sum |terms| + |prefill|, plus per term:
      d bias = sum dz; d w = sum dz s (1 + the error of s); d gamma_t = -sum dz w h_t / gamma_t^2 (6: four products,
      two reciprocals); d crisp = F sum dz_edge zlin with F = -sg (1 - sg) crisp^2, whose error carries the sigmoid's
      through |1 - 2 sg| and crisp's twice, plus 4 products."""
    dev, L, st = _dev(), lib(), stream()
    n, HW = B * H * W, H * W
    p = _fc_params(700, crisp, negative)
    h = [_randn((B, 3, H, W), 701 + t, 0.25) for t in range(3)]
    dout = [_randn((B, 1, H, W), 711 + k) for k in range(3)]
    pre = _randn((16,), 720)
    hr = [t.clone().requires_grad_(True) for t in h]
    pr = [p[k].clone().requires_grad_(True) for k in range(16)]
    o64 = R.final_combine_ref(hr[0], hr[1], hr[2], pr, SMOOTH)
    grads = torch.autograd.grad(sum((o * d).sum() for o, d in zip(o64, dout)), hr + pr)
    dh64, dp64 = grads[:3], torch.stack(grads[3:])
    fb, sg, cr, r_crisp = _fc_forward_bounds(h, p)
    # the relative-error model needs every intermediate to be a normal fp32 number: sigmoid(-60) = 9e-27 leaves room
    # for the products with d out (crisp gamma = -3 multiplies the edge logits by 17.4, hence the 0.25 on h)
    assert max(float(f["z"].abs().max()) for f in fb) < 60.0

    pd = p.float().to(dev)
    hd = [t.float().to(dev).contiguous() for t in h]
    outs = [Flat((B, 1, H, W), dev) for _ in range(3)]
    L.call("cn_final_combine_fwd_f32", hd[0].data_ptr(), hd[1].data_ptr(), hd[2].data_ptr(), _ptr16(pd), outs[0].ptr,
           outs[1].ptr, outs[2].ptr, B, HW, SMOOTH, st)
    torch.cuda.synchronize()
    for k, name in enumerate(("dist", "edge", "crop")):
        o = o64[k].detach()
        e = 0.25 * fb[k]["e_z"] + (fb[k]["z"].abs() + fb[k]["e_z"] + 8) * U32 * o
        bounded(outs[k].t, o, e, f"final combine {name} n={n} crisp={crisp}")
        outs[k].assert_slack(name)

    # backward on the rounded float64 outputs
    o32 = [o.detach().float().double() for o in o64]
    od = [o.float().to(dev).contiguous() for o in o32]
    dd = [d.float().to(dev).contiguous() for d in dout]
    dh = [Flat((B, 3, H, W), dev) for _ in range(3)]
    dpar = Flat((16,), dev, data=pre)
    L.call("cn_final_combine_bwd_f32", hd[0].data_ptr(), hd[1].data_ptr(), hd[2].data_ptr(), _ptr16(pd),
           od[0].data_ptr(), od[1].data_ptr(), od[2].data_ptr(), dd[0].data_ptr(), dd[1].data_ptr(), dd[2].data_ptr(),
           dh[0].ptr, dh[1].ptr, dh[2].ptr, _ptr16(dpar.buf), B, HW, SMOOTH, st)
    torch.cuda.synchronize()
    nb = min(256, math.ceil(n / 256))
    red = math.ceil(n / (256 * nb)) + RED + nb + 1
    if n > 65536:
        assert nb == 256 and math.ceil(n / (256 * nb)) == 2 and n % 256 != 0
    b_dh = [torch.zeros(B, 3, H, W, dtype=torch.float64) for _ in range(3)]
    b_dp = torch.zeros(16, dtype=torch.float64)
    tsum = torch.zeros(16, dtype=torch.float64)  # sum |terms| of every parameter gradient
    for k in range(3):
        o, d, f = o32[k], dout[k], fb[k]
        w = p[9 + k]
        dz = d * o * (1 - o)
        e_dz = 3 * U32 * dz.abs() + U32 * d.abs() * o
        if k == 1:
            # d crisp: T = sum dz zlin (dz before the crisp factor), times F
            t15 = dz * f["zlin"]
            e_t15 = f["zlin"].abs() * e_dz + dz.abs() * f["e_zlin"] + U32 * t15.abs()
            F_ = -sg * (1 - sg) * cr * cr
            e_sg = (p[15].abs() + 8) * U32 * sg
            e_F = (1 - 2 * sg).abs() * cr * cr * e_sg + 2 * r_crisp * F_.abs() + 5 * U32 * F_.abs()
            T_abs = t15.abs().sum()
            b_dp[15] = F_.abs() * (e_t15.sum() + red * U32 * T_abs) + e_F * T_abs + U32 * F_.abs() * T_abs
            tsum[15] = 0.0
            dz = dz * cr
            e_dz = cr * e_dz + (r_crisp + U32) * dz.abs()
        # d bias, d w
        b_dp[12 + k], tsum[12 + k] = e_dz.sum(), dz.abs().sum()
        tw = dz * f["s"]
        b_dp[9 + k] = (f["s"].abs() * e_dz + dz.abs() * f["e_s"] + U32 * tw.abs()).sum()
        tsum[9 + k] = tw.abs().sum()
        for t in range(3):
            gm = p[3 * k + t]
            v = h[t][:, k:k + 1]
            dht = dz * w / gm
            b_dh[t][:, k:k + 1] = (w / gm).abs() * e_dz + 3 * U32 * dht.abs()
            tg = dht * v / gm
            b_dp[3 * k + t] = ((w * v / (gm * gm)).abs() * e_dz + 6 * U32 * tg.abs()).sum()
            tsum[3 * k + t] = tg.abs().sum()
    b_dp = b_dp + red * U32 * (tsum + pre.abs())
    b_dp[15] = b_dp[15] + 2 * U32 * (pre[15].abs() + dp64[15].abs())
    for t in range(3):
        bounded(dh[t].t, dh64[t], b_dh[t], f"final combine dh{t} n={n} crisp={crisp}")
        dh[t].assert_slack("dh")
    got = dpar.t.cpu().double()
    ratio = (got - (dp64 + pre)).abs() / b_dp
    print(f"BOUND final combine dparams n={n} crisp={crisp}: worst err/bound {float(ratio.max()):.3f} "
          f"(reduction {red} roundings)")
    assert bool((ratio <= 1).all()), f"dparams err/bound {ratio.tolist()}"
    dpar.assert_slack("dparams")


def test_final_combine_f32_empty_batch_is_a_noop():
    dev, L, st = _dev(), lib(), stream()
    pd = torch.ones(16, device=dev)
    bufs = [Flat((64,), dev) for _ in range(13)]
    dpar = Flat((16,), dev, fill=3.0)
    a = [b.ptr for b in bufs]
    L.call("cn_final_combine_fwd_f32", a[0], a[1], a[2], _ptr16(pd), a[3], a[4], a[5], 0, 400, SMOOTH, st)
    L.call("cn_final_combine_bwd_f32", a[0], a[1], a[2], _ptr16(pd), a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11],
           _ptr16(dpar.buf), 0, 400, SMOOTH, st)
    torch.cuda.synchronize()
    assert all(bool(b.buf.isnan().all()) for b in bufs) and bool((dpar.buf == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# predict tiling: cn_window_chips_f32, cn_stitch_predictions_u16
# ---------------------------------------------------------------------------------------------------------------------
NP_DTYPES = {0: np.float32, 1: np.int32, 2: np.int16, 3: np.uint16}


def _scene(code, P, H, W, seed):
    rng = np.random.default_rng(seed)
    if code == 0:
        return rng.normal(3000, 4000, (P, H, W)).astype(np.float32)
    if code == 1:
        return rng.integers(-40000, 70000, (P, H, W)).astype(np.int32)
    if code == 2:
        s = rng.integers(-32768, 32768, (P, H, W)).astype(np.int16)
        assert (s < 0).any()
        return s
    s = rng.integers(0, 65536, (P, H, W)).astype(np.uint16)
    assert (s > 32767).any()
    return s


@pytest.mark.parametrize("code", [0, 1, 2, 3])
@pytest.mark.parametrize("H,W,ws,pad", [(70, 90, 32, 8), (50, 41, 64, 4)])
@pytest.mark.parametrize("zscore", [True, False])
def test_window_chips_f32_bit_exact(code, H, W, ws, pad, zscore):
    """Bit-equal to the numpy restatement for all four scene dtypes (int16 with negative values, uint16 above 32767):
    windows at every corner, so the padding reaches outside the scene on every side; a scene smaller than one window
    (50 x 41 under a 64 window); S*S > 1024, so the per-window loop strides; mean / std present and absent."""
    dev, L, st = _dev(), lib(), stream()
    C, T = 2, 3
    S = ws + 2 * pad
    assert S * S > 1024
    scene = _scene(code, C * T, H, W, 800 + code)
    wins = [(r, c) for r in range(0, H, ws) for c in range(0, W, ws)]
    mean = np.array([0.21, 0.35], dtype=np.float32) if zscore else None
    std = np.array([0.11, 0.07], dtype=np.float32) if zscore else None
    want = R.window_chips_ref(scene, wins, T, S, pad, mean, std, 1e-4, 0.0, 1.0)
    assert (want[0, :, :pad] == want[0, :, :1, :1]).all()  # window (0, 0): its top padding lies outside the scene
    sd = torch.from_numpy(scene.view(np.int16) if code == 3 else scene).to(dev)
    wd = torch.tensor(wins, dtype=torch.int32, device=dev)
    out = Flat(want.shape, dev)
    md = None if mean is None else torch.from_numpy(mean).to(dev)
    vd = None if std is None else torch.from_numpy(std).to(dev)
    L.call("cn_window_chips_f32", sd.data_ptr(), code, out.ptr, wd.data_ptr(), len(wins), C, T, H, W, S, pad,
           None if md is None else md.data_ptr(), None if vd is None else vd.data_ptr(), 1e-4, 0.0, 1.0, st)
    torch.cuda.synchronize()
    got = out.t.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {want.size} values differ"
    out.assert_slack("chips")


def test_window_chips_f32_padding_as_wide_as_the_window_is_an_error():
    L, st = lib(), stream()
    t = torch.zeros(4096, device=_dev())
    w = torch.zeros(2, dtype=torch.int32, device=_dev())
    for S, pad in ((16, 8), (16, 9)):
        with pytest.raises(L.HipKernelError):
            L.call("cn_window_chips_f32", t.data_ptr(), 0, t.data_ptr(), w.data_ptr(), 1, 1, 1, 8, 8, S, pad, None, None,
                   1e-4, 0.0, 1.0, st)
    torch.cuda.synchronize()


def test_stitch_predictions_u16_bit_exact():
    """Probabilities on and next to integer counts (k / 10000 and its fp32 neighbours), outside [0, 1], and NaN;
    windows clipped at the bottom and right edge; one window left out: its part of the mosaic stays zero."""
    dev, L, st = _dev(), lib(), stream()
    S, pad, ws, H, W, scale = 40, 4, 32, 70, 50, 10000.0
    wins = [(r, c) for r in range(0, H, ws) for c in range(0, W, ws)]
    left_out = wins.pop(1)
    rng = np.random.default_rng(9)
    maps = []
    for k in range(3):
        ks = rng.integers(0, 10001, (len(wins), S, S))
        v = (ks / 10000.0).astype(np.float32)
        step = rng.integers(-1, 2, v.shape)
        v = np.where(step < 0, np.nextafter(v, np.float32(-1)), np.where(step > 0, np.nextafter(v, np.float32(2)), v))
        v = v.astype(np.float32)
        v[k, 5, 5:9] = [np.nan, -0.25, 1.5, 7.0]
        v[0, 6 + k, 6] = np.nan
        maps.append(v)
    want = R.stitch_ref(maps[0], maps[1], maps[2], wins, S, pad, ws, H, W, scale)
    assert (want[:, left_out[0]:left_out[0] + ws, left_out[1]:] == 0).all() and (want == 10000).any()
    md = [torch.from_numpy(m).to(dev) for m in maps]
    wd = torch.tensor(wins, dtype=torch.int32, device=dev)
    out = Flat((3, H, W), dev, fill=0, dtype=torch.int16)
    L.call("cn_stitch_predictions_u16", md[0].data_ptr(), md[1].data_ptr(), md[2].data_ptr(), out.ptr, wd.data_ptr(),
           len(wins), S, pad, ws, H, W, scale, st)
    torch.cuda.synchronize()
    got = out.t.cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} counts differ"
    out.assert_slack("mosaic")
