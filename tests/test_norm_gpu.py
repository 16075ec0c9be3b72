"""The normalisation kernels (cn_norm.hip, cn_bnorm.hip, the statistics epilogue of cn_bconv.hip) against the float64
restatement of tests/test_norm_ref.py, at training shapes and at the edges of the kernels' launch paths.

Every comparison is per element, with a bound built from the magnitudes that feed that element (no floor, no max|ref|).
u = 2^-24 (fp32 unit roundoff), c = 16 for every rounding of an element's own chain (subtract, two multiplies, add,
exp + divide in SiLU, residual add: <= 8 roundings, doubled for the fp32 mean and rstd every element shares). For fp32:
  y      c*u*(|g|*rstd*(|x| + |m| + s) + |b| + |r|) + |g|*(rstd*dm + |xh|*dv*rstd^2/2)     s = sqrt(var)
  mean   c*u*(|m| + s) + dm;   rstd: relative c*u + dv*rstd^2/2 (a variance error reaches rstd through var + eps)
  dx     c*u*|g|*rstd*(|dy| + |dz| + |mean dz| + |xh|*|mean(dz*xh)|) + D*u*|g|*rstd*(mean|dz| + |xh|*mean|dz*xh|) + P
  dgamma (c + D)*u*sum|dz*xh| + P;   dbeta (c + D)*u*sum(|dz| + |dy|) + P
  running statistics c*u*(|old| + momentum*|batch value|) + momentum*(dm or dv)
|dy| sits beside |dz| because SiLU' is evaluated in fp32 (its rounding is absolute, ~u).
D is the serial length of the fp32 chains a kernel's sums go through: a chain of D fp32 additions is off by at most
D*u*sum|terms|. The fp32 BatchNorm kernels sum in fp64 (D = 0); the bf16 ones sum rows/R pixels per thread, then R
thread rows (bbn_depth, 56-74 at batch 32); the conv epilogue's rows are tile sums of <= 128 pixels (D = 128).
Statistics from such sums get dm = D*u*(|m| + s) and dv = 3*D*u*(m^2 + var) (sum x^2 - n m^2 cancels that much), except
for a constant channel: the tests' constant 0.75 has exact fp32 partial sums (k*0.75, k*0.5625 for k < 2^20), so it is
held to D = 0 -- a wrong rstd there shows in dx.
P is the first-order effect of the error of xh, e = c*u*rstd*(|x| + |m| + s) + rstd*dm + |xh|*dv*rstd^2/2 per element,
carried through dz = dy*SiLU'(g*xh + b) (|SiLU''| <= 1/2) and the two channel means.

bf16 outputs: the reference runs on the bf16-rounded inputs and the bound adds half a bf16 ulp of y64. LayerNorm uses
the same forms per pixel row, with D the depth of its sums over C (ln_depth: 12-36 for C <= 128, C above, 8 + log2(C/8)
in bf16) and, for dw / db, of the reduction over pixels (ln_param_depth). Each check prints its worst ratio of error to
bound; run with -s to read the margins.
"""
import ctypes
import math
import zlib

import pytest
import torch
import torch.nn as nn

from test_norm_ref import bn_bwd64, bn_fwd64, ln_bwd64, ln_fwd64

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_F32 = 16.0
BF = torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _tab(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _within(got, ref, bound, what):
    got = got.detach().double().to(ref.device)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs()
    ratio = err / bound
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst err/bound {worst:.3f}")
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: err {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e} at flat "
                             f"index {i} (got {float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r})")


def _ch(v):
    return v[None, :, None]


def _half_ulp16(y, slack):
    """Half a bf16 ulp (8 significant bits) of the rounded value: it lies within |y| + slack (slack: the bound of the
    fp32 result before rounding), so the ulp is taken there -- a result just across a power of two from y64 is rounded
    in its own binade."""
    _, e = torch.frexp(y.abs() + slack)
    return torch.ldexp(torch.ones_like(y), e - 9)


# ---------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------

def bbn_depth(P, C):
    """Serial length of the fp32 chains of the bf16 BatchNorm statistics / parameter-gradient passes (bbn_grid of
    cn_bnorm.hip): every thread sums rows/R pixels, then one thread per column sums the R thread rows of its block;
    the block rows are combined in fp64."""
    R = 256 // (C // 8)
    want = min(max(-(-P // (R * 8)), 1), 512)
    rows = -(-P // want)
    rows = -(-rows // R) * R
    return rows // R + R


def ln_depth(C, bf16):
    """Serial length of the fp32 sums over the C values of one LayerNorm row: the C <= 128 kernels sum CPW channels per
    wave and then the 4 waves, the wide kernel sums all C in turn; bf16: 8 channels per lane, then a shuffle tree."""
    if bf16:
        return 8 + int(math.log2(C // 8))
    if C <= 128:
        return (8 if C <= 32 else 16 if C <= 64 else 32) + 4
    return C


def ln_param_depth(B, C, L, bf16):
    """Serial length of the fp32 chains behind LayerNorm dw / db. C <= 128: a lane's tiles, the wave tree, the block
    partials summed by cn_ln_param_finalize_kernel (nblk / 128 each, then 8 in LDS, then 16 atomics); wider: the wave
    tree, 4 waves, one atomic per block. bf16: a thread's pixels, R thread rows, one atomic per block."""
    P = B * L
    if bf16:
        R = 256 // (C // 8)
        nb = min(max(-(-P // (R * 8)), 1), 1024)
        return -(-P // (nb * R)) + R + nb
    if C <= 128:
        ntiles = -(-P // 64)
        nblk = min(ntiles, 2048)
        return -(-ntiles // nblk) + 6 + -(-nblk // 128) + 8 + 16
    return 10 + -(-P // 256)


def _bn_stat_allowance(fwd, training, depth, stat_err=None):
    """(mean, variance, relative rstd) allowances per channel of batch statistics summed in fp32 chains of `depth`."""
    m, s, var = fwd["mean"].abs(), fwd["var"].sqrt(), fwd["var"]
    if not training:
        z = torch.zeros_like(var)
        return z, z, z
    D = torch.where(var == 0, torch.zeros_like(var), torch.full_like(var, float(depth)))  # exact: see the docstring
    dm = D * U * (m + s)
    dv = 3 * D * U * (m * m + var)
    if stat_err is not None:
        dm, dv = dm + stat_err[0], dv + stat_err[1]
    return dm, dv, 0.5 * dv * fwd["rstd"] ** 2  # a variance error reaches rstd = (var + eps)^-1/2 through var + eps


def _bn_y_bound(fwd, x, gamma, beta, res, dm, rrel, c=C_F32):
    g, rs = _ch(gamma.double().abs()), _ch(fwd["rstd"])
    ms = _ch(fwd["mean"].abs() + fwd["var"].sqrt())
    return c * U * (g * rs * (x.abs() + ms) + _ch(beta.double().abs()) + (res.double().abs() if res is not None else 0.0)) \
        + g * (rs * _ch(dm) + fwd["xhat"].abs() * _ch(rrel))


def _bn_check(tag, fwd, bwd, x, gamma, beta, res, dy, *, act, training, momentum, got, old=None, c=C_F32, bf16=False,
              depth=0, stat_err=None, dx_prior=None):
    """got: dict of kernel results on [B, C, L] views (y, dx, dgamma, dbeta, mean, rstd, running_mean, running_var;
    any may be missing). old: running statistics before the call. depth: D of the module docstring (0: fp64 sums).
    stat_err: per-channel (mean, variance) allowances of statistics taken from elsewhere (the conv epilogue's rows)."""
    x, dy = x.double(), dy.double()
    g, rs = _ch(gamma.double().abs()), _ch(fwd["rstd"])
    m, s, var = fwd["mean"].abs(), fwd["var"].sqrt(), fwd["var"]
    n = x.shape[0] * x.shape[2]
    dm, dv, rrel = _bn_stat_allowance(fwd, training, depth, stat_err)
    ey = _bn_y_bound(fwd, x, gamma, beta, res, dm, rrel, c)
    if "y" in got:
        _within(got["y"], fwd["y"], ey + (_half_ulp16(fwd["y"], ey) if bf16 else 0.0), f"{tag} y")
    if training and "mean" in got:
        _within(got["mean"], fwd["mean"], c * U * (m + s) + dm, f"{tag} mean")
    if "rstd" in got:
        _within(got["rstd"], fwd["rstd"], (c * U + rrel) * fwd["rstd"], f"{tag} rstd")
    if "running_mean" in got and "running_mean" in fwd:
        unb = var * n / (n - 1) if n > 1 else var
        _within(got["running_mean"], fwd["running_mean"],
                c * U * (old[0].double().abs() + momentum * (m + s)) + momentum * dm + 1e-45, f"{tag} running_mean")
        _within(got["running_var"], fwd["running_var"],
                c * U * (old[1].double().abs() + momentum * unb) + momentum * dv * max(n, 2) / max(n - 1, 1) + 1e-45,
                f"{tag} running_var")
    if bwd is None:
        return
    dz, xh = bwd["dz"], fwd["xhat"]
    # the error of xh: its own roundings plus those of the statistics (see the module docstring)
    ex = c * U * rs * (x.abs() + _ch(m + s)) + rs * _ch(dm) + xh.abs() * _ch(rrel)
    ddz = 0.5 * dy.abs() * g * ex if act else torch.zeros_like(ex)
    md, mdx = _ch(bwd["dbeta"].abs() / n), _ch(bwd["dgamma"].abs() / n)
    # the channel means of dz and dz*xh come from sums of depth D
    m1, m2 = _ch((dz.abs() + dy.abs()).sum(dim=(0, 2)) / n), _ch((dz * xh).abs().sum(dim=(0, 2)) / n)
    base = c * U * g * rs * (dy.abs() + dz.abs() + md + xh.abs() * mdx) + depth * U * g * rs * (m1 + xh.abs() * m2)
    if training:
        prop = g * rs * (ddz + _ch(ddz.sum(dim=(0, 2)) / n) + ex * mdx
                         + xh.abs() * _ch((ddz * xh.abs() + dz.abs() * ex).sum(dim=(0, 2)) / n))
    else:
        prop = g * rs * ddz + g * dz.abs() * c * U * rs
    if dx_prior is not None:  # accumulated into a prior gradient: one more rounding of that magnitude
        base = base + c * U * dx_prior.double().abs()
    if "dx" in got:
        _within(got["dx"], bwd["dx"], base + prop + (_half_ulp16(bwd["dx"], base + prop) if bf16 else 0.0),
                f"{tag} dx")
    pg = (ddz * xh.abs() + dz.abs() * ex).sum(dim=(0, 2))
    if "dgamma" in got:
        _within(got["dgamma"], bwd["dgamma"], (c + depth) * U * (dz * xh).abs().sum(dim=(0, 2)) + pg + 1e-45,
                f"{tag} dgamma")
    if "dbeta" in got:
        _within(got["dbeta"], bwd["dbeta"], (c + depth) * U * (dz.abs() + dy.abs()).sum(dim=(0, 2))
                + ddz.sum(dim=(0, 2)) + 1e-45, f"{tag} dbeta")


def _ln_check(tag, fwd, bwd, x, w, b, res, dy, got, c=C_F32, bf16=False, dx_prior=None):
    x = x.double()
    B, C, L = x.shape
    wa, rs = _ch(w.double().abs()), fwd["rstd"]
    m, s, var = fwd["mean"].abs(), fwd["var"].sqrt(), fwd["var"]
    Dl = ln_depth(C, bf16)
    exact = var == 0  # the tests' constant rows (0.5 in every channel): every fp32 partial sum is exact
    dm = torch.where(exact, torch.zeros_like(var), Dl * U * (m + s))
    dv = torch.where(exact, torch.zeros_like(var), Dl * U * var + dm * dm)  # centred sum of squares: depth Dl
    rrel = 0.5 * dv * rs ** 2
    ey = c * U * (wa * rs * (x.abs() + m + s) + _ch(b.double().abs())
                  + (res.double().abs() if res is not None else 0.0)) + wa * (rs * dm + fwd["xhat"].abs() * rrel)
    _within(got["y"], fwd["y"], ey + (_half_ulp16(fwd["y"], ey) if bf16 else 0.0), f"{tag} y")
    if bwd is None:
        return
    dy = dy.double()
    xh = fwd["xhat"]
    gg = dy * _ch(w.double())
    ga = gg.abs()
    a1, a2 = (gg.sum(dim=1, keepdim=True) / C).abs(), ((gg * xh).sum(dim=1, keepdim=True) / C).abs()
    ex = c * U * rs * (x.abs() + m + s) + rs * dm + xh.abs() * rrel
    bound = c * U * rs * (ga + a1 + xh.abs() * a2) \
        + Dl * U * rs * (ga.sum(dim=1, keepdim=True) + xh.abs() * (ga * xh.abs()).sum(dim=1, keepdim=True)) / C \
        + rs * (ex * a2 + xh.abs() * (ga * ex).sum(dim=1, keepdim=True) / C)
    if dx_prior is not None:  # accumulated into a prior gradient: one more rounding of that magnitude
        bound = bound + c * U * dx_prior.abs()
    _within(got["dx"], bwd["dx"], bound + (_half_ulp16(bwd["dx"], bound) if bf16 else 0.0), f"{tag} dx")
    Dp = ln_param_depth(B, C, L, bf16)
    _within(got["dw"], bwd["dw"], (c + Dp) * U * (dy * xh).abs().sum(dim=(0, 2)) + (dy.abs() * ex).sum(dim=(0, 2))
            + 1e-45, f"{tag} dw")
    _within(got["db"], bwd["db"], (c + Dp) * U * dy.abs().sum(dim=(0, 2)) + 1e-45, f"{tag} db")


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _randn(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=_gen(seed), device=_dev()) * scale + shift


def _bn_module(C, seed, eps=1e-5, momentum=0.1, track=True, kind=nn.BatchNorm2d):
    bn = kind(C, eps=eps, momentum=momentum, track_running_stats=track)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
        bn.bias.copy_(0.2 * torch.randn(C, generator=g))
        if track:
            bn.running_mean.copy_(0.2 * torch.randn(C, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    return bn.to(_dev())


def _x(shape, seed, edges=False):
    """Activations with a per-channel offset. edges: channel 0 constant 0.75 (var 0); channel 1 at mean/std ~ 1e3
    ("f32", or True) or ~ 4 ("bf16": the bf16 statistics are fp32 sums, see the module docstring)."""
    C = shape[1]
    x = _randn(shape, seed, 1.5) + _randn((1, C) + (1,) * (len(shape) - 2), seed + 1, 0.5)
    if edges and C >= 2:
        x[:, 0] = 0.75
        if edges == "bf16":
            x[:, 1] = x[:, 1] * 0.25 + 1.5
        else:
            x[:, 1] = x[:, 1] * 0.01 + 15.0  # std ~0.015
    return x


def _slice_of(shape, lead=1, extra=3, odd=False):
    """A [B, C, ...] channel slice of a wider buffer (batch stride (C + extra) * L, channel offset `lead`); odd: the
    base pointer sits one float past a 16-byte boundary (the float4 staging gate is off)."""
    B, C = shape[0], shape[1]
    inner = shape[2:]
    n = B * (C + extra) * math.prod(inner)
    flat = torch.full((n + 1,), float("nan"), device=_dev())
    buf = flat[1:] if odd else flat[:n]
    return buf.view(B, C + extra, *inner)[:, lead:lead + C]


def _run(params_mod, fn, xs, dys):
    """fn(*Vars) under a recording tape with the parameters of `params_mod` in a ParamStore; dys: one gradient per
    output (or None for an output left without one). Returns (outputs, input grads, store)."""
    from cultionet_amd import engine as E

    store = E.ParamStore(params_mod)
    store.zero_grad()
    with E.using_store(store), E.recording(True) as tape:
        vs = [E.Var(t, True) for t in xs]
        outs = fn(*vs)
        outs = outs if isinstance(outs, list) else [outs]
        for o, d in zip(outs, dys):
            o.grad = d
        tape.backward()
    torch.cuda.synchronize()
    return [o.t for o in outs], [v.grad for v in vs], store


def _flat3(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 bn_act
# ---------------------------------------------------------------------------------------------------------------------
# id: (shape, act, residual, training, edges, layout) -- layout: dense | slices (x, residual and y as channel slices of
# wider buffers) | odd (x at an odd float offset: scalar staging)
BN_CASES = {
    "l100_c32_b8": ((8, 32, 100, 100), 1, True, True, True, "dense"),
    "l50_c64_b8": ((8, 64, 50, 50), 1, False, True, False, "dense"),
    "l25_c128_b8": ((8, 128, 25, 25), 1, True, True, True, "dense"),
    "l13_c256_b8_fused": ((8, 256, 13, 13), 1, True, True, True, "dense"),
    "l13_c128_b8_fused_eval": ((8, 128, 13, 13), 1, True, False, True, "dense"),
    "l100_c128_b8": ((8, 128, 100, 100), 1, True, True, False, "dense"),
    "l100_c128_b8_eval": ((8, 128, 100, 100), 1, False, False, False, "dense"),
    "l50_c128_b8_eval": ((8, 128, 50, 50), 0, True, False, True, "dense"),
    "gate_2048_c32_fused": ((8, 32, 16, 16), 1, True, True, True, "dense"),
    "gate_2048_c31": ((8, 31, 16, 16), 1, True, True, True, "dense"),
    "gate_2049_c32": ((1, 32, 2049, 1), 1, True, True, True, "dense"),
    "gate_2049_c31": ((1, 31, 2049, 1), 0, False, True, True, "dense"),
    "gate_2048_c32_eval": ((8, 32, 16, 16), 1, False, False, False, "dense"),
    "plane_625_scalar": ((4, 32, 25, 25), 1, True, True, True, "dense"),
    "odd_offset_scalar": ((4, 48, 20, 20), 1, True, True, True, "odd"),
    "slices": ((2, 64, 100, 100), 1, True, True, True, "slices"),
    "slices_fused": ((4, 64, 13, 13), 1, True, True, False, "slices"),
    "count_one": ((1, 32, 1, 1), 1, False, True, False, "dense"),
    "count_one_wide": ((1, 8, 1, 1), 0, False, True, False, "dense"),
}


def _bn_case(shape, act, res, training, edges, layout, *, eps=1e-5, momentum=0.1, channels=None, seed=0, tag=""):
    from cultionet_amd import engine as E

    C = channels or shape[1]
    kind = nn.BatchNorm3d if channels else nn.BatchNorm2d
    bn = _bn_module(C, 100 + seed, eps=eps, momentum=momentum, kind=kind)
    bn.train(training)
    xv = _x(shape if not channels else (shape[0], C, shape[1] // C) + tuple(shape[2:]), seed, edges).reshape(shape)
    rv = _randn(shape, seed + 2) if res else None
    dy = _randn(shape, seed + 3)
    x_in, r_in, out = xv, rv, None
    if layout in ("slices", "odd"):
        x_in = _slice_of(shape, odd=(layout == "odd"))
        x_in.copy_(xv)
    if layout == "slices":
        if res:
            r_in = _slice_of(shape, lead=2, extra=5)
            r_in.copy_(rv)
        out = _slice_of(shape, lead=0, extra=2)
    old = (bn.running_mean.clone(), bn.running_var.clone())
    gamma, beta = bn.weight.detach().clone(), bn.bias.detach().clone()
    B = shape[0]
    v3 = lambda t: t.reshape(B, C, -1)
    fwd = bn_fwd64(v3(xv), gamma, beta, old[0], old[1], training=training, momentum=momentum, eps=eps, act=act,
                   res=v3(rv) if res else None)
    bwd = bn_bwd64(fwd, gamma, v3(dy), training=training, act=act)
    ins = [x_in] + ([r_in] if res else [])

    def fn(x, r=None):
        return E.bn_act(x, bn, act, residual=r, channels=channels, training=training, out=out)

    (y,), grads, store = _run(bn, fn, ins, [dy])
    got = dict(y=v3(y), dx=v3(grads[0]), dgamma=store.grad_of(bn.weight), dbeta=store.grad_of(bn.bias))
    if training:
        got.update(running_mean=bn.running_mean, running_var=bn.running_var)
    if out is not None:
        assert y.data_ptr() == out.data_ptr()
    _bn_check(tag, fwd, bwd, v3(xv), gamma, beta, v3(rv) if res else None, v3(dy), act=act, training=training,
              momentum=momentum, got=got, old=old)
    if res:
        assert torch.equal(grads[1], dy), "the residual's gradient is dy"
    return bn


@pytest.mark.parametrize("case", list(BN_CASES), ids=list(BN_CASES))
def test_bn_act_f32_vs_float64(case):
    shape, act, res, training, edges, layout = BN_CASES[case]
    bn = _bn_case(shape, act, res, training, edges, layout, seed=zlib.crc32(case.encode()) % 1000, tag=case)
    if case.startswith("count_one"):
        assert torch.isfinite(bn.running_var).all()


@pytest.mark.parametrize("eps,momentum", [(1e-3, 0.0), (0.5, 1.0), (1e-5, 1.0)])
@pytest.mark.parametrize("shape", [(8, 128, 13, 13), (2, 16, 40, 40)], ids=["fused", "wide"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_act_f32_eps_momentum(eps, momentum, shape, training):
    _bn_case(shape, 1, True, training, True, "dense", eps=eps, momentum=momentum, seed=7,
             tag=f"eps{eps}_mom{momentum}")


@pytest.mark.parametrize("B,C,T,H,W", [(2, 3, 12, 100, 100), (2, 4, 25, 110, 110)], ids=["235_splits", "256_cap"])
def test_bn3d_view_wide_splits(B, C, T, H, W):
    """BatchNorm3d on the [B, C*T, H, W] view (PreTimeReduction): C <= 8 channels of T*H*W values take up to
    BN_SPLIT_MAX = 256 partial rows each (235 at L = 120 000; the cap at L = 302 500)."""
    _bn_case((B, C * T, H, W), 1, False, True, True, "dense", channels=C, seed=11, tag=f"bn3d_C{C}_L{T * H * W}")


@pytest.mark.parametrize("shape", [(8, 128, 13, 13), (2, 16, 40, 40), (3, 8, 25, 25)], ids=["fused", "wide", "scalar"])
@pytest.mark.parametrize("training", [1, 0])
def test_bn_act_bwd_accumulate_flags_c_abi(shape, training):
    """cn_bn_act_bwd_f32 called directly with accumulate_dx = accumulate_params = 1 on prefilled buffers, and without
    a dx buffer (parameter gradients only)."""
    from cultionet_amd import _lib

    dev = _dev()
    B, C, H, W = shape
    L = H * W
    x = _x(shape, 21, edges=True)
    dy = _randn(shape, 22)
    bn = _bn_module(C, 23)
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    fwd = bn_fwd64(_flat3(x), gamma, beta, rm, rv, training=bool(training), momentum=0.1, eps=1e-5, act=1)
    bwd = bn_bwd64(fwd, gamma, _flat3(dy), training=bool(training), act=1)
    mean, rstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    y = torch.empty_like(x)
    ws = torch.empty(_lib.query("cn_bn_workspace_doubles", C), dtype=torch.float64, device=dev)
    _lib.call("cn_bn_act_fwd_f32", x.data_ptr(), C * L, gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(),
              None, 0, y.data_ptr(), C * L, mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), B, C, L, training, 0.1,
              1e-5, 1, _s())
    base = _randn(shape, 24)
    dx = base.clone()
    p0g, p0b = _randn((C,), 25), _randn((C,), 26)
    dg, db = p0g.clone(), p0b.clone()
    coef = torch.empty(2 * C, device=dev)
    _lib.call("cn_bn_act_bwd_f32", x.data_ptr(), C * L, dy.data_ptr(), C * L, mean.data_ptr(), rstd.data_ptr(),
              gamma.data_ptr(), beta.data_ptr(), dx.data_ptr(), C * L, dg.data_ptr(), db.data_ptr(), coef.data_ptr(),
              ws.data_ptr(), B, C, L, training, 1, 1, 1, _s())
    dg2, db2 = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    _lib.call("cn_bn_act_bwd_f32", x.data_ptr(), C * L, dy.data_ptr(), C * L, mean.data_ptr(), rstd.data_ptr(),
              gamma.data_ptr(), beta.data_ptr(), None, 0, dg2.data_ptr(), db2.data_ptr(), coef.data_ptr(),
              ws.data_ptr(), B, C, L, training, 1, 0, 0, _s())
    torch.cuda.synchronize()
    tag = f"acc_{'fused' if C >= 32 and B * L <= 2048 else 'wide'}_t{training}"
    _bn_check(tag, fwd, dict(bwd, dx=bwd["dx"] + _flat3(base).double(), dgamma=bwd["dgamma"] + p0g.double(),
                             dbeta=bwd["dbeta"] + p0b.double()), _flat3(x), gamma, beta, None, _flat3(dy), act=1,
              training=bool(training), momentum=0.1,
              got=dict(dx=_flat3(dx), dgamma=dg, dbeta=db), dx_prior=_flat3(base))
    _bn_check(tag + "_nodx", fwd, bwd, _flat3(x), gamma, beta, None, _flat3(dy), act=1, training=bool(training),
              momentum=0.1, got=dict(dgamma=dg2, dbeta=db2, mean=mean, rstd=rstd))


# ---------------------------------------------------------------------------------------------------------------------
# fp32 bn_act_group
# ---------------------------------------------------------------------------------------------------------------------

def _group_case(G, shape, summed, training, *, edges="f32", outs_slices=False, bns=None, tag="", dtype=torch.float32):
    """E.bn_act_group against G per-layer float64 references; returns nothing, asserts everything. bns: prebuilt layers
    (their eps / momentum / tracking may differ)."""
    from cultionet_amd import engine as E

    B, C = shape[0], shape[1]
    if bns is None:
        bns = [_bn_module(C, 200 + g) for g in range(G)]
    G = len(bns)
    mods = nn.ModuleList(bns)
    mods.train(training)
    bf16 = dtype == BF
    depth = bbn_depth(B * math.prod(shape[2:]), C) if bf16 else 0
    xs = [_x(shape, 300 + 7 * g, edges=edges) for g in range(G)]
    r = _randn(shape, 399) if summed else None
    dys = [_randn(shape, 400 + g) for g in range(1 if summed else G)]
    if bf16:
        xs = [t.to(BF).float() for t in xs]
        r = r.to(BF).float() if r is not None else None
        dys = [d.to(BF).float() for d in dys]
    olds = [(bn.running_mean.clone(), bn.running_var.clone()) if bn.running_mean is not None else (None, None)
            for bn in bns]
    fwds, bwds = [], []
    for g, bn in enumerate(bns):
        use_batch = training or bn.running_mean is None
        f = bn_fwd64(_flat3(xs[g]), bn.weight.detach(), bn.bias.detach(), olds[g][0], olds[g][1], training=use_batch,
                     momentum=bn.momentum, eps=bn.eps, act=1)
        if use_batch and not training:
            f.pop("running_mean", None)
            f.pop("running_var", None)
        fwds.append(f)
        bwds.append(bn_bwd64(f, bn.weight.detach(), _flat3(dys[0 if summed else g]), training=use_batch, act=1))
    if summed:  # res + f_0 + f_1 + ...: each layer's residual is the running sum before it
        acc = _flat3(r).double()
        ress = []
        for f in fwds:
            ress.append(acc)
            acc = acc + (f["y"])
        y_ref = acc
    outs = None
    if outs_slices:
        buf = torch.full((B, (1 if summed else G) * C + 3) + tuple(shape[2:]), float("nan"), device=_dev())
        outs = [buf[:, 1 + i * C:1 + (i + 1) * C] for i in range(1 if summed else G)]

    def to_dev(t):
        if not bf16:
            return t.contiguous()
        return t.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)

    ins = [to_dev(t) for t in xs] + ([to_dev(r)] if summed else [])

    def fn(*vs):
        return E.bn_act_group(list(vs[:G]), bns, E.ACT_SILU, residual=vs[G] if summed else None, sum_outputs=summed,
                              training=training, outs=outs if not bf16 else None)

    ys, grads, store = _run(mods, fn, ins, [to_dev(d) for d in dys])
    if outs is not None:
        assert all(y.data_ptr() == o.data_ptr() for y, o in zip(ys, outs))
    for g, bn in enumerate(bns):
        got = dict(dx=_flat3(grads[g].float()), dgamma=store.grad_of(bn.weight), dbeta=store.grad_of(bn.bias))
        if "running_mean" in fwds[g]:
            got.update(running_mean=bn.running_mean, running_var=bn.running_var)
        elif bn.running_mean is not None:
            assert torch.equal(bn.running_mean, olds[g][0]) and torch.equal(bn.running_var, olds[g][1]), \
                f"{tag}: eval must leave layer {g}'s running statistics alone"
        if not summed:
            got["y"] = _flat3(ys[g].float())
        _bn_check(f"{tag} layer{g}", fwds[g], bwds[g], _flat3(xs[g]), bn.weight.detach(), bn.bias.detach(),
                  ress[g] if summed else None, _flat3(dys[0 if summed else g]), act=1,
                  training=training or bn.running_mean is None, momentum=bn.momentum, got=got, old=olds[g], bf16=bf16,
                  depth=depth)
    if summed:
        # bound of the sum: the per-layer bounds added up (each layer adds its rounding to the running sum)
        from cultionet_amd import engine as E

        chained = bf16 and not E._bn_group_uniform(bns)  # one bn_act per layer: each running sum is stored in bf16
        bound = 0.0
        for g, bn in enumerate(bns):
            dm, _, rrel = _bn_stat_allowance(fwds[g], training or bn.running_mean is None, depth)
            bound = bound + _bn_y_bound(fwds[g], _flat3(xs[g]).double(), bn.weight.detach(), bn.bias.detach(), ress[g],
                                        dm, rrel)
            if chained and g < G - 1:
                bound = bound + _half_ulp16(ress[g + 1], bound)
        if bf16:
            bound = bound + _half_ulp16(y_ref, bound)
        _within(ys[0].float().reshape(y_ref.shape), y_ref, bound, f"{tag} sum")
        assert torch.equal(grads[G].float(), dys[0]), "the residual's gradient is dy"


@pytest.mark.parametrize("G", [1, 2, 3, 4])
@pytest.mark.parametrize("summed", [False, True], ids=["separate", "summed"])
def test_bn_act_group_f32(G, summed):
    _group_case(G, (4, 32, 25, 25), summed, True, tag=f"group G{G} summed{summed}")


@pytest.mark.parametrize("case", ["big_g2", "cap64_plane200", "slices", "eval", "fused_size"])
def test_bn_act_group_f32_shapes(case):
    if case == "big_g2":
        _group_case(2, (8, 128, 100, 100), True, True, tag=case)
    elif case == "cap64_plane200":  # C*G <= 16 and L > 32 256: BN_SPLIT_GROUP = 64 partial rows per channel
        _group_case(2, (2, 8, 200, 200), False, True, tag=case)
    elif case == "slices":
        _group_case(3, (2, 16, 50, 50), False, True, outs_slices=True, tag=case)
        _group_case(2, (2, 16, 50, 50), True, True, outs_slices=True, tag=case + " summed")
    elif case == "eval":
        _group_case(2, (4, 32, 25, 25), True, False, tag=case)
    else:
        _group_case(2, (8, 256, 13, 13), True, True, tag=case)


def _mixed_layers(C, what):
    if what == "eps":
        return [_bn_module(C, 500, eps=1e-5), _bn_module(C, 501, eps=1e-3)]
    if what == "momentum":
        return [_bn_module(C, 502, momentum=0.1), _bn_module(C, 503, momentum=0.3)]
    return [_bn_module(C, 504), _bn_module(C, 505, track=False)]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("summed", [False, True], ids=["separate", "summed"])
@pytest.mark.parametrize("what", ["eps", "momentum", "tracking"])
def test_bn_act_group_layers_that_differ(what, summed, training, dtype):
    """A group whose layers differ in eps, momentum or track_running_stats: every output, gradient and running statistic
    against each layer's own float64 reference (the grouped launch takes one eps / momentum for all layers)."""
    C = 32
    _group_case(2, (4, C, 20, 20), summed, training, bns=_mixed_layers(C, what), edges="bf16" if dtype == BF else "f32",
                tag=f"mixed {what}", dtype=dtype)


def test_bn_act_group_bf16_layers_that_differ_write_outs():
    """bf16, summed, two layers of different eps (one bn_act per layer): the result lands in the caller's ``outs``
    buffer, with the values of the same call without ``outs``."""
    from cultionet_amd import engine as E

    B, C, H, W = 4, 32, 20, 20
    bns = _mixed_layers(C, "eps")
    mods = nn.ModuleList(bns).train()
    ins = [_x((B, C, H, W), 310 + g, edges="bf16").to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
           for g in range(2)]
    dy = _randn((B, C, H, W), 410).to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    buf = torch.full((B, H, W, C), float("nan"), dtype=BF, device=_dev()).permute(0, 3, 1, 2)

    def fn(outs):
        return lambda *vs: E.bn_act_group(list(vs), bns, E.ACT_SILU, sum_outputs=True, training=True, outs=outs)

    (y_ref,), dx_ref, _ = _run(mods, fn(None), ins, [dy])
    (y,), dx, _ = _run(mods, fn([buf]), ins, [dy])
    assert y.data_ptr() == buf.data_ptr()
    assert torch.equal(buf, y_ref)
    for g in range(2):
        assert torch.equal(dx[g], dx_ref[g])


# ---------------------------------------------------------------------------------------------------------------------
# bf16 bn_act / bn_act_group, and the statistics epilogue of the convolution
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [32, 128])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_bn_act_bf16_batch32(C, training):
    shape = (32, C, 100, 100)
    _group_case(1, shape, True, training, edges="bf16", tag=f"bf16 b32 C{C}", dtype=BF)


def test_bn_act_group_bf16_edges():
    """bf16 group with a constant channel (its sums are exact, so it is held to the fp32 bound: a wrong rstd there
    changes dx) and a channel at mean/std ~ 4 (fp32 sums: the variance allowance grows by (m^2 + s^2)/(s^2 + eps))."""
    bns = [_bn_module(32, 600), _bn_module(32, 601)]
    _group_case(2, (8, 32, 25, 25), True, True, bns=bns, tag="bf16 edges", dtype=BF, edges="bf16")
    _group_case(2, (8, 32, 25, 25), False, True, tag="bf16 edges separate", dtype=BF, edges="bf16")


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("H", [100, 50], ids=["rows_2500_tiles", "finished_in_launch"])
def test_bn_act_bf16_from_conv_statistics(G, H):
    """conv2d(want_stats, bn) -> bn_act / bn_act_group at batch 32, the production pairing. At 100x100 a 128-cout
    convolution has 2560 pixel tiles (> 1008): the BatchNorm finishes the conv epilogue's fp32 rows (conv_sums). At
    50x50 (< 1008 tiles) the convolution launch finishes them itself and the BatchNorm only applies them
    (conv_rows = -1).
    Reference: the statistics of the float64 convolution, applied to the stored bf16 conv output. Their allowance adds
    to the fp32-chain terms (tile rows of <= 128 pixels: D = 128) the convolution's own error E = K*u*(|x|*|w|) per
    pixel (bf16 products are exact in fp32, K = 9*Cin terms): mean(E) for the mean, mean(2|y|E) + 2|m|mean(E) for the
    variance."""
    from cultionet_amd import engine as E

    dev = _dev()
    B, Cin, Cout, W = 32, 32, 128, H
    convs = [nn.Conv2d(Cin, Cout, 3, padding=1 + g, dilation=1 + g, bias=False).to(dev) for g in range(G)]
    bns = [_bn_module(Cout, 620 + g) for g in range(G)]
    for conv in convs:
        with torch.no_grad():
            conv.weight.copy_(conv.weight.to(BF).float())
    mods = nn.ModuleList(convs + bns).train()
    x = _randn((B, Cin, H, W), 630).to(BF).float()
    r = _randn((B, Cout, H, W), 631).to(BF).float()
    dy = _randn((B, Cout, H, W), 632).to(BF).float()
    nhwc = lambda t: t.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    olds = [(bn.running_mean.clone(), bn.running_var.clone()) for bn in bns]
    store = E.ParamStore(mods)
    store.zero_grad()
    with E.using_store(store):
        with E.recording(False):
            ys = [E.conv2d(E.Var(nhwc(x)), convs[g], 1, 1 + g, 1 + g, want_stats=True, bn=bns[g]) for g in range(G)]
        for y in ys:
            assert y.stats is not None
            assert (y.bnfin is not None) == (H == 50), "the 1008-tile limit decides who finishes the statistics"
            y.req = True
        with E.recording(True) as tape:
            rv = E.Var(nhwc(r), True)
            out = E.bn_act_group(ys, bns, E.ACT_SILU, residual=rv, sum_outputs=True) if G > 1 else \
                E.bn_act(ys[0], bns[0], E.ACT_SILU, residual=rv)
            out.grad = nhwc(dy)
            tape.backward()
    torch.cuda.synchronize()
    acc = _flat3(r).double()
    bound = 0.0
    for g in range(G):
        c64 = torch.nn.functional.conv2d(x.double(), convs[g].weight.double(), padding=1 + g, dilation=1 + g)
        E64 = 9 * Cin * U * torch.nn.functional.conv2d(x.double().abs(), convs[g].weight.double().abs(), padding=1 + g,
                                                        dilation=1 + g)
        m64, v64 = c64.mean(dim=(0, 2, 3)), c64.var(dim=(0, 2, 3), unbiased=False)
        y16 = _flat3(ys[g].t.float())
        gamma, beta = bns[g].weight.detach(), bns[g].bias.detach()
        fwd = bn_fwd64(y16, gamma, beta, m64, v64, training=False, momentum=0.1, eps=1e-5, act=1, res=acc)
        n = B * H * W
        fwd["running_mean"] = 0.9 * olds[g][0].double() + 0.1 * m64
        fwd["running_var"] = 0.9 * olds[g][1].double() + 0.1 * v64 * n / (n - 1)
        bwd = bn_bwd64(fwd, gamma, _flat3(dy), training=True, act=1)
        Em = E64.mean(dim=(0, 2, 3))
        stat_err = (Em, 2 * (c64.abs() * E64).mean(dim=(0, 2, 3)) + 2 * m64.abs() * Em)
        got = dict(dx=_flat3(ys[g].grad.float()), dgamma=store.grad_of(bns[g].weight),
                   dbeta=store.grad_of(bns[g].bias), running_mean=bns[g].running_mean,
                   running_var=bns[g].running_var)
        if G == 1:
            got["y"] = _flat3(out.t.float())
        _bn_check(f"conv stats G{G} H{H} layer{g}", fwd, bwd, y16, gamma, beta, acc, _flat3(dy), act=1, training=True,
                  momentum=0.1, got=got, old=olds[g], bf16=True, depth=128, stat_err=stat_err)
        dm, _, rrel = _bn_stat_allowance(fwd, True, 128, stat_err)
        bound = bound + _bn_y_bound(fwd, y16.double(), gamma, beta, acc, dm, rrel)
        acc = fwd["y"]
    if G > 1:
        _within(_flat3(out.t.float()), acc, bound + _half_ulp16(acc, bound), f"conv stats G{G} H{H} sum")


def _pack16(w):
    from cultionet_amd import _lib

    Cout, Cin = w.shape[0], w.shape[1]
    n = _lib.query("cn_bconv_packed_elems", 9, Cin, Cout)
    wp = torch.empty(n, dtype=BF, device=_dev())
    _lib.call("cn_pack_weights_bf16", w.data_ptr(), wp.data_ptr(), 9, Cin, Cout, 9, Cin * 9, 1, _s())
    return wp


@pytest.mark.parametrize("B,Cin,H,W,Cout,G,offset,expect", [
    (7, 32, 100, 100, 32, 2, 0.0, 1),     # 560 tiles: finished in the launch
    (12, 16, 100, 100, 128, 1, 0.0, 1),   # 960 tiles of 128 pixels
    (14, 16, 100, 100, 128, 1, 0.0, 0),   # 1120 tiles > 1008: rows only
    (8, 32, 25, 25, 128, 2, 4.0, 1),      # mean/std = 4 (see the docstring)
])
def test_conv_bnstats_finalize_vs_float64(B, Cin, H, W, Cout, G, offset, expect):
    """cn_conv2d_fwd_grouped_bnstats_bf16: the launch's own finalize (last-block tickets) against float64 formulas on
    its per-tile rows -- mean, rstd and running statistics to c*u -- twice in a row on one workspace (the tickets must
    return to zero), and the rows against the float64 convolution: |sum rows - sum conv64| <= (K + 128) * u *
    sum |x| * |w| (bf16 products are exact in fp32; K = 9 * Cin terms per output, <= 128 per tile row).
    offset: a constant added to the input's first channel with a matching weight, so a channel's mean/std is ~4.
    The rows are fp32, so E[y^2] - m^2 cancels (m^2 + s^2)/s^2 = 17: the rstd is asserted at 16 * u * D * 17."""
    from cultionet_amd import _lib

    dev = _dev()
    P = B * H * W
    x = _randn((B, Cin, H, W), 31)
    x[:, 0] += offset
    x = x.to(BF).float()
    wts = []
    for g in range(G):
        w = _randn((Cout, Cin, 3, 3), 32 + g, 1.0 / math.sqrt(9 * Cin))
        if offset:
            w[:, 0, 1, 1] = 0.5
        wts.append(w.to(BF).float())
    pads = dils = [1 + (g % 2) for g in range(G)]
    xg = x.to(BF).permute(0, 2, 3, 1).contiguous()
    wps = [_pack16(w) for w in wts]
    ys = [torch.empty((B, H, W, Cout), dtype=BF, device=dev) for _ in range(G)]
    rows = _lib.query("cn_conv2d_stats_rows_bf16", B, H, W, Cout, 3, 3, 1, max(pads), max(dils))
    stats = [torch.full((rows, 2, Cout), float("nan"), device=dev) for _ in range(G)]
    rm = [_randn((Cout,), 40 + g, 0.1) for g in range(G)]
    rv = [0.5 + torch.rand(Cout, generator=_gen(50 + g), device=dev) for g in range(G)]
    mean = torch.full((G, Cout), float("nan"), device=dev)
    rstd = torch.full((G, Cout), float("nan"), device=dev)
    nws = _lib.query("cn_bn_group_workspace_floats_bf16", G, Cout)
    ws = torch.zeros(nws, device=dev)
    fin = ctypes.c_int(-7)
    conv64 = [torch.nn.functional.conv2d(x.double(), wts[g].double(), padding=pads[g], dilation=dils[g])
              for g in range(G)]
    absconv = [torch.nn.functional.conv2d(x.double().abs(), wts[g].double().abs(), padding=pads[g], dilation=dils[g])
               for g in range(G)]
    for rep in range(2):
        olds = [(rm[g].clone(), rv[g].clone()) for g in range(G)]
        _lib.call("cn_conv2d_fwd_grouped_bnstats_bf16", G, _tab([xg.data_ptr()] * G), Cin,
                  _tab([w.data_ptr() for w in wps]), _tab([y.data_ptr() for y in ys]), Cout, B, Cin, H, W, Cout, 3, 3,
                  1, (ctypes.c_int * G)(*pads), (ctypes.c_int * G)(*dils), _tab([t.data_ptr() for t in stats]),
                  _tab([mean[g].data_ptr() for g in range(G)]), _tab([rstd[g].data_ptr() for g in range(G)]),
                  _tab([t.data_ptr() for t in rm]), _tab([t.data_ptr() for t in rv]), 0.1, 1e-5, ws.data_ptr(), nws,
                  ctypes.byref(fin), _s())
        torch.cuda.synchronize()
        assert fin.value == expect
        for g in range(G):
            srow = stats[g].double().sum(0)
            _within(stats[g][:, 0].double().sum(0), conv64[g].sum(dim=(0, 2, 3)),
                    (9 * Cin + 128) * U * absconv[g].sum(dim=(0, 2, 3)), f"finalize rows sum g{g}")
            if not expect:
                continue
            m64 = srow[0] / P
            var64 = (srow[1] / P - m64 ** 2).clamp_min(0)
            s64 = var64.sqrt()
            _within(mean[g], m64, C_F32 * U * (m64.abs() + s64), f"finalize mean g{g} rep{rep}")
            _within(rstd[g], 1 / torch.sqrt(var64 + 1e-5), C_F32 * U / torch.sqrt(var64 + 1e-5),
                    f"finalize rstd g{g} rep{rep}")
            rmr = 0.9 * olds[g][0].double() + 0.1 * m64
            rvr = 0.9 * olds[g][1].double() + 0.1 * var64 * P / (P - 1)
            _within(rm[g], rmr, C_F32 * U * (olds[g][0].double().abs() + 0.1 * (m64.abs() + s64)),
                    f"finalize running_mean g{g}")
            _within(rv[g], rvr, C_F32 * U * (olds[g][1].double().abs() + 0.1 * var64 * P / (P - 1)),
                    f"finalize running_var g{g}")
            # against the float64 convolution itself: the rows' fp32 squares cancel by cond
            mc = conv64[g].mean(dim=(0, 2, 3))
            vc = conv64[g].var(dim=(0, 2, 3), unbiased=False)
            # the rows' fp32 squares (tile sums of <= 128 pixels) and the convolution's own error E reach the variance
            Ec = 9 * Cin * U * absconv[g]
            dvc = 3 * 128 * U * (mc ** 2 + vc) + 2 * (conv64[g].abs() * Ec).mean(dim=(0, 2, 3)) + 2 * mc.abs() * Ec.mean(
                dim=(0, 2, 3))
            _within(rstd[g], 1 / torch.sqrt(vc + 1e-5), (C_F32 * U + 0.5 * dvc / (vc + 1e-5)) / torch.sqrt(vc + 1e-5),
                    f"finalize rstd vs conv64 g{g}")
            _within(mean[g], mc, (9 * Cin + 128) * U * absconv[g].mean(dim=(0, 2, 3)) + C_F32 * U * (mc.abs() + vc.sqrt()),
                    f"finalize mean vs conv64 g{g}")
        if expect:
            head = ws[:_lib.query("cn_bn_workspace_head_ints")].view(torch.int32)
            assert int(head.abs().sum()) == 0, "ticket counters left non-zero"
        else:
            assert torch.isnan(mean).all()


# ---------------------------------------------------------------------------------------------------------------------
# eval fold, channel sums
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", [False, True])
def test_conv_bn_act_eval_fold_vs_float64(bias):
    """conv_bn_act_eval: cn_bn_fold_f32 (scale / shift to c*u) and the fused launch against float64 conv -> eval
    BatchNorm -> SiLU (+ residual). The folded weights W * scale are rounded to bf16: per output
    |err| <= 2^-8 * (|x| * |W'|) + (K + 8) * u * (|x| * |W'|) + c*u*|shift| + the SiLU, + half a bf16 ulp of |y64|."""
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    dev = _dev()
    B, Cin, H, W, Cout = 4, 64, 25, 25, 128
    conv = nn.Conv2d(Cin, Cout, 3, padding=1, bias=bias).to(dev)
    bn = _bn_module(Cout, 700).eval()
    with torch.no_grad():
        bn.running_mean[0] = 30.0  # a large frozen offset
        bn.running_var[1] = 0.0    # a frozen constant channel: scale = gamma / sqrt(eps)
        conv.weight.copy_(conv.weight.to(BF).float())
    x = _randn((B, Cin, H, W), 701).to(BF).float()
    r = _randn((B, Cout, H, W), 702).to(BF).float()
    g64, b64 = bn.weight.detach().double(), bn.bias.detach().double()
    sc64 = g64 / torch.sqrt(bn.running_var.double() + bn.eps)
    cb = conv.bias.detach().double() if bias else torch.zeros(Cout, dtype=torch.float64, device=dev)
    sh64 = b64 - bn.running_mean.double() * sc64 + cb * sc64
    scale, shift = torch.empty(Cout, device=dev), torch.empty(Cout, device=dev)
    _lib.call("cn_bn_fold_f32", bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
              bn.running_var.data_ptr(), conv.bias.data_ptr() if bias else None, float(bn.eps), Cout, scale.data_ptr(),
              shift.data_ptr(), _s())
    torch.cuda.synchronize()
    _within(scale, sc64, C_F32 * U * sc64.abs(), "fold scale")
    _within(shift, sh64, C_F32 * U * (b64.abs() + (bn.running_mean.double().abs() + cb.abs()) * sc64.abs()),
            "fold shift")
    conv64 = torch.nn.functional.conv2d(x.double(), conv.weight.double(), cb if bias else None, padding=1)
    z = (conv64 - bn.running_mean.double()[None, :, None, None]) * sc64[None, :, None, None] \
        + b64[None, :, None, None]
    y64 = z / (1 + torch.exp(-z)) + r.double()
    wabs = conv.weight.double().abs() * sc64.abs()[:, None, None, None]
    mag = torch.nn.functional.conv2d(x.double().abs(), wabs, padding=1)
    bound = 1.1 * ((2.0 ** -8 + (9 * Cin + 8) * U) * mag + C_F32 * U * (sh64.abs()[None, :, None, None] + z.abs())) \
        + C_F32 * U * r.double().abs()
    bound = bound + _half_ulp16(y64, bound)
    store = E.ParamStore(nn.ModuleList([conv, bn]))
    xv = E.Var(x.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    rvv = E.Var(r.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    with E.using_store(store), E.recording(False):
        assert E.can_fuse_eval(xv, bn, False)
        y = E.conv_bn_act_eval(xv, conv, bn, E.ACT_SILU, 1, 1, 1, residual=rvv)
    torch.cuda.synchronize()
    _within(y.t.float(), y64, bound, f"eval fold y bias{bias}")


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape,odd", [((8, 32, 100, 100), False), ((8, 128, 25, 25), True), ((3, 5, 200, 200), False)])
def test_channel_sum_f32(shape, odd, accumulate):
    """cn_channel_sum_f32 (bias gradients): fp64 block sums, one fp32 atomic per block and channel:
    |err| <= c*u*(|prior| + sum|x|) per channel."""
    from cultionet_amd import _lib

    dev = _dev()
    B, C = shape[0], shape[1]
    L = shape[2] * shape[3]
    x = _slice_of(shape, odd=odd) if odd else torch.empty(shape, device=dev)
    x.copy_(_randn(shape, 800, 2.0, 0.5))
    prior = _randn((C,), 801, 100.0)
    out = prior.clone()
    _lib.call("cn_channel_sum_f32", x.data_ptr(), x.stride(0), B, C, L, out.data_ptr(), accumulate, _s())
    torch.cuda.synchronize()
    ref = x.double().sum(dim=(0, 2, 3)) + (prior.double() if accumulate else 0.0)
    bound = C_F32 * U * (x.double().abs().sum(dim=(0, 2, 3)) + (prior.double().abs() if accumulate else 0.0))
    _within(out, ref, bound, f"channel_sum acc{accumulate}")


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------

def _ln_case(shape, *, res, out_slice, accumulate, edges, seed, tag, bf16=False):
    from cultionet_amd import engine as E

    B, C = shape[0], shape[1]
    ln = nn.LayerNorm(C, eps=1e-5).to(_dev())
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        ln.weight.copy_(1 + 0.2 * torch.randn(C, generator=g))
        ln.bias.copy_(0.2 * torch.randn(C, generator=g))
    x = _randn(shape, seed + 1, 1.5) + _randn((B, 1) + tuple(shape[2:]), seed + 2, 1.0)
    if edges:
        x[:, :, 0, 0] = 0.5  # a constant row (var = 0)
        if bf16:
            x[:, :, 0, 1] = x[:, :, 0, 1] * 0.25 + 1.5  # mean/std ~ 4
        else:
            x[:, :, 0, 1] = x[:, :, 0, 1] * 0.01 + 10.0  # mean/std ~ 1e3
    r = _randn(shape, seed + 3) if res else None
    dy = _randn(shape, seed + 4)
    prior = _randn(shape, seed + 5) if accumulate else None
    if bf16:
        x, dy = x.to(BF).float(), dy.to(BF).float()
        r = r.to(BF).float() if r is not None else None
    fwd = ln_fwd64(_flat3(x), ln.weight.detach(), ln.bias.detach(), eps=1e-5, res=_flat3(r) if res else None)
    bwd = ln_bwd64(fwd, ln.weight.detach(), _flat3(dy))
    out = None
    if out_slice:
        buf = torch.full((B, C + 7) + tuple(shape[2:]), float("nan"), device=_dev())
        out = buf[:, 3:3 + C]
    to_dev = (lambda t: t.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)) if bf16 else (lambda t: t)

    def fn(xv, rv=None):
        return E.layer_norm_c(xv, ln, rv, out=out)

    ins = [to_dev(x)] + ([to_dev(r)] if res else [])
    if accumulate:  # a gradient already waiting in x's buffer (a second consumer)
        store = E.ParamStore(ln)
        store.zero_grad()
        with E.using_store(store), E.recording(True) as tape:
            vs = [E.Var(t, True) for t in ins]
            vs[0].grad = to_dev(prior).clone()
            yv = fn(*vs)
            yv.grad = to_dev(dy)
            tape.backward()
        torch.cuda.synchronize()
        y, grads = yv.t, [v.grad for v in vs]
    else:
        (y,), grads, store = _run(ln, fn, ins, [to_dev(dy)])
    if out is not None:
        assert y.data_ptr() == out.data_ptr()
    bwd_got = dict(bwd)
    prior3 = None
    if accumulate:
        prior3 = _flat3(prior.to(BF).float() if bf16 else prior).double()
        bwd_got["dx"] = bwd["dx"] + prior3
    got = dict(y=_flat3(y.float()), dx=_flat3(grads[0].float()), dw=store.grad_of(ln.weight),
               db=store.grad_of(ln.bias))
    _ln_check(tag, fwd, bwd_got, _flat3(x), ln.weight.detach(), ln.bias.detach(), _flat3(r) if res else None,
              _flat3(dy), got, bf16=bf16, dx_prior=prior3)


LN_CASES = {f"C{C}": ((2, C, 20, 20), False, False, False) for C in (8, 32, 33, 64, 65, 128, 129, 256, 512)}
LN_CASES.update({
    "C32_160k_pixels": ((16, 32, 100, 100), True, False, False),
    "C128_160k_pixels": ((16, 128, 100, 100), False, True, True),
    "C128_b8": ((8, 128, 100, 100), True, True, False),
    "C256_res_slice_acc": ((4, 256, 13, 13), True, True, True),
    "C65_acc": ((3, 65, 17, 9), False, False, True),
})


@pytest.mark.parametrize("case", list(LN_CASES), ids=list(LN_CASES))
def test_layer_norm_f32_vs_float64(case):
    shape, res, out_slice, acc = LN_CASES[case]
    _ln_case(shape, res=res, out_slice=out_slice, accumulate=acc, edges=True, seed=900 + len(case), tag=f"ln {case}")


@pytest.mark.parametrize("C,res", [(32, True), (128, False)])
def test_layer_norm_bf16_batch32(C, res):
    _ln_case((32, C, 100, 100), res=res, out_slice=False, accumulate=False, edges=True, seed=950, tag=f"ln bf16 C{C}",
             bf16=True)


def test_layer_norm_over_512_channels_is_refused_before_any_launch():
    """cn_layernorm_c_bwd_f32 refuses C > 512; the forward runs at any width. With a tape the engine refuses at the
    forward, before anything is launched; without one the forward matches the reference."""
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    C, shape = 520, (2, 520, 6, 7)
    ln = nn.LayerNorm(C).to(_dev())
    x = _randn(shape, 990)
    store = E.ParamStore(ln)
    with E.using_store(store), E.recording(True):
        out = torch.full(shape, float("nan"), device=_dev())
        with pytest.raises(NotImplementedError, match="512"):
            E.layer_norm_c(E.Var(x, True), ln, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), "nothing may be written before the refusal"
        xb = x.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        with pytest.raises(NotImplementedError, match="512"):
            E.layer_norm_c(E.Var(xb, True), ln)
    with E.using_store(store), E.recording(False):
        y = E.layer_norm_c(E.Var(x), ln)
    torch.cuda.synchronize()
    fwd = ln_fwd64(_flat3(x), ln.weight.detach(), ln.bias.detach(), eps=ln.eps)
    _ln_check("ln C520 forward", fwd, None, _flat3(x), ln.weight.detach(), ln.bias.detach(), None, None,
              dict(y=_flat3(y.t)))
    P = shape[0] * shape[2] * shape[3]
    mu = torch.empty(P, device=_dev())
    dw = torch.zeros(C, device=_dev())
    rc = _lib.load().cn_layernorm_c_bwd_f32(x.data_ptr(), C * 42, x.data_ptr(), C * 42, ln.weight.data_ptr(),
                                            mu.data_ptr(), mu.data_ptr(), out.data_ptr(), C * 42, dw.data_ptr(),
                                            dw.data_ptr(), 2, C, 42, 0, None, 0, _s())
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(out).all(), "the C ABI refuses the backward over C > 512 without writing"
