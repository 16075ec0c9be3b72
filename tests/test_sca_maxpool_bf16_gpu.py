"""The bf16 NHWC kernels of attention_weights="spatial_channel" (SpatialChannelAttention, reference
nn/modules/attention.py:12-126) and pool_by_max=True (F.adaptive_max_pool2d, convolution.py:499-503), through the C ABI
and through the engine, against torch float64 on the CPU evaluated on the SAME bf16-rounded inputs.

Tolerances: fp32 outputs (pools, d ca, d sconv, d gamma, MLP / conv weight gradients) <= 1e-4 relative to the tensor's
max |ref|; bf16 outputs within one bf16 rounding of the float64 result (<= 2^-8 relative to the tensor's max |ref|).
"Few-valued" inputs are drawn from a handful of values so that ties are certain: the H*W max and the max-pool windows
route the gradient to the FIRST maximum (ATen), the channel max (einops 'max' = torch.amax) splits it evenly.
"""
import pytest
import torch
import torch.nn.functional as F

from pointwise_ref import sca_ref64 as _sca_ref64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32_TOL = 1e-4
BF_TOL = 2.0 ** -8


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _input(shape, seed, few=False, scale=1.0):
    """bf16-representable fp32 CPU values; few=True draws from 5 values (ties everywhere)."""
    g = torch.Generator().manual_seed(seed)
    if few:
        return (torch.randint(-2, 3, shape, generator=g).float() * 0.5 * scale).to(BF).float()
    return (torch.randn(shape, generator=g) * scale).to(BF).float()


def _nhwc(t, ld=None, fill=0.0):
    """[B,C,H,W] fp32 CPU -> logical NCHW view of a bf16 NHWC GPU buffer with pixel stride ld (a channel slice when
    ld > C: the columns past C hold `fill` and must survive every call)."""
    B, C, H, W = t.shape
    ld = ld or C
    buf = torch.full((B, H, W, ld), fill, dtype=BF, device=_dev())
    buf[..., :C] = t.permute(0, 2, 3, 1).to(BF).to(_dev())
    return buf[..., :C].permute(0, 3, 1, 2), buf


def _close(got, ref, rel, what):
    got = got.detach().float().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got - ref).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} > {rel * scale:.3e} (scale {scale:.3e})"


def _untouched(buf, C, fill, what):
    assert bool((buf[..., C:].float() == fill).all()), f"{what}: columns past C were written"


def _call(name, *args):
    from cultionet_amd import _lib

    _lib.call(name, *args)


def _ws(B, C, L):
    from cultionet_amd import _lib

    n = _lib.query("cn_sca_workspace_floats_bf16", B, C, L)
    assert n > 0
    return torch.full((n,), float("nan"), device=_dev()), n


# ---------------------------------------------------------------------------
# spatial-channel attention: C ABI
# ---------------------------------------------------------------------------
SCA_CASES = [
    # B, C, H, W, ld, few-valued
    (2, 32, 28, 28, None, False),
    (1, 96, 25, 25, None, True),
    (2, 96, 25, 25, 128, False),   # channel slice of a wider buffer
    (3, 128, 50, 50, None, False),
    (1, 128, 100, 100, None, True),
    (2, 256, 100, 100, None, False),
    (4, 256, 28, 28, 264, True),
]


@pytest.mark.parametrize("B,C,H,W,ld,few", SCA_CASES)
def test_sca_pool_fwd_bf16(B, C, H, W, ld, few):
    x = _input((B, C, H, W), seed=C + H, few=few)
    xv, _ = _nhwc(x, ld)
    L = H * W
    f = lambda *s: torch.full(s, float("nan"), device=_dev())
    avg, mx, pooled = f(B, C), f(B, C), f(B, 2, H, W)
    idx = torch.full((B, C), -7, dtype=torch.int32, device=_dev())
    ws, n = _ws(B, C, L)
    _call("cn_sca_pool_fwd_bf16", xv.data_ptr(), xv.stride(3), B, C, L, avg.data_ptr(), mx.data_ptr(), idx.data_ptr(),
          pooled.data_ptr(), ws.data_ptr(), n, _s())
    torch.cuda.synchronize()
    x64 = x.double()
    _close(avg, x64.mean((2, 3)), F32_TOL, "avg")
    rmx, ridx = F.adaptive_max_pool2d(x64, 1, return_indices=True)  # first maximum (ATen)
    assert torch.equal(mx.cpu().double(), rmx.view(B, C)), "mx"
    assert torch.equal(idx.cpu().long(), ridx.view(B, C)), "idx (first maximum)"
    _close(pooled[:, 0], x64.mean(1), F32_TOL, "channel mean")
    assert torch.equal(pooled[:, 1].cpu().double(), x64.amax(1)), "channel max"
    if few:
        assert bool((ridx.view(B, C) > 0).any())  # ties really occurred before the chosen index


@pytest.mark.parametrize("B,C,H,W,ld,few", SCA_CASES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_sca_pool_bwd_bf16(B, C, H, W, ld, few, accumulate):
    x = _input((B, C, H, W), seed=2 * C + H, few=few)
    xv, _ = _nhwc(x, ld)
    L = H * W
    davg, dmx = _input((B, C), seed=3, scale=4.0), _input((B, C), seed=4, scale=4.0)
    dpool = _input((B, 2, H, W), seed=5)
    base = _input((B, C, H, W), seed=6, scale=0.05)
    dxv, dxbuf = _nhwc(base if accumulate else torch.zeros_like(base), ld, fill=3.0)
    idx = F.adaptive_max_pool2d(x, 1, return_indices=True)[1].view(B, C).int()
    dg = [t.to(_dev()) for t in (davg, dmx, idx, dpool)]  # held until the kernel has run
    _call("cn_sca_pool_bwd_bf16", xv.data_ptr(), xv.stride(3), dg[0].data_ptr(), dg[1].data_ptr(), dg[2].data_ptr(),
          dg[3].data_ptr(), dxv.data_ptr(), dxv.stride(3), B, C, L, accumulate, _s())
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    tot = (x64.mean((2, 3)) * davg.double()).sum() + (F.adaptive_max_pool2d(x64, 1).view(B, C) * dmx.double()).sum() \
        + (x64.mean(1) * dpool[:, 0].double()).sum() + (x64.amax(1) * dpool[:, 1].double()).sum()
    tot.backward()
    ref = x64.grad + (base.double() if accumulate else 0.0)
    _close(dxv, ref, BF_TOL, "dskip")
    _untouched(dxbuf, C, 3.0, "dskip")


@pytest.mark.parametrize("B,C,H,W,ld,few", SCA_CASES)
def test_sca_apply_fwd_bwd_bf16(B, C, H, W, ld, few):
    out = _input((B, C, H, W), seed=C + 7, few=few)
    dy = _input((B, C, H, W), seed=C + 8)
    ca = torch.sigmoid(_input((B, C), seed=9))
    sconv = _input((B, 1, H, W), seed=10, scale=2.0)
    gamma = torch.tensor([0.9])
    ov, _ = _nhwc(out, ld)
    dyv, _ = _nhwc(dy, ld)
    L = H * W
    yv, ybuf = _nhwc(torch.zeros(B, C, H, W), ld, fill=3.0)
    cag, sg, gg = ca.cuda(), sconv.cuda(), gamma.cuda()
    _call("cn_sca_apply_fwd_bf16", ov.data_ptr(), ov.stride(3), cag.data_ptr(), sg.data_ptr(), gg.data_ptr(),
          yv.data_ptr(), yv.stride(3), B, C, L, _s())
    o64, ca64, s64, g64 = (t.double().requires_grad_(True) for t in (out, ca, sconv, gamma))
    y64 = o64 * (1 + g64 * 0.5 * (ca64.view(B, C, 1, 1) + torch.sigmoid(s64)))
    y64.backward(dy.double())
    torch.cuda.synchronize()
    _close(yv, y64, BF_TOL, "y")
    _untouched(ybuf, C, 3.0, "y")
    ws, n = _ws(B, C, L)
    for accumulate in (0, 1):
        base = _input((B, C, H, W), seed=11, scale=0.1)
        dov, dobuf = _nhwc(base if accumulate else torch.full_like(base, float("nan")), ld, fill=3.0)
        dca = torch.full((B, C), float("nan"), device=_dev())
        dsconv = torch.full((B, 1, H, W), float("nan"), device=_dev())
        dgamma = torch.tensor([0.25], device=_dev())  # accumulated into
        _call("cn_sca_apply_bwd_bf16", dyv.data_ptr(), dyv.stride(3), ov.data_ptr(), ov.stride(3), cag.data_ptr(),
              sg.data_ptr(), gg.data_ptr(), dov.data_ptr(), dov.stride(3), accumulate, dca.data_ptr(),
              dsconv.data_ptr(), dgamma.data_ptr(), ws.data_ptr(), n, B, C, L, _s())
        torch.cuda.synchronize()
        _close(dov, o64.grad + (base.double() if accumulate else 0.0), BF_TOL, f"dout acc={accumulate}")
        _untouched(dobuf, C, 3.0, "dout")
        _close(dca, ca64.grad, F32_TOL, "dca")
        _close(dsconv, s64.grad, F32_TOL, "dsconv")
        _close(dgamma - 0.25, g64.grad, F32_TOL, "dgamma")
    # bit-reproducible: the same call twice gives identical sums
    d2 = torch.empty_like(dca)
    s2 = torch.empty_like(dsconv)
    g2 = torch.zeros(1, device=_dev())
    g3 = torch.zeros(1, device=_dev())
    for dc, dg in ((d2, g2), (dca, g3)):
        _call("cn_sca_apply_bwd_bf16", dyv.data_ptr(), dyv.stride(3), ov.data_ptr(), ov.stride(3), cag.data_ptr(),
              sg.data_ptr(), gg.data_ptr(), None, 0, 0, dc.data_ptr(), s2.data_ptr(), dg.data_ptr(), ws.data_ptr(), n,
              B, C, L, _s())
    torch.cuda.synchronize()
    assert torch.equal(d2, dca) and torch.equal(g2, g3)


@pytest.mark.parametrize("B,C,H,W,few", [(2, 32, 28, 28, False), (1, 96, 25, 25, True), (2, 128, 50, 50, False),
                                          (2, 256, 100, 100, True)])
def test_sca_engine_bf16(B, C, H, W, few):
    """engine.spatial_channel_attention on bf16 Vars: y, d skip, d out and every parameter gradient (the MLPs, the 3x3
    conv, gamma) against float64 autograd."""
    from cultionet_amd import engine as E
    from cultionet_amd.convolution import SpatialChannelAttention

    torch.manual_seed(C)
    mod = SpatialChannelAttention(C, "SiLU")
    with torch.no_grad():
        mod.gamma.fill_(0.8)  # nonzero: the attention path carries gradient
    skip = _input((B, C, H, W), seed=C + 20, few=few)
    out = _input((B, C, H, W), seed=C + 21)
    dy = _input((B, C, H, W), seed=C + 22)
    s64, o64 = skip.double().requires_grad_(True), out.double().requires_grad_(True)
    y64, pw = _sca_ref64(mod, s64, o64)
    y64.backward(dy.double())
    mod = mod.to(_dev())
    store = E.ParamStore(mod)
    store.zero_grad()
    with E.using_store(store), E.recording(True) as tape:
        sv, ov = E.Var(_nhwc(skip)[0], True), E.Var(_nhwc(out)[0], True)
        yv = E.spatial_channel_attention(sv, ov, mod)
        assert yv.t.dtype == BF
        yv.grad = _nhwc(dy)[0]
        tape.backward()
    torch.cuda.synchronize()
    _close(yv.t, y64, BF_TOL, "y")
    _close(ov.grad, o64.grad, BF_TOL, "dout")
    _close(sv.grad, s64.grad, BF_TOL, "dskip")
    for n, p in mod.named_parameters():
        _close(store.grad_of(p), pw[n].grad, F32_TOL, n)


# ---------------------------------------------------------------------------
# adaptive max pool
# ---------------------------------------------------------------------------
POOL_CASES = [
    # B, C, Hi, Wi, Ho, Wo, ld, few
    (2, 32, 28, 28, 14, 14, None, False),
    (2, 64, 7, 7, 3, 3, None, True),         # overlapping windows
    (3, 128, 25, 25, 12, 12, None, True),    # down_d at the 100 px chip: overlapping windows
    (1, 128, 100, 100, 50, 50, 136, False),  # channel slice
    (2, 24, 25, 25, 12, 12, 32, False),      # width 24: a multiple of 8, not 8 * 2^n
]


@pytest.mark.parametrize("B,C,Hi,Wi,Ho,Wo,ld,few", POOL_CASES)
def test_adaptive_maxpool_bf16(B, C, Hi, Wi, Ho, Wo, ld, few):
    x = _input((B, C, Hi, Wi), seed=Hi + C, few=few)
    xv, _ = _nhwc(x, ld)
    yv, ybuf = _nhwc(torch.zeros(B, C, Ho, Wo), ld, fill=3.0)
    idx = torch.full((B, Ho, Wo, C), -7, dtype=torch.int32, device=_dev())
    _call("cn_adaptive_maxpool_fwd_bf16", xv.data_ptr(), xv.stride(3), yv.data_ptr(), yv.stride(3), idx.data_ptr(), B,
          C, Hi, Wi, Ho, Wo, _s())
    x64 = x.double().requires_grad_(True)
    y64, i64 = F.adaptive_max_pool2d(x64, (Ho, Wo), return_indices=True)
    dy = _input((B, C, Ho, Wo), seed=Ho)
    y64.backward(dy.double())
    torch.cuda.synchronize()
    assert torch.equal(yv.float().cpu().double(), y64.detach()), "y"
    assert torch.equal(idx.permute(0, 3, 1, 2).cpu().long(), i64), "idx (first maximum of the window)"
    _untouched(ybuf, C, 3.0, "y")
    # eval form: no index output
    y2, _ = _nhwc(torch.zeros(B, C, Ho, Wo), ld)
    _call("cn_adaptive_maxpool_fwd_bf16", xv.data_ptr(), xv.stride(3), y2.data_ptr(), y2.stride(3), None, B, C, Hi, Wi,
          Ho, Wo, _s())
    torch.cuda.synchronize()
    assert torch.equal(y2.float().cpu(), yv.float().cpu())
    dyv, _ = _nhwc(dy, ld)
    for accumulate in (0, 1):
        base = _input((B, C, Hi, Wi), seed=1, scale=0.1)
        dxv, dxbuf = _nhwc(base if accumulate else torch.full_like(base, float("nan")), ld, fill=3.0)
        _call("cn_adaptive_maxpool_bwd_bf16", dyv.data_ptr(), dyv.stride(3), idx.data_ptr(), dxv.data_ptr(),
              dxv.stride(3), B, C, Hi, Wi, Ho, Wo, accumulate, _s())
        torch.cuda.synchronize()
        _close(dxv, x64.grad + (base.double() if accumulate else 0.0), BF_TOL, f"dx acc={accumulate}")
        _untouched(dxbuf, C, 3.0, "dx")


def test_adaptive_maxpool_engine_bf16():
    """engine.adaptive_max_pool2d on a bf16 Var under the tape (28 -> 14), and with the tape off (no index buffer)."""
    from cultionet_amd import engine as E

    B, C, H, W = 2, 40, 28, 28
    x = _input((B, C, H, W), seed=77, few=True)
    dy = _input((B, C, 14, 14), seed=78)
    x64 = x.double().requires_grad_(True)
    y64 = F.adaptive_max_pool2d(x64, (14, 14))
    y64.backward(dy.double())
    with E.recording(True) as tape:
        xv = E.Var(_nhwc(x)[0], True)
        yv = E.adaptive_max_pool2d(xv, (14, 14))
        yv.grad = _nhwc(dy)[0]
        tape.backward()
    with E.recording(False):
        ye = E.adaptive_max_pool2d(E.Var(_nhwc(x)[0]), (14, 14))
    torch.cuda.synchronize()
    assert yv.t.dtype == BF and torch.equal(yv.t.float().cpu().double(), y64.detach())
    assert torch.equal(ye.t.float().cpu(), yv.t.float().cpu())
    _close(xv.grad, x64.grad, BF_TOL, "dx")
