"""The bf16 NHWC kernels of attention_weights="spatial_channel" (SpatialChannelAttention, reference
nn/modules/attention.py:12-126) and pool_by_max=True (F.adaptive_max_pool2d, convolution.py:499-503), through the C ABI
and through the engine, against torch float64 on the CPU evaluated on the SAME bf16-rounded inputs.

Tolerances: fp32 outputs (pools, d ca, d sconv, d gamma, MLP / conv weight gradients) <= 1e-4 relative to the tensor's
max |ref|; bf16 outputs per element, by the bounds of tests/pointwise_ref.py that tests/test_sca_maxpool_bf16_exact_gpu.py
derives from the kernels: the fp32 roundings on the way to the element plus half a bf16 ulp at the element's own |ref|.
"Few-valued" inputs are drawn from a handful of values so that ties are certain: the H*W max and the max-pool windows
route the gradient to the FIRST maximum (ATen), the channel max (einops 'max' = torch.amax) splits it evenly.
"""
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from conv_exact_worker import bounded, half_ulp_bf16
from pointwise_ref import sca_ref64 as _sca_ref64

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32_TOL = 1e-4
ROUTE = 1e-4  # the engine tests' routing allowance (test_pointwise_exact_gpu.py::test_sca_engine_f32), per element


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
    g, A = R.sca_pool_bwd_terms64(x.double(), davg.double(), dmx.double(), dpool.double())
    ref = sum(g) + (base.double() if accumulate else 0.0)
    bounded(dxv, ref, R.sca_pool_bwd_bound(ref, A, base.double() if accumulate else None),
            f"sca pool bwd bf16 {B}x{C}x{H}x{W} acc={accumulate} dskip")
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
    _, _, _, _, att, mag, e_att = R.sca_att64(ca.double(), sconv.double(), float(gamma))
    bounded(yv, *R.sca_gate_bound(out.double(), att, mag, e_att), f"sca apply bf16 {B}x{C}x{H}x{W} y")
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
        bounded(dov, *R.sca_gate_bound(dy.double(), att, mag, e_att, base.double() if accumulate else None),
                f"sca apply bf16 {B}x{C}x{H}x{W} dout acc={accumulate}")
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


def _route_bound(ref, A):
    """Per element: 1e-4 of A (the absolute terms that make up the element) and the store's half bf16 ulp."""
    return ROUTE * A + half_ulp_bf16(ref.abs() + ROUTE * A)


class _handed_to:
    """Copies of fp32 arguments of one C-ABI entry point, taken when the engine calls it inside the block:
    floats = {argument index: element count}; afterwards self.got[index] is a CPU float32 tensor."""

    def __init__(self, name, floats):
        self.name, self.floats, self.got = name, floats, {}

    def __enter__(self):
        import ctypes

        from cultionet_amd import _lib

        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        hip.hipMemcpy.restype = ctypes.c_int
        self.lib, self.orig = _lib, _lib.call

        def call(name, *args):
            if name == self.name:
                torch.cuda.synchronize()  # everything the arguments depend on has run
                for i, n in self.floats.items():
                    host = torch.empty(n, dtype=torch.float32)
                    assert hip.hipMemcpy(host.data_ptr(), args[i], 4 * n, 2) == 0  # device to host
                    self.got[i] = host
            return self.orig(name, *args)

        _lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.orig
        return False


@pytest.mark.parametrize("B,C,H,W,few", [(2, 32, 28, 28, False), (1, 96, 25, 25, True), (2, 128, 50, 50, False),
                                          (2, 256, 100, 100, True)])
def test_sca_engine_bf16(B, C, H, W, few):
    """engine.spatial_channel_attention on bf16 Vars: y, d skip, d out and every parameter gradient (the MLPs, the 3x3
    conv, gamma) against float64 autograd.

    d skip is checked in the two steps it is made in. The fp32 davg, dmx (channel MLPs' backward) and d pooled (the 3x3
    conv's backward of d sconv) that the engine hands to cn_sca_pool_bwd_bf16 are copied at the call and held to this
    file's rule for fp32 tensors, 1e-4 of the tensor's max |ref|. The kernel's result is then held per element to its
    own bound (7 roundings on the four absolute terms and half a bf16 ulp, pointwise_ref.sca_pool_bwd_bound) against
    float64 on exactly those handed values: nothing there is scaled by a tensor's maximum.
    End to end against float64 autograd, d skip is within 1e-4 of the element's own four absolute path gradients plus
    half a bf16 ulp where C <= 128. At [2,256,100,100] that form cannot hold: d pooled is a sum of 9 taps of d sconv,
    itself a sum over 256 channels, so its error is relative to the sums' terms, not to its own value, and among
    20000 pixels some have a d pooled hundreds of times smaller than the tensor's maximum; dpool1 / n (about 50 tied
    channels) is then all of the element and carries that error whole. The two steps above bound exactly that."""
    from cultionet_amd import engine as E
    from cultionet_amd.convolution import SpatialChannelAttention

    torch.manual_seed(C)
    mod = SpatialChannelAttention(C, "SiLU")
    with torch.no_grad():
        mod.gamma.fill_(0.8)  # nonzero: the attention path carries gradient
    skip = _input((B, C, H, W), seed=C + 20, few=few)
    out = _input((B, C, H, W), seed=C + 21)
    dy = _input((B, C, H, W), seed=C + 22)
    o64 = out.double().requires_grad_(True)
    y64, pw, leaves = _sca_ref64(mod, skip.double(), o64, paths=True)
    y64.backward(dy.double())
    dskip64 = sum(l.grad for l in leaves)  # the four pool paths into skip
    mod = mod.to(_dev())
    store = E.ParamStore(mod)
    store.zero_grad()
    L = H * W
    with E.using_store(store), E.recording(True) as tape, \
            _handed_to("cn_sca_pool_bwd_bf16", {2: B * C, 3: B * C, 5: B * 2 * L}) as handed:
        sv, ov = E.Var(_nhwc(skip)[0], True), E.Var(_nhwc(out)[0], True)
        yv = E.spatial_channel_attention(sv, ov, mod)
        assert yv.t.dtype == BF
        yv.grad = _nhwc(dy)[0]
        tape.backward()
    torch.cuda.synchronize()
    what = f"sca engine bf16 {B}x{C}x{H}x{W}"
    bounded(yv.t, y64.detach(), _route_bound(y64.detach(), y64.detach().abs()), what + " y")
    bounded(ov.grad, o64.grad, _route_bound(o64.grad, o64.grad.abs()), what + " dout")
    g64 = [l.grad for l in leaves]
    davg, dmx, dpool = handed.got[2].view(B, C).double(), handed.got[3].view(B, C).double(), \
        handed.got[5].view(B, 2, H, W).double()
    _close(davg, g64[0][:, :, 0, 0] * L, F32_TOL, "davg handed to the pool backward")
    _close(dmx, g64[1].sum((2, 3)), F32_TOL, "dmx handed to the pool backward")
    _close(dpool[:, 0], g64[2][:, 0] * C, F32_TOL, "d pooled (mean) handed to the pool backward")
    _close(dpool[:, 1], g64[3].sum(1), F32_TOL, "d pooled (max) handed to the pool backward")
    gk, Ak = R.sca_pool_bwd_terms64(skip.double(), davg, dmx, dpool)
    bounded(sv.grad, sum(gk), R.sca_pool_bwd_bound(sum(gk), Ak), what + " dskip against float64 on the handed gradients")
    if C <= 128:
        bounded(sv.grad, dskip64, _route_bound(dskip64, sum(g.abs() for g in g64)), what + " dskip")
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
    dy = _input((B, C, Ho, Wo), seed=Ho)
    y64, i64, dx64, dxa, cnt = R.maxpool_bwd64(x.double(), dy.double(), (Ho, Wo))
    torch.cuda.synchronize()
    assert torch.equal(yv.float().cpu().double(), y64), "y"
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
        ref = dx64 + (base.double() if accumulate else 0.0)
        bounded(dxv, ref, R.bf16_store_bound(ref, cnt, dxa, base.double() if accumulate else None),
                f"max pool bf16 {B}x{C} {Hi}x{Wi}->{Ho}x{Wo} dx acc={accumulate}")
        _untouched(dxbuf, C, 3.0, "dx")


def test_adaptive_maxpool_engine_bf16():
    """engine.adaptive_max_pool2d on a bf16 Var under the tape (28 -> 14), and with the tape off (no index buffer)."""
    from cultionet_amd import engine as E

    B, C, H, W = 2, 40, 28, 28
    x = _input((B, C, H, W), seed=77, few=True)
    dy = _input((B, C, 14, 14), seed=78)
    y64, _, dx64, dxa, cnt = R.maxpool_bwd64(x.double(), dy.double(), (14, 14))
    with E.recording(True) as tape:
        xv = E.Var(_nhwc(x)[0], True)
        yv = E.adaptive_max_pool2d(xv, (14, 14))
        yv.grad = _nhwc(dy)[0]
        tape.backward()
    with E.recording(False):
        ye = E.adaptive_max_pool2d(E.Var(_nhwc(x)[0]), (14, 14))
    torch.cuda.synchronize()
    assert yv.t.dtype == BF and torch.equal(yv.t.float().cpu().double(), y64)
    assert torch.equal(ye.t.float().cpu(), yv.t.float().cpu())
    bounded(xv.grad, dx64, R.bf16_store_bound(dx64, cnt, dxa), "max pool engine bf16 dx")
