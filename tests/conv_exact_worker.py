"""Exact-arithmetic checks of the convolution kernels, shared by tests/test_conv_exact_gpu.py and run on its own as the
child process of the forced tile / split sweep:

    CN_DBG_CFG=<cfg> CN_DBG_SPLITS=<splits> python tests/conv_exact_worker.py

Integer inputs (x in -4..4, weights and upstream gradients in -3..3, biases in -8..8, some zeros) make every product
and every partial sum an integer. While the sum of the absolute terms of every output stays below 2^24 each of them
is exact in fp32, whatever the tile, summation order, K split, slice reduce or atomic order, so an fp32 result must
EQUAL the float64 reference and a bf16 result must equal it rounded to nearest even. `premise` asserts that bound
(from max|a| * max|b| * terms, which is >= conv(|a|, |b|)) for every output of every check.

The outputs live in sentinel-filled buffers (padded batch strides for fp32 NCHW, pixel-stride padding lanes for bf16
NHWC, slack after the end); inputs sit in buffers whose gaps hold a finite garbage value, which no result may pick up.
"""
from __future__ import annotations

import contextlib
import math
import os
import sys

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
LIMIT = 2.0 ** 24
SENT = -7776.0  # sentinel of output buffers: exact in fp32 and bf16
GARB = 992.0    # gaps of input buffers: exact in fp32 and bf16, never part of a result
SLACK = 64      # sentinel elements after the end of every output buffer
BF = torch.bfloat16
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# inputs, premise, references
# ---------------------------------------------------------------------------------------------------------------------

def ints(shape, lo, hi, seed, zeros=0.15):
    """Integers in [lo, hi] as float64, about `zeros` of them 0."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).double()
    t[torch.rand(tuple(shape), generator=g, dtype=torch.float64) < zeros] = 0.0
    return t


def term_bound(a, b, terms):
    """max|a| * max|b| * terms: an upper bound of every element of conv(|a|, |b|) with `terms` products per output."""
    return float(a.abs().max()) * float(b.abs().max()) * terms


def premise(what, *bounds):
    """Every partial sum of every output is an integer below 2^24 in magnitude: fp32 holds all of them exactly."""
    total = float(sum(bounds))
    assert total < LIMIT, f"{what}: exact premise fails, |partial sums| may reach {total:.0f} >= 2^24"
    return total


def out_size(H, W, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1


def ref_conv(x, w, b, dy, stride=1, pad=0, dil=1):
    """float64 y, dx, dw of nn.Conv2d."""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    y = F.conv2d(x, w, None if b is None else b.double(), stride, pad, dil)
    dx, dw = torch.autograd.grad(y, (x, w), dy.double())
    return y.detach(), dx, dw


def ref_convT(x, w, b, dy, stride, pad, op=0):
    """float64 y, dx, dw of nn.ConvTranspose2d (weight [Cin][Cout][k][k])."""
    x = x.double().requires_grad_(True)
    w = w.double().requires_grad_(True)
    y = F.conv_transpose2d(x, w, None if b is None else b.double(), stride, pad, output_padding=op)
    dx, dw = torch.autograd.grad(y, (x, w), dy.double())
    return y.detach(), dx, dw


def rb(t):
    """Round to bf16 (nearest even), as float64."""
    return t.float().to(BF).double()


def assert_exact(got, ref, what):
    got = got.detach().double().cpu()
    ref = ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = got != ref
        idx = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ; first at {idx}: "
                             f"got {float(got[idx])}, want {float(ref[idx])}")


def bounded(got, ref, bound, what):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"BOUND {what}: worst err/bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: err/bound {ratio:.3f}"


def half_ulp_bf16(v):
    """Half a bf16 ulp at |v| (as float64): spacing 2^(e-8) in the binade [2^(e-1), 2^e)."""
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), e - 9)


# ---------------------------------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------------------------------

class Canvas:
    """A [B,C,H,W] tensor inside a filled buffer: fp32 NCHW with batch stride `pitch` (>= C*H*W), or bf16 NHWC with
    pixel stride `pitch` (>= C, a multiple of 8), followed by SLACK more elements."""

    def __init__(self, shape, dtype, dev, pitch=None, fill=SENT, data=None):
        B, C, H, W = shape
        self.shape, self.dtype, self.fill = tuple(shape), dtype, fill
        if dtype == F32:
            self.pitch = pitch or C * H * W
            n = B * self.pitch
        else:
            self.pitch = pitch or (C + 7) // 8 * 8
            assert self.pitch % 8 == 0 and self.pitch >= C
            n = B * H * W * self.pitch
        self.buf = torch.full((n + SLACK,), fill, dtype=dtype, device=dev)
        self.t = self.view(self.buf)
        if data is not None:
            self.t.copy_(data.to(dev).to(dtype))

    def view(self, buf):
        B, C, H, W = self.shape
        if self.dtype == F32:
            return buf[:B * self.pitch].view(B, self.pitch)[:, :C * H * W].view(B, C, H, W)
        return buf[:B * H * W * self.pitch].view(B, H, W, self.pitch)[..., :C].permute(0, 3, 1, 2)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def assert_canary(self, what):
        c = self.buf.clone()
        self.view(c).fill_(self.fill)
        assert torch.equal(c, torch.full_like(c, self.fill)), f"{what}: written outside the tensor"


NAN = float("nan")
RED = 9  # roundings of cn_block_sum<float, 256>: 6 wave levels + 3 adds of the four wave totals


def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def canary(cv, what):
    """Canvas.assert_canary that also works for a NaN fill."""
    c = cv.buf.clone()
    cv.view(c).fill_(cv.fill)
    ok = bool(c.isnan().all()) if cv.fill != cv.fill else bool((c == cv.fill).all())
    assert ok, f"{what}: written outside the tensor"


class Flat:
    """A dense tensor of any shape at the front of a filled buffer with SLACK elements behind it."""

    def __init__(self, shape, dev, fill=NAN, dtype=F32, data=None):
        self.n, self.fill = math.prod(int(d) for d in shape), fill
        self.buf = torch.full((self.n + SLACK,), fill, dtype=dtype, device=dev)
        self.t = self.buf[:self.n].view(*shape)
        if data is not None:
            self.t.copy_(data.to(dev).to(dtype))

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def assert_slack(self, what):
        s = self.buf[self.n:]
        ok = bool(s.isnan().all()) if self.fill != self.fill else bool((s == self.fill).all())
        assert ok, f"{what}: written past the end"


def same(got, ref, what):
    """torch.equal that lets NaN equal NaN."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok = (got == ref) | (got.isnan() & ref.isnan())
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ref.numel()} differ; first at {tuple((~ok).nonzero()[0].tolist())}"


def act_err(v, e_v, a):
    """Error of an fp32 sigmoid / SiLU a(v) evaluated at v +- e_v: slope within [-0.1, 1.1] times e_v, plus
    (|v| + 8) u relative for the expf, the add and the division (see test_fused_bf16_random_bound)."""
    return 1.1 * e_v + (v.abs() + e_v + 8) * U32 * (a.abs() + e_v)


def lib():
    from cultionet_amd import _lib

    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack_f32(wd, T, K, N, sk, sn, st):
    L = lib()
    n = T * L.query("cn_conv_kpad", K) * L.query("cn_conv_npad", N)
    wp = torch.full((n,), float("nan"), device=wd.device)
    L.call("cn_pack_weights_f32", wd.data_ptr(), wp.data_ptr(), T, K, N, sk, sn, st, stream())
    return wp


def pack_bf16(wd, T, K, N, sk, sn, st, nscale=None):
    L = lib()
    n = L.query("cn_bconv_packed_elems", T, K, N)
    wp = torch.full((n,), float("nan"), dtype=BF, device=wd.device)
    if nscale is None:
        L.call("cn_pack_weights_bf16", wd.data_ptr(), wp.data_ptr(), T, K, N, sk, sn, st, stream())
    else:
        L.call("cn_pack_weights_scaled_bf16", wd.data_ptr(), nscale.data_ptr(), wp.data_ptr(), T, K, N, sk, sn, st,
               stream())
    return wp


class conv_workspace:
    """Split-K scratch of the current stream for the block: "ws" registers one (slice-and-reduce), "none" unregisters
    (float atomics). Afterwards the engine binds its own again on its next launch."""

    def __init__(self, mode, floats=16 << 20):
        self.mode, self.floats = mode, floats

    def __enter__(self):
        self.ws = torch.empty(self.floats, device="cuda") if self.mode == "ws" else None
        lib().call("cn_conv_set_workspace", stream(), None if self.ws is None else self.ws.data_ptr(),
                   0 if self.ws is None else self.floats)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        lib().call("cn_conv_set_workspace", stream(), None, 0)
        from cultionet_amd import engine as E

        E._conv_ws.clear()
        return False


def wgrad_ws_f32(B, Cin, H, W, Cout, Ho, Wo, mode):
    """(pointer, floats) of the fp32 weight-gradient scratch: "full" as the engine sizes it, "none" the dword
    fallback for operands that are not 16-byte friendly."""
    if mode == "none":
        return None, 0, None
    n = (16 << 20) + B * (Cout * (Ho * (Wo + 1) + 3) + Cin * (H * (W + 1) + 3))
    ws = torch.empty(n, device="cuda")
    return ws.data_ptr(), n, ws


# ---------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------

def part(routes, label, *facts):
    """routes.part(label, *facts) of a tests/route_ledger.py Routes, or nothing to record (the forced sweep's children:
    forcing a tile and a split is their purpose)."""
    return contextlib.nullcontext() if routes is None else routes.part(label, *facts)


def check_conv_f32(case, seed=0, accumulate=False, xpad=0, ypad=0, wgrad_ws="full", parts=("y", "dx", "dw"), routes=None,
                   tag=""):
    """cn_conv2d_{fwd,bwd_data,bwd_weight}_f32 on integer inputs: equal to float64. case: B, Cin, H, W, Cout, k,
    stride, pad, dil, bias. xpad / ypad: extra batch-stride elements of the inputs / outputs. routes: the recorder
    of the calling test, which learns the route of every part under the label tag + part."""
    B, Cin, H, W, Cout, k, s, p, d, bias = case
    T = k * k
    Ho, Wo = out_size(H, W, k, s, p, d)
    x = ints((B, Cin, H, W), -4, 4, seed)
    w = ints((Cout, Cin, k, k), -3, 3, seed + 1)
    b = ints((Cout,), -8, 8, seed + 2) if bias else None
    dy = ints((B, Cout, Ho, Wo), -3, 3, seed + 3)
    y0 = ints((B, Cout, Ho, Wo), -8, 8, seed + 4) if accumulate else torch.zeros(B, Cout, Ho, Wo, dtype=torch.float64)
    x0 = ints((B, Cin, H, W), -8, 8, seed + 5) if accumulate else torch.zeros(B, Cin, H, W, dtype=torch.float64)
    w0 = ints((Cout, Cin, k, k), -8, 8, seed + 6)  # the weight gradient always accumulates
    premise(f"conv f32 {case}", term_bound(x, w, Cin * T), 8 + 8)
    premise(f"conv f32 {case} dx", term_bound(dy, w, Cout * T), 8)
    premise(f"conv f32 {case} dw", term_bound(x, dy, B * Ho * Wo), 8)
    y64, dx64, dw64 = ref_conv(x, w, b, dy, s, p, d)
    dev = torch.device("cuda")
    L, st = lib(), stream()
    wd = w.float().to(dev)
    bd = b.float().to(dev) if bias else None
    acc = int(accumulate)
    if "y" in parts:
        xc = Canvas(x.shape, F32, dev, pitch=Cin * H * W + xpad, fill=GARB, data=x)
        yc = Canvas(y64.shape, F32, dev, pitch=Cout * Ho * Wo + ypad, data=y0 if accumulate else None)
        wp = pack_f32(wd, T, Cin, Cout, T, Cin * T, 1)
        with part(routes, tag + "y"):
            L.call("cn_conv2d_fwd_f32", xc.ptr, xc.pitch, wp.data_ptr(), None if bd is None else bd.data_ptr(), yc.ptr,
                   yc.pitch, B, Cin, H, W, Cout, k, k, s, p, d, acc, st)
        torch.cuda.synchronize()
        assert_exact(yc.t, y64 + y0, f"y {case}")
        yc.assert_canary(f"y {case}")
    if "dx" in parts:
        dyc = Canvas(dy.shape, F32, dev, pitch=Cout * Ho * Wo + ypad, fill=GARB, data=dy)
        dxc = Canvas(x.shape, F32, dev, pitch=Cin * H * W + xpad, data=x0 if accumulate else None)
        wpt = pack_f32(wd, T, Cout, Cin, Cin * T, T, 1)
        with part(routes, tag + "dx"):
            L.call("cn_conv2d_bwd_data_f32", dyc.ptr, dyc.pitch, wpt.data_ptr(), dxc.ptr, dxc.pitch, B, Cin, H, W, Cout,
                   k, k, s, p, d, acc, st)
        torch.cuda.synchronize()
        assert_exact(dxc.t, dx64 + x0, f"dx {case}")
        dxc.assert_canary(f"dx {case}")
    if "dw" in parts:
        xc = Canvas(x.shape, F32, dev, pitch=Cin * H * W + xpad, fill=GARB, data=x)
        dyc = Canvas(dy.shape, F32, dev, pitch=Cout * Ho * Wo + ypad, fill=GARB, data=dy)
        dwc = Canvas(w.shape, F32, dev, data=w0)
        wsp, wsn, _keep = wgrad_ws_f32(B, Cin, H, W, Cout, Ho, Wo, wgrad_ws)
        with part(routes, tag + "dw", "ws " + wgrad_ws):
            L.call("cn_conv2d_bwd_weight_f32", xc.ptr, xc.pitch, dyc.ptr, dyc.pitch, dwc.ptr, B, Cin, H, W, Cout, k, k, s,
                   p, d, wsp, wsn, st)
        torch.cuda.synchronize()
        assert_exact(dwc.t, dw64 + w0, f"dw {case} ws={wgrad_ws}")
        dwc.assert_canary(f"dw {case}")


def bwgrad_ws_floats(B, Cin, H, W, Cout, k, s, p, d, transposed, mode):
    """bf16 weight-gradient scratch: "full" (cn_bwgrad_workspace_floats), "one" (exactly one split's slice), "mid"."""
    full = lib().query("cn_bwgrad_workspace_floats", B, Cin, H, W, Cout, k, k, s, p, d, transposed)
    one = ((Cout + 63) // 64 * 64) * ((Cin + 63) // 64 * 64) * k * k
    if mode == "full":
        return full
    if mode == "one":
        return min(one, full)
    return min(full, max(one, int((one * full) ** 0.5)))


def bf16_store(v, old, cout, accumulate):
    """The bf16 store of the conv epilogue: bf16(v), or with accumulate bf16(bf16(v) + old) when Cout % 8 == 0 (the
    16-byte stores round the result, then add) and bf16(v + old) for ragged couts (element-wise stores)."""
    if not accumulate:
        return rb(v)
    return rb(rb(v) + old) if cout % 8 == 0 else rb(v + old)


def check_conv_bf16(case, seed=0, accumulate=False, xpad=8, ypad=16, wgrad_ws="full", parts=("y", "dx", "dw"),
                    routes=None, tag=""):
    """cn_conv2d_fwd_bf16 (bf16 NHWC and fp32 NCHW outputs), cn_conv2d_bwd_data_bf16, cn_conv2d_bwd_weight_bf16 on
    integer inputs: bf16 results equal float64 rounded to nearest even, fp32 ones equal float64. routes: as in
    check_conv_f32 (parts "y", "y f32 out", "dx", "dw")."""
    B, Cin, H, W, Cout, k, s, p, d, bias = case
    T = k * k
    Ho, Wo = out_size(H, W, k, s, p, d)
    x = ints((B, Cin, H, W), -4, 4, seed)
    w = ints((Cout, Cin, k, k), -3, 3, seed + 1)
    b = ints((Cout,), -8, 8, seed + 2) if bias else None
    dy = ints((B, Cout, Ho, Wo), -3, 3, seed + 3)
    y0 = ints((B, Cout, Ho, Wo), -8, 8, seed + 4) if accumulate else None
    x0 = ints((B, Cin, H, W), -8, 8, seed + 5) if accumulate else None
    w0 = ints((Cout, Cin, k, k), -8, 8, seed + 6)
    premise(f"conv bf16 {case}", term_bound(x, w, Cin * T), 16)
    premise(f"conv bf16 {case} dx", term_bound(dy, w, Cout * T), 8)
    premise(f"conv bf16 {case} dw", term_bound(x, dy, B * Ho * Wo), 8)
    y64, dx64, dw64 = ref_conv(x, w, b, dy, s, p, d)
    dev = torch.device("cuda")
    L, st = lib(), stream()
    wd = w.float().to(dev)
    bd = b.float().to(dev) if bias else None
    acc = int(accumulate)
    c8 = lambda c: (c + 7) // 8 * 8
    xc = Canvas(x.shape, BF, dev, pitch=c8(Cin) + xpad, fill=GARB, data=x)
    dyc = Canvas(dy.shape, BF, dev, pitch=c8(Cout) + ypad, fill=GARB, data=dy)
    if "y" in parts:
        wp = pack_bf16(wd, T, Cin, Cout, T, Cin * T, 1)
        yc = Canvas(y64.shape, BF, dev, pitch=c8(Cout) + ypad, data=y0)
        with part(routes, tag + "y"):
            L.call("cn_conv2d_fwd_bf16", xc.ptr, xc.pitch, wp.data_ptr(), None if bd is None else bd.data_ptr(), yc.ptr,
                   yc.pitch, 0, B, Cin, H, W, Cout, k, k, s, p, d, acc, 0, None, st)
        torch.cuda.synchronize()
        assert_exact(yc.t, bf16_store(y64, y0, Cout, accumulate), f"y bf16 {case}")
        yc.assert_canary(f"y bf16 {case}")
        # fp32 NCHW output (the thin heads' hand-over), padded batch stride
        y32 = Canvas(y64.shape, F32, dev, pitch=Cout * Ho * Wo + 4, data=y0)
        with part(routes, tag + "y f32 out"):
            L.call("cn_conv2d_fwd_bf16", xc.ptr, xc.pitch, wp.data_ptr(), None if bd is None else bd.data_ptr(),
                   y32.ptr, 0, y32.pitch, B, Cin, H, W, Cout, k, k, s, p, d, acc, 1, None, st)
        torch.cuda.synchronize()
        assert_exact(y32.t, y64 + (y0 if accumulate else 0), f"y f32 out {case}")
        y32.assert_canary(f"y f32 out {case}")
    if "dx" in parts:
        wpt = pack_bf16(wd, T, Cout, Cin, Cin * T, T, 1)
        dxc = Canvas(x.shape, BF, dev, pitch=c8(Cin) + xpad, data=x0)
        with part(routes, tag + "dx"):
            L.call("cn_conv2d_bwd_data_bf16", dyc.ptr, dyc.pitch, wpt.data_ptr(), dxc.ptr, dxc.pitch, B, Cin, H, W, Cout,
                   k, k, s, p, d, acc, st)
        torch.cuda.synchronize()
        assert_exact(dxc.t, bf16_store(dx64, x0, Cin, accumulate), f"dx bf16 {case}")
        dxc.assert_canary(f"dx bf16 {case}")
    if "dw" in parts:
        n = bwgrad_ws_floats(B, Cin, H, W, Cout, k, s, p, d, 0, wgrad_ws)
        ws = torch.empty(n + 4, device=dev)
        dwc = Canvas(w.shape, F32, dev, data=w0)
        with part(routes, tag + "dw", "ws " + wgrad_ws):
            L.call("cn_conv2d_bwd_weight_bf16", xc.ptr, xc.pitch, dyc.ptr, dyc.pitch, dwc.ptr, B, Cin, H, W, Cout, k, k,
                   s, p, d, ws.data_ptr(), n, st)
        torch.cuda.synchronize()
        assert_exact(dwc.t, dw64 + w0, f"dw bf16 {case} ws={wgrad_ws}")
        dwc.assert_canary(f"dw bf16 {case}")


# ---------------------------------------------------------------------------------------------------------------------
# the forced tile / split sweep (one child per (CN_DBG_CFG, CN_DBG_SPLITS) pair)
# ---------------------------------------------------------------------------------------------------------------------

SWEEP_F32 = [
    # B, Cin, H, W, Cout, k, stride, pad, dil, bias
    (2, 64, 13, 13, 128, 3, 1, 1, 1, True),    # NT 128, 16-byte odd-plane kernel: 3 tile configs, 8 K chunks
    (2, 72, 12, 12, 40, 3, 1, 1, 1, True),     # NT 64, 16-byte kernel
    (1, 40, 10, 7, 20, 3, 1, 2, 2, True),      # NT 32, dword kernel (H*W % 4 == 2), dilated
    (2, 48, 9, 9, 136, 3, 2, 1, 1, False),     # strided gather, ragged NT 128 tiles
]
SWEEP_BF16 = [(2, 64, 13, 13, 64, 3, 1, 1, 1, True), (1, 32, 25, 25, 40, 3, 1, 2, 2, False)]


def sweep():
    for mode in ("ws", "none"):
        with conv_workspace(mode):
            for i, case in enumerate(SWEEP_F32):
                check_conv_f32(case, seed=100 + i, parts=("y", "dx"))
                check_conv_f32(case, seed=110 + i, accumulate=True, parts=("y",))
    for i, case in enumerate(SWEEP_F32[:2]):
        check_conv_f32(case, seed=120 + i, parts=("dw",))
    for i, case in enumerate(SWEEP_BF16):
        check_conv_bf16(case, seed=130 + i, wgrad_ws="mid")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")
    import cultionet_amd

    cultionet_amd.configure_runtime()
    assert torch.cuda.is_available(), "the sweep worker needs a GPU"
    sweep()
    print("conv_exact_worker: ok", os.environ.get("CN_DBG_CFG"), os.environ.get("CN_DBG_SPLITS"), flush=True)
