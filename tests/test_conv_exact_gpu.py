"""Every convolution entry point against float64, exactly.

Layer 1 (exact): integer inputs keep every partial sum an exact fp32 integer (tests/conv_exact_worker.py states the
premise and asserts it per check), so fp32 results must equal the float64 reference and bf16 results must equal it
rounded to nearest even -- compared with torch.equal, no tolerance. Epilogues that round twice by design (accumulating
or adding a residual into bf16) are restated in the reference. Outputs sit in sentinel-filled buffers with padded batch
strides / pixel strides and slack after the end; the sentinels must survive.

Layer 2 (bounded): random inputs against float64 with a per-element bound and no floor,
|y - y64| <= (D + 4) * 2^-24 * conv64(|x|, |w|) (+ half a bf16 ulp of |y64| for bf16 outputs), where D bounds the
number of fp32 roundings on the way to one output (the K terms of one output plus its splits / slices). The reference
takes bf16 operands rounded to nearest even, so a weight pack that truncates is off by ~2^-9 per term, far above it.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_exact_worker import (BF, F32, GARB, U32, Canvas, assert_exact, bf16_store, bwgrad_ws_floats,
                               check_conv_bf16, check_conv_f32, conv_workspace, ints, lib, out_size, pack_bf16,
                               pack_f32, part, premise, rb, ref_conv, ref_convT, stream, term_bound, wgrad_ws_f32)
from conv_exact_worker import bounded as _bounded
from conv_exact_worker import half_ulp_bf16 as _half_ulp_bf16
from route_ledger import Routes, case_id

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _tab(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _ints_c(vals):
    return (ctypes.c_int * len(vals))(*vals)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 Conv2d: forward, backward-data, weight gradient
# ---------------------------------------------------------------------------------------------------------------------

F32_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad, dil, bias       H*W % 4, channels, edges
    (2, 1, 12, 12, 1, 3, 1, 1, 1, True),       # 0; one channel in and out
    (2, 3, 13, 13, 3, 3, 1, 1, 1, True),       # 1 (odd plane); head-like 3 -> 3
    (1, 7, 5, 6, 31, 3, 1, 1, 1, False),       # 2; Cin 8k-1, Cout below 32, plane smaller than a tile
    (2, 9, 7, 5, 33, 3, 1, 1, 1, True),        # 3 (odd W); Cin 8k+1, Cout just past NT 32
    (1, 17, 2, 9, 63, 3, 1, 1, 1, False),      # 2; H below the 3x3 halo
    (2, 15, 9, 2, 65, 3, 1, 1, 1, True),       # 2; W below the halo, Cout just past NT 64
    (2, 24, 11, 11, 64, 3, 2, 1, 1, False),    # 1; stride 2 from an odd plane
    (1, 31, 25, 25, 127, 3, 2, 1, 1, True),    # 1; stride 2, Cout 127
    (2, 16, 14, 14, 129, 3, 1, 2, 2, False),   # 0; dilation 2 (pad = dil), Cout 129
    (1, 33, 13, 15, 136, 3, 1, 3, 3, True),    # 3; dilation 3, Cout 136 (pad boundary)
    (2, 64, 7, 7, 256, 3, 1, 1, 1, True),      # 1; deep K on a tiny plane: K split
    (2, 40, 10, 10, 32, 1, 1, 0, 1, True),     # 0; 1x1 on the tap kernel (too few blocks for the GEMM)
    (3, 130, 9, 11, 128, 1, 1, 0, 1, False),   # 3; 1x1, ragged K chunk
    (8, 128, 25, 25, 128, 3, 1, 1, 1, False),  # production: up_cu / tower_c
    (8, 640, 25, 25, 128, 3, 1, 1, 1, False),  # production: tower_c block 0
    (8, 576, 50, 50, 128, 3, 1, 1, 1, False),  # production: tower_b block 0
    # the strided gathers of the training step and the predict forward (routes no case above takes: route ledger)
    (8, 128, 100, 100, 128, 3, 2, 1, 1, False),
    (8, 128, 25, 25, 256, 3, 2, 1, 1, False),
    (4, 128, 28, 28, 256, 3, 2, 1, 1, False),
    (4, 64, 55, 55, 128, 3, 2, 1, 1, False),
]


# Cases the route ledger asked for: the smallest shapes a probe of the dispatcher found for every instantiation of
# cn_conv_igemm_vec_kernel<WAVES_N, TN, TM, NV, RP> and cn_conv_igemm_kernel<WAVES_N, TN, NI_T> no case above reaches.
# NV follows the staged image (wide planes, dilation 5: 1024 / 2048 / 4096 floats), RP the row padding (W % 4 == 0: 1,
# W % 2 == 0: 2, odd W or |dx| > 4: 0, odd planes: 3), NI_T the halo plane of the dword kernel (H * W % 4 >= 2), the
# tile config of 128 couts the block count (hence batch 32).
F32_LEDGER_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad, dil, bias
    (1, 8, 100, 100, 40, 3, 2, 1, 1, False),  # production <1, 2, 6> G1 cls1 is2 os1 taps9 whole il0 ws
    (1, 8, 12, 12, 128, 3, 1, 5, 5, False),  # _vec<2, 2, 2, 1, 0>
    (1, 8, 12, 12, 40, 3, 1, 5, 5, False),  # _vec<1, 2, 2, 1, 0>
    (1, 8, 12, 12, 8, 3, 1, 5, 5, False),  # _vec<1, 1, 2, 1, 0>
    (1, 8, 13, 13, 128, 3, 2, 1, 1, False),  # production _vec<2, 2, 2, 1, 3> G1 cls1 is2 os1 taps9 whole il0 ws
    (1, 8, 28, 28, 128, 3, 1, 5, 5, False),  # _vec<4, 1, 3, 1, 0>
    (1, 8, 3, 101, 8, 3, 1, 5, 5, False),  # <1, 1, 6>
    (1, 8, 3, 301, 128, 3, 1, 2, 2, False),  # <2, 2, 12>
    (1, 8, 4, 256, 128, 3, 1, 1, 1, False),  # _vec<4, 1, 3, 2, 1>
    (1, 8, 4, 512, 40, 3, 1, 1, 1, False),  # _vec<1, 2, 2, 4, 1>
    (1, 8, 4, 512, 8, 3, 1, 1, 1, False),  # _vec<1, 1, 2, 4, 1>
    (1, 8, 5, 205, 128, 3, 1, 2, 2, False),  # _vec<4, 1, 3, 2, 3>
    (1, 8, 5, 205, 40, 3, 1, 1, 1, False),  # _vec<1, 2, 2, 2, 3>
    (1, 8, 5, 205, 40, 3, 1, 5, 5, False),  # _vec<1, 2, 2, 4, 3>
    (1, 8, 5, 205, 8, 3, 1, 1, 1, False),  # _vec<1, 1, 2, 2, 3>
    (1, 8, 5, 205, 8, 3, 1, 5, 5, False),  # _vec<1, 1, 2, 4, 3>
    (1, 8, 6, 101, 40, 3, 1, 5, 5, False),  # <1, 2, 12>
    (1, 8, 6, 101, 8, 3, 1, 5, 5, False),  # <1, 1, 12>
    (1, 8, 6, 510, 40, 3, 1, 1, 1, False),  # _vec<1, 2, 2, 4, 2>
    (1, 8, 6, 510, 8, 3, 1, 1, 1, False),  # _vec<1, 1, 2, 4, 2>
    (1, 8, 8, 128, 128, 3, 1, 5, 5, False),  # _vec<4, 1, 3, 2, 0>
    (1, 8, 8, 128, 40, 3, 1, 2, 2, False),  # _vec<1, 2, 2, 2, 1>
    (1, 8, 8, 128, 40, 3, 1, 5, 5, False),  # _vec<1, 2, 2, 2, 0>
    (1, 8, 8, 128, 8, 3, 1, 2, 2, False),  # _vec<1, 1, 2, 2, 1>
    (1, 8, 8, 128, 8, 3, 1, 5, 5, False),  # _vec<1, 1, 2, 2, 0>
    (1, 8, 8, 130, 40, 3, 1, 2, 2, False),  # _vec<1, 2, 2, 2, 2>
    (1, 8, 8, 255, 40, 3, 1, 5, 5, False),  # _vec<1, 2, 2, 4, 0>
    (1, 8, 8, 255, 8, 3, 1, 5, 5, False),  # _vec<1, 1, 2, 4, 0>
    (1, 8, 8, 258, 128, 3, 1, 1, 1, False),  # _vec<4, 1, 3, 2, 2>
    (32, 8, 5, 205, 128, 3, 1, 2, 2, False),  # _vec<4, 1, 5, 2, 3>
    (32, 8, 8, 129, 128, 3, 1, 1, 1, False),  # _vec<4, 1, 5, 1, 0>
    (32, 8, 8, 129, 128, 3, 1, 5, 5, False),  # _vec<4, 1, 5, 2, 0>
    (32, 8, 8, 130, 128, 3, 1, 2, 2, False),  # _vec<4, 1, 5, 2, 2>
    (8, 72, 8, 258, 128, 3, 1, 1, 1, False),  # _vec<2, 2, 2, 2, 2>
]


@pytest.mark.parametrize("case", F32_LEDGER_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_conv2d_f32_exact_ledger_cases(case, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path, "ws")
    with conv_workspace("ws"):
        check_conv_f32(case, seed=20, parts=("y", "dx"), routes=routes)
    routes.verify()


@pytest.mark.parametrize("case", F32_CASES)
def test_conv2d_f32_exact(case, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path, "ws")
    with conv_workspace("ws"):
        check_conv_f32(case, seed=1, routes=routes)
    routes.verify()


@pytest.mark.parametrize("case", [F32_CASES[1], F32_CASES[6], F32_CASES[10], F32_CASES[13]])
def test_conv2d_f32_exact_atomic_split(case, request, tmp_path):
    """No workspace registered: K splits combine with float atomics on the output."""
    _dev()
    routes = Routes(case_id(request), tmp_path, "atomics")
    with conv_workspace("none"):
        check_conv_f32(case, seed=2, parts=("y", "dx"), routes=routes)
        check_conv_f32(case, seed=3, accumulate=True, parts=("y", "dx"), routes=routes, tag="+= ")
    routes.verify()


@pytest.mark.parametrize("case,xpad,ypad", [(F32_CASES[3], 4, 8), (F32_CASES[7], 3, 5), (F32_CASES[10], 8, 1),
                                            ((2, 72, 12, 12, 40, 3, 1, 1, 1, True), 3, 0)])
def test_conv2d_f32_exact_accumulate_padded_strides(case, xpad, ypad, request, tmp_path):
    """accumulate into integer-prefilled outputs, batch strides larger than C*H*W (unaligned ones included)."""
    _dev()
    routes = Routes(case_id(request), tmp_path, "ws", f"xpad{xpad} ypad{ypad}")
    with conv_workspace("ws"):
        check_conv_f32(case, seed=4, accumulate=True, xpad=xpad, ypad=ypad, routes=routes, tag="+= ")
    routes.verify()


@pytest.mark.parametrize("case", [(4, 48, 100, 100, 129, 1, 1, 0, 1, True),   # the dedicated 1x1 GEMM, ragged Cout
                                  (8, 480, 100, 100, 128, 1, 1, 0, 1, True),   # tower_a skip
                                  (8, 130, 50, 50, 200, 1, 1, 0, 1, False)])
def test_conv2d_f32_exact_1x1_gemm(case, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path, "ws")
    with conv_workspace("ws"):
        check_conv_f32(case, seed=5, parts=("y", "dx"), routes=routes)
        check_conv_f32(case, seed=6, accumulate=True, parts=("y",), routes=routes, tag="+= ")
    routes.verify()


@pytest.mark.parametrize("case", [(8, 480, 100, 100, 128, 3, 1, 1, 1, False)])
def test_conv2d_f32_exact_production_100(case, request, tmp_path):
    """tower_a block 0: more blocks than one round over the CUs."""
    _dev()
    routes = Routes(case_id(request), tmp_path, "ws")
    with conv_workspace("ws"):
        check_conv_f32(case, seed=7, routes=routes)
    routes.verify()


@pytest.mark.parametrize("case", [
    (2, 16, 12, 12, 24, 3, 1, 1, 1, False),    # H*W % 4 == 0, even W: the 16-byte DMA path directly
    (2, 16, 13, 13, 24, 3, 1, 1, 1, False),    # odd plane: aligned copies in the workspace / dword fallback
    (2, 12, 10, 7, 20, 3, 1, 2, 2, False),     # odd W, dilated
    (3, 24, 100, 100, 32, 3, 1, 1, 1, False),  # the largest sum: 3 x 100 x 100 pixels
    (2, 40, 25, 25, 128, 1, 1, 0, 1, False),   # 1x1, odd plane
    (2, 32, 26, 26, 48, 3, 2, 1, 1, False),    # stride 2
    (2, 32, 28, 28, 48, 1, 2, 0, 1, False),    # 1x1, stride 2: cn_wgrad_vec_kernel<1, 2> (route ledger)
    # the staging branches of cn_wgrad_vec_kernel<1, 1>. PR = 10 on 14 rows: the second chunk of an image runs past the
    # plane, both operands zero-fill per 16-byte piece; a ragged second cout tile and Cin < 32: idle DMA lanes; two k-parts
    (2, 24, 14, 12, 40, 1, 1, 0, 1, False),
    # one cout tile, four k-part waves on two pixel pairs per row: two waves own no pair and add zeros in the LDS reduction
    (1, 8, 4, 4, 8, 1, 1, 0, 1, False),
])
@pytest.mark.parametrize("ws", ["full", "none"])
def test_conv2d_f32_weight_gradient_routes(case, ws, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path)
    check_conv_f32(case, seed=8, wgrad_ws=ws, parts=("dw",), routes=routes)
    routes.verify()


def test_conv2d_f32_weight_gradient_padded_batch_stride(request, tmp_path):
    """A batch stride that breaks 16-byte alignment forces the aligned copies (with ws) or the dword kernel."""
    _dev()
    routes = Routes(case_id(request), tmp_path, "xpad1 ypad3")
    for ws in ("full", "none"):
        check_conv_f32((2, 16, 12, 12, 24, 3, 1, 1, 1, False), seed=9, xpad=1, ypad=3, wgrad_ws=ws, parts=("dw",),
                       routes=routes, tag=f"ws {ws}: ")
    routes.verify()


def test_conv2d_f32_exact_largest_weight_gradient(request, tmp_path):
    """8 x 100 x 100 pixels per weight: the premise holds with margin (8e4 x 12 < 2^24)."""
    _dev()
    routes = Routes(case_id(request), tmp_path)
    check_conv_f32((8, 24, 100, 100, 32, 3, 1, 1, 1, False), seed=10, parts=("dw",), routes=routes)
    routes.verify()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 ConvTranspose2d, the stride-4 taps route, the time convolution
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [
    # B, Cin, H, W, Cout, stride, out_pad, bias, accumulate
    (2, 16, 13, 13, 16, 2, 0, True, False),
    (2, 32, 25, 25, 32, 2, 1, True, False),    # the output_padding grid the engine uses (49 -> 50)
    (1, 24, 14, 14, 24, 2, 0, False, True),
    (2, 40, 50, 50, 40, 2, 1, True, False),    # 99 -> 100
    (1, 9, 7, 5, 33, 2, 1, True, True),
    (2, 16, 7, 7, 16, 4, 0, True, False),      # stride 4 as a plain transposed conv (some outputs: bias only)
    (1, 128, 25, 25, 128, 2, 1, True, False),
    # the parity-class scatters of the training step and the predict forward (route ledger)
    (8, 128, 25, 25, 128, 2, 1, True, False),
    (8, 128, 50, 50, 128, 2, 1, True, False),
    (8, 128, 25, 25, 64, 2, 1, True, False),
    (4, 128, 14, 14, 128, 2, 1, True, False),
    (4, 128, 28, 28, 128, 2, 0, True, False),
    (4, 64, 55, 55, 64, 2, 1, True, False),
    (4, 128, 55, 55, 128, 2, 1, True, False),
    # the remaining production scatters, at the smallest batch that selects their tile (route ledger)
    (4, 8, 50, 50, 128, 2, 1, True, False),  # production _vec<4, 1, 3, 1, 2> G1 cls4 is1 os2 taps4 whole il1 ws
    (4, 8, 28, 28, 128, 2, 0, True, False),  # production _vec<2, 2, 2, 1, 1> cls4 os2 taps4 whole il0: unequal class tiles
    (36, 8, 28, 28, 128, 2, 0, True, False),  # the same at the block count of the 36-window predict forward
])
def test_conv_transpose2d_f32_exact(case, request, tmp_path):
    B, Cin, H, W, Cout, s, op, bias, acc = case
    dev = _dev()
    routes = Routes(case_id(request), tmp_path)
    facts = ("ws", "acc") if acc else ("ws",)  # of the forward / data-gradient parts; a weight gradient knows neither
    k, p, T = 3, 1, 9
    Ho, Wo = (H - 1) * s - 2 * p + k + op, (W - 1) * s - 2 * p + k + op
    x = ints((B, Cin, H, W), -4, 4, 11)
    w = ints((Cin, Cout, k, k), -3, 3, 12)
    b = ints((Cout,), -8, 8, 13) if bias else None
    dy = ints((B, Cout, Ho, Wo), -3, 3, 14)
    y0 = ints((B, Cout, Ho, Wo), -8, 8, 15) if acc else torch.zeros(B, Cout, Ho, Wo, dtype=torch.float64)
    x0 = ints((B, Cin, H, W), -8, 8, 16) if acc else torch.zeros(B, Cin, H, W, dtype=torch.float64)
    w0 = ints(w.shape, -8, 8, 17)
    premise("convT", term_bound(x, w, Cin * T), 16)
    premise("convT dx", term_bound(dy, w, Cout * T), 8)
    premise("convT dw", term_bound(x, dy, B * H * W), 8)
    y64, dx64, dw64 = ref_convT(x, w, b, dy, s, p, op)
    L, st = lib(), stream()
    wd = w.float().to(dev)
    bd = b.float().to(dev) if bias else None
    with conv_workspace("ws"):
        xc = Canvas(x.shape, F32, dev, fill=GARB, data=x)
        yc = Canvas(y64.shape, F32, dev, data=y0 if acc else None)
        wp, wpt = pack_f32(wd, T, Cin, Cout, Cout * T, T, 1), pack_f32(wd, T, Cout, Cin, T, Cout * T, 1)
        with routes.part("transposed y", *facts):
            L.call("cn_conv_transpose2d_fwd_f32", xc.ptr, xc.pitch, wp.data_ptr(), None if bd is None else bd.data_ptr(),
                   yc.ptr, yc.pitch, B, Cin, H, W, Cout, k, k, s, p, op, int(acc), st)
        dyc = Canvas(dy.shape, F32, dev, fill=GARB, data=dy)
        dxc = Canvas(x.shape, F32, dev, data=x0 if acc else None)
        with routes.part("transposed dx", *facts):
            L.call("cn_conv_transpose2d_bwd_data_f32", dyc.ptr, dyc.pitch, wpt.data_ptr(), dxc.ptr, dxc.pitch, B, Cin, H,
                   W, Cout, k, k, s, p, op, int(acc), st)
        for ws in ("full", "none"):
            dwc = Canvas(w.shape, F32, dev, data=w0)
            wsp, wsn, _keep = wgrad_ws_f32(B, Cin, H, W, Cout, Ho, Wo, ws)
            with routes.part(f"transposed dw ws {ws}"):
                L.call("cn_conv_transpose2d_bwd_weight_f32", xc.ptr, xc.pitch, dyc.ptr, dyc.pitch, dwc.ptr, B, Cin, H, W,
                       Cout, k, k, s, p, op, wsp, wsn, st)
            torch.cuda.synchronize()
            assert_exact(dwc.t, dw64 + w0, f"dw ws={ws}")
            dwc.assert_canary("dw")
    assert_exact(yc.t, y64 + y0, "y")
    yc.assert_canary("y")
    assert_exact(dxc.t, dx64 + x0, "dx")
    dxc.assert_canary("dx")
    routes.verify()

# Wide planes: the 2048- and 4096-float staging images (NV 2 | 4) of the 128-cout tiles under every row-padding variant
# and tile config. With 128 couts the 4096-float image leaves LDS room for at most 7 taps, so only the 4-tap parity
# classes of a strided scatter reach it (a 3x3 gather that needs it answers CN_ERR_LDS, as do the data and weight
# gradients of these shapes): the forward alone, on the output_padding 1 grid (H -> 2 H). Shapes from a probe of the
# dispatcher; batch 32 / 64 is what selects the 160-pixel tile.
CONVT_WIDE_F32 = [
    # B, Cin, H, W, Cout
    (1, 8, 4, 511, 128),  # _vec<2, 2, 2, 2, 0>
    (1, 8, 4, 256, 128),  # _vec<2, 2, 2, 2, 1>
    (1, 8, 5, 409, 128),  # _vec<2, 2, 2, 2, 3>
    (1, 8, 4, 1022, 128),  # _vec<2, 2, 2, 4, 0>
    (1, 8, 4, 512, 128),  # _vec<2, 2, 2, 4, 1>
    (1, 8, 4, 510, 128),  # _vec<2, 2, 2, 4, 2>
    (1, 8, 3, 683, 128),  # _vec<2, 2, 2, 4, 3>
    (1, 72, 4, 1022, 128),  # _vec<4, 1, 3, 4, 0>
    (2, 72, 4, 512, 128),  # _vec<4, 1, 3, 4, 1>
    (2, 72, 4, 510, 128),  # _vec<4, 1, 3, 4, 2>
    (4, 8, 3, 683, 128),  # _vec<4, 1, 3, 4, 3>
    (64, 8, 8, 256, 72),  # _vec<4, 1, 5, 2, 1>
    (32, 8, 4, 1022, 72),  # _vec<4, 1, 5, 4, 0>
    (64, 8, 4, 512, 72),  # _vec<4, 1, 5, 4, 1>
    (64, 8, 4, 510, 72),  # _vec<4, 1, 5, 4, 2>
    (8, 8, 3, 683, 128),  # _vec<4, 1, 5, 4, 3>
    (16, 8, 5, 205, 128),  # production _vec<4, 1, 5, 1, 3> G1 cls4 is1 os2 taps4 whole il1 ws
]


@pytest.mark.parametrize("B,Cin,H,W,Cout", CONVT_WIDE_F32)
def test_conv_transpose2d_f32_forward_wide_exact(B, Cin, H, W, Cout, request, tmp_path):
    dev = _dev()
    x = ints((B, Cin, H, W), -4, 4, 18)
    w = ints((Cin, Cout, 3, 3), -3, 3, 19)
    b = ints((Cout,), -8, 8, 20)
    premise("convT wide", term_bound(x, w, Cin * 9), 8)
    y64 = F.conv_transpose2d(x, w, b, 2, 1, output_padding=1)
    L, st = lib(), stream()
    wd, bd = w.float().to(dev), b.float().to(dev)
    routes = Routes(case_id(request), tmp_path)
    with conv_workspace("ws"):
        xc = Canvas(x.shape, F32, dev, fill=GARB, data=x)
        yc = Canvas(y64.shape, F32, dev)
        wp = pack_f32(wd, 9, Cin, Cout, Cout * 9, 9, 1)
        with routes.part("transposed y", "ws"):
            L.call("cn_conv_transpose2d_fwd_f32", xc.ptr, xc.pitch, wp.data_ptr(), bd.data_ptr(), yc.ptr, yc.pitch, B, Cin,
                   H, W, Cout, 3, 3, 2, 1, 1, 0, st)
        torch.cuda.synchronize()
    assert_exact(yc.t, y64, "y")
    yc.assert_canary("y")
    routes.verify()


def _engine_run(mod, fn, inputs, dy, routes=None):
    from cultionet_amd import engine as E

    dev = _dev()
    mod = mod.to(dev)
    store = E.ParamStore(mod)
    store.zero_grad()
    with E.using_store(store), E.recording(True) as tape:
        xs = [E.Var(t.to(dev).float().contiguous(), True) for t in inputs]
        with part(routes, "engine forward"):
            y = fn(*xs)
        y.grad = dy.to(dev).float().contiguous()
        with part(routes, "engine backward"):
            tape.backward()
    torch.cuda.synchronize()
    return y.t.cpu(), [x.grad.cpu() for x in xs], {n: store.grad_of(p).cpu() for n, p in mod.named_parameters()}


@pytest.mark.parametrize("B,C,H,W", [(2, 16, 7, 7), (1, 9, 25, 25), (2, 3, 5, 6)])
def test_convt_taps_route_exact(B, C, H, W, request, tmp_path):
    """final_c's ConvTranspose2d(k 3, stride 4, padding 1) at its natural size: the 1x1 GEMM into taps-as-channels
    and cn_convt_taps_fwd_f32 / cn_convt_taps_bwd_f32 (no resize), through the engine."""
    from cultionet_amd import engine as E

    mod = nn.ConvTranspose2d(C, C, 3, stride=4, padding=1)
    with torch.no_grad():
        mod.weight.copy_(ints(mod.weight.shape, -3, 3, 21).float())
        mod.bias.copy_(ints((C,), -8, 8, 22).float())
    x = ints((B, C, H, W), -4, 4, 23)
    Ho, Wo = (H - 1) * 4 + 1, (W - 1) * 4 + 1
    dy = ints((B, C, Ho, Wo), -3, 3, 24)
    y64, dx64, dw64 = ref_convT(x, mod.weight.detach(), mod.bias.detach(), dy, 4, 1)
    premise("taps", term_bound(x, mod.weight.detach(), C), 8)
    premise("taps dw", term_bound(x, dy, B * H * W), 0)
    routes = Routes(case_id(request), tmp_path)
    y, (dx,), pg = _engine_run(mod, lambda v: E.conv_transpose2d(v, mod, 4, 1), [x], dy, routes)
    assert_exact(y, y64, "y")
    assert_exact(dx, dx64, "dx")
    assert_exact(pg["weight"], dw64, "dw")
    assert_exact(pg["bias"], dy.sum(dim=(0, 2, 3)), "db")
    routes.verify()


@pytest.mark.parametrize("B,C,H,W,size", [(1, 16, 25, 25, 100), (2, 8, 7, 7, 30)])
def test_convt_taps_route_resized_bound(B, C, H, W, size):
    """The same route resized in its pointwise pass (bilinear, align_corners): random inputs, per-element bound on the
    output. The conv part costs C + 1 roundings; the resize 4 products and 3 adds of fp32 weights, and each weight is
    off by up to ~2 * size * u absolute (its source coordinate is o * (n - 1) / (size - 1) in fp32), which multiplies
    the largest |z| of the 3 x 3 neighbourhood rather than a weighted one. (The adjoint at natural size is exact-tested
    above; the resized one stays with test_kernels_gpu.py's relative bounds.)"""
    from cultionet_amd import engine as E

    torch.manual_seed(25)
    mod = nn.ConvTranspose2d(C, C, 3, stride=4, padding=1)
    g = torch.Generator().manual_seed(26)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64).float().double()
    dy = torch.randn(B, C, size, size, generator=g, dtype=torch.float64).float().double()
    w64, b64 = mod.weight.detach().double(), mod.bias.detach().double()
    up = lambda z: F.interpolate(z, size=(size, size), mode="bilinear", align_corners=True)
    y64 = up(F.conv_transpose2d(x, w64, b64, 4, 1))
    zabs = F.conv_transpose2d(x.abs(), w64.abs(), b64.abs(), 4, 1)
    bound = (C + 12) * U32 * up(zabs) + 2 * size * U32 * up(F.max_pool2d(zabs, 3, 1, 1))
    y, _, _ = _engine_run(mod, lambda v: E.conv_transpose2d(v, mod, 4, 1, size=(size, size)), [x], dy)
    _bounded(y, y64, bound, "taps resized y")


@pytest.mark.parametrize("k", [3, 5])
def test_time_conv_exact(k, request, tmp_path):
    """nn.Conv3d(kernel (k,1,1)) of PreTimeReduction: cn_pack_timeconv_f32 (both orientations), the banded 1x1
    contraction and cn_fold_timeconv_grad_f32."""
    from cultionet_amd import engine as E

    B, C, Tn, H, W, Cout = 2, 3, 12, 10, 9, 5
    conv = nn.Conv3d(C, Cout, (k, 1, 1), bias=False)
    with torch.no_grad():
        conv.weight.copy_(ints(conv.weight.shape, -3, 3, 31).float())
    x = ints((B, C, Tn, H, W), -4, 4, 32)
    xr = x.clone().requires_grad_(True)
    wr = conv.weight.detach().double().requires_grad_(True)
    y64 = F.conv3d(xr, wr)
    dy = ints(y64.shape, -3, 3, 33)
    dx64, dw64 = torch.autograd.grad(y64, (xr, wr), dy)
    premise("time conv dw", term_bound(x, dy, B * H * W * (Tn - k + 1)), 0)
    routes = Routes(case_id(request), tmp_path)
    y, (dx,), pg = _engine_run(conv, lambda v: E.time_conv(v, conv, Tn), [x.reshape(B, C * Tn, H, W)],
                               dy.reshape(B, -1, H, W), routes)
    assert_exact(y.reshape(y64.shape), y64.detach(), "y")
    assert_exact(dx.reshape(x.shape), dx64, "dx")
    assert_exact(pg["weight"], dw64, "dw")
    routes.verify()


# ---------------------------------------------------------------------------------------------------------------------
# fp32 grouped launches
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G,B,Cin,H,W,Cout,dils,shared_in,ws", [
    (1, 2, 16, 13, 13, 24, (1,), False, "ws"),
    (2, 2, 24, 14, 14, 32, (1, 2), True, "ws"),
    (3, 1, 9, 11, 7, 33, (1, 2, 3), False, "ws"),
    (4, 2, 32, 25, 25, 64, (1, 2, 3, 4), True, "ws"),
    (2, 8, 128, 25, 25, 128, (1, 2), True, "none"),
    (3, 2, 64, 7, 7, 128, (1, 1, 2), False, "none"),
    # two convolutions of one input per launch, as the training step and the predict forward group them (route ledger)
    (2, 8, 32, 100, 100, 32, (1, 1), True, "ws"),
    (2, 8, 64, 50, 50, 64, (1, 1), True, "ws"),
    (2, 8, 128, 50, 50, 128, (1, 1), True, "ws"),
    (2, 8, 128, 25, 25, 128, (1, 1), True, "ws"),
    (2, 4, 64, 55, 55, 64, (1, 1), True, "ws"),
    (2, 4, 128, 28, 28, 128, (1, 1), True, "ws"),
    (2, 4, 128, 55, 55, 128, (1, 1), True, "ws"),
    # the unsplit two-group launches (few K chunks, or many blocks) of the predict forward and the eval forward
    (2, 1, 8, 13, 13, 40, (1, 1), True, "ws"),  # production _vec<1, 2, 2, 1, 3> G>1 cls2 is1 os1 taps9 whole il0 ws
    (2, 16, 8, 28, 28, 128, (1, 1), True, "ws"),  # production _vec<2, 2, 2, 1, 1> G>1 cls2 is1 os1 taps9 whole il0 ws
    (2, 1, 8, 13, 13, 128, (1, 1), True, "ws"),  # production _vec<2, 2, 2, 1, 3> G>1 cls2 is1 os1 taps9 whole il0 ws
    (2, 1, 8, 14, 14, 128, (1, 1), True, "ws"),  # production _vec<4, 1, 3, 1, 2> G>1 cls2 is1 os1 taps9 whole il0 ws
    (2, 4, 8, 100, 100, 128, (1, 1), True, "ws"),  # production _vec<4, 1, 5, 1, 1> G>1 cls2 is1 os1 taps9 whole il0 ws
    (2, 16, 8, 50, 50, 128, (1, 1), True, "ws"),  # production _vec<4, 1, 5, 1, 2> G>1 cls2 is1 os1 taps9 whole il0 ws
])
def test_grouped_f32_exact(G, B, Cin, H, W, Cout, dils, shared_in, ws, request, tmp_path):
    """cn_conv2d_{fwd,bwd_data}_grouped_f32 with distinct and summed outputs (pad = dil per group), and
    cn_conv2d_bwd_weight_grouped_f32 (one pad / dilation for all groups)."""
    dev = _dev()
    L, st = lib(), stream()
    k, T = 3, 9
    xs = [ints((B, Cin, H, W), -4, 4, 40 + (0 if shared_in else i)) for i in range(G)]
    ws_ = [ints((Cout, Cin, k, k), -3, 3, 50 + i) for i in range(G)]
    bs = [ints((Cout,), -8, 8, 60 + i) for i in range(G)]
    dys = [ints((B, Cout, H, W), -3, 3, 70 + i) for i in range(G)]
    premise("grouped", G * term_bound(xs[0], ws_[0], Cin * T), G * 8)
    premise("grouped dx", G * term_bound(dys[0], ws_[0], Cout * T), 0)
    refs = [ref_conv(xs[i], ws_[i], bs[i], dys[i], 1, dils[i], dils[i]) for i in range(G)]
    xcs = [Canvas(xs[0].shape, F32, dev, fill=GARB, data=xs[i]) for i in range(1 if shared_in else G)]
    xptr = [xcs[0 if shared_in else i].ptr for i in range(G)]
    wds = [w.float().to(dev) for w in ws_]
    bds = [b.float().to(dev) for b in bs]
    wps = [pack_f32(wd, T, Cin, Cout, T, Cin * T, 1) for wd in wds]
    wpts = [pack_f32(wd, T, Cout, Cin, Cin * T, T, 1) for wd in wds]
    pads = _ints_c(list(dils))
    routes = Routes(case_id(request), tmp_path)
    wsf = "ws" if ws == "ws" else "atomics"
    with conv_workspace(ws):
        ycs = [Canvas((B, Cout, H, W), F32, dev) for _ in range(G)]
        with routes.part("grouped y", wsf):
            L.call("cn_conv2d_fwd_grouped_f32", G, _tab(xptr), xcs[0].pitch, _tab([w.data_ptr() for w in wps]),
                   _tab([b.data_ptr() for b in bds]), _tab([y.ptr for y in ycs]), ycs[0].pitch, B, Cin, H, W, Cout, k, k,
                   1, pads, pads, 0, st)
        ysum0 = ints((B, Cout, H, W), -8, 8, 80)
        ysum = Canvas((B, Cout, H, W), F32, dev, data=ysum0)
        with routes.part("grouped summed y", wsf, "acc"):
            L.call("cn_conv2d_fwd_grouped_f32", G, _tab(xptr), xcs[0].pitch, _tab([w.data_ptr() for w in wps]),
                   _tab([b.data_ptr() for b in bds]), _tab([ysum.ptr] * G), ysum.pitch, B, Cin, H, W, Cout, k, k, 1, pads,
                   pads, 1, st)
        dycs = [Canvas((B, Cout, H, W), F32, dev, fill=GARB, data=d) for d in dys]
        dxcs = [Canvas((B, Cin, H, W), F32, dev) for _ in range(G)]
        k3 = _ints_c([3] * G)
        with routes.part("grouped dx", wsf):
            L.call("cn_conv2d_bwd_data_grouped_f32", G, _tab([d.ptr for d in dycs]), dycs[0].pitch,
                   _tab([w.data_ptr() for w in wpts]), _tab([d.ptr for d in dxcs]), dxcs[0].pitch, B, Cin, H, W, Cout, k3,
                   k3, 1, pads, pads, 0, st)
        dxsum = Canvas((B, Cin, H, W), F32, dev)
        with routes.part("grouped summed dx", wsf):
            L.call("cn_conv2d_bwd_data_grouped_f32", G, _tab([d.ptr for d in dycs]), dycs[0].pitch,
                   _tab([w.data_ptr() for w in wpts]), _tab([dxsum.ptr] * G), dxsum.pitch, B, Cin, H, W, Cout, k3, k3, 1,
                   pads, pads, 0, st)
        torch.cuda.synchronize()
    for i in range(G):
        assert_exact(ycs[i].t, refs[i][0], f"y{i}")
        ycs[i].assert_canary(f"y{i}")
        assert_exact(dxcs[i].t, refs[i][1], f"dx{i}")
        dxcs[i].assert_canary(f"dx{i}")
    assert_exact(ysum.t, ysum0 + sum(r[0] for r in refs), "summed y (+=)")
    ysum.assert_canary("summed y")
    assert_exact(dxsum.t, sum(r[1] for r in refs), "summed dx")
    dxsum.assert_canary("summed dx")
    # weight gradient: one padding / dilation for every group
    d = dils[-1]
    w0s = [ints((Cout, Cin, k, k), -8, 8, 90 + i) for i in range(G)]
    dws = [Canvas((Cout, Cin, k, k), F32, dev, data=w0) for w0 in w0s]
    wsp, wsn, _keep = wgrad_ws_f32(B, Cin, H, W, Cout, H, W, "full")
    with routes.part("grouped dw", "ws full"):
        L.call("cn_conv2d_bwd_weight_grouped_f32", G, _tab(xptr), xcs[0].pitch, _tab([c.ptr for c in dycs]),
               dycs[0].pitch, _tab([c.ptr for c in dws]), B, Cin, H, W, Cout, k, k, 1, d, d, wsp, wsn, st)
    torch.cuda.synchronize()
    for i in range(G):
        premise("grouped dw", term_bound(xs[i], dys[i], B * H * W), 8)
        _, _, dw64 = ref_conv(xs[i], ws_[i], None, dys[i], 1, d, d)
        assert_exact(dws[i].t, dw64 + w0s[i], f"dw{i}")
        dws[i].assert_canary(f"dw{i}")
    routes.verify()


# ---------------------------------------------------------------------------------------------------------------------
# thin 3x3 head convolutions
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsets,cin,cp,grouped,bias,B,H,W,dil,wpack", [
    (3, 40, 3, False, True, 2, 13, 13, 1, True),    # (3,3,0): the wide layers, packed weights
    (3, 40, 3, False, False, 2, 12, 9, 2, False),   # (3,3,0) without wpack, dilated
    (3, 3, 1, True, True, 2, 25, 25, 1, False),     # (3,1,1)
    (3, 5, 1, True, False, 1, 9, 11, 3, False),     # (3,1,1) dilated 3
    (1, 3, 3, False, True, 2, 28, 28, 1, False),    # (1,3,0)
    (1, 7, 3, False, False, 1, 2, 5, 1, False),     # (1,3,0), H below the halo
    (1, 5, 1, False, True, 1, 9, 11, 1, False),     # (1,1,0)
    (1, 128, 1, False, False, 2, 100, 100, 2, False),
])
def test_thin_conv3x3_exact(nsets, cin, cp, grouped, bias, B, H, W, dil, wpack):
    dev = _dev()
    L, st = lib(), stream()
    xch = nsets * cin if grouped else cin
    x = ints((B, xch, H, W), -4, 4, 100)
    wts = [ints((cp, cin, 3, 3), -3, 3, 101 + i) for i in range(nsets)]
    bs = [ints((cp,), -8, 8, 110 + i) for i in range(nsets)] if bias else None
    dy = ints((B, nsets * cp, H, W), -3, 3, 120)
    premise("thin", term_bound(x, wts[0], cin * 9), 8)
    premise("thin dw", term_bound(x, dy, B * H * W), 8)
    premise("thin dx", nsets * term_bound(dy, wts[0], cp * 9), 8)
    ys, dxs, dws = [], torch.zeros(B, xch, H, W, dtype=torch.float64), []
    for i in range(nsets):
        xi = x[:, i * cin:(i + 1) * cin] if grouped else x
        y64, dx64, dw64 = ref_conv(xi, wts[i], None if bs is None else bs[i], dy[:, i * cp:(i + 1) * cp], 1, dil, dil)
        ys.append(y64)
        if grouped:
            dxs[:, i * cin:(i + 1) * cin] += dx64
        else:
            dxs += dx64
        dws.append(dw64)
    wds = [w.float().to(dev) for w in wts]
    bds = [b.float().to(dev) for b in bs] if bias else None
    wp = torch.empty(cin * 84, device=dev) if wpack else None
    xc = Canvas(x.shape, F32, dev, pitch=xch * H * W + 4, fill=GARB, data=x)
    yc = Canvas(dy.shape, F32, dev, pitch=nsets * cp * H * W + 3)
    L.call("cn_thin_conv3x3_fwd_f32", xc.ptr, xc.pitch, _tab([w.data_ptr() for w in wds]),
           _tab([b.data_ptr() for b in bds]) if bias else None, yc.ptr, yc.pitch, B, cin, H, W, nsets, cp, int(grouped),
           dil, None if wp is None else wp.data_ptr(), st)
    dyc = Canvas(dy.shape, F32, dev, fill=GARB, data=dy)
    dxc = Canvas(x.shape, F32, dev)
    L.call("cn_thin_conv3x3_bwd_data_f32", dyc.ptr, dyc.pitch, _tab([w.data_ptr() for w in wds]), dxc.ptr, dxc.pitch, B,
           cin, H, W, nsets, cp, int(grouped), dil, 0, None if wp is None else wp.data_ptr(), st)
    x0 = ints(x.shape, -8, 8, 130)
    dxa = Canvas(x.shape, F32, dev, data=x0)
    L.call("cn_thin_conv3x3_bwd_data_f32", dyc.ptr, dyc.pitch, _tab([w.data_ptr() for w in wds]), dxa.ptr, dxa.pitch, B,
           cin, H, W, nsets, cp, int(grouped), dil, 1, None if wp is None else wp.data_ptr(), st)
    w0s = [ints((cp, cin, 3, 3), -8, 8, 140 + i) for i in range(nsets)]
    dwcs = [Canvas((cp, cin, 3, 3), F32, dev, data=w0) for w0 in w0s]
    L.call("cn_thin_conv3x3_bwd_weight_f32", xc.ptr, xc.pitch, dyc.ptr, dyc.pitch, _tab([c.ptr for c in dwcs]), B, cin,
           H, W, nsets, cp, int(grouped), dil, st)
    torch.cuda.synchronize()
    assert_exact(yc.t, torch.cat(ys, 1), "y")
    yc.assert_canary("y")
    assert_exact(dxc.t, dxs, "dx")
    dxc.assert_canary("dx")
    assert_exact(dxa.t, dxs + x0, "dx (+=)")
    for i in range(nsets):
        assert_exact(dwcs[i].t, dws[i] + w0s[i], f"dw{i}")
        dwcs[i].assert_canary(f"dw{i}")


# ---------------------------------------------------------------------------------------------------------------------
# bf16 Conv2d, grouped, bnstats, fused, ConvTranspose2d
# ---------------------------------------------------------------------------------------------------------------------

BF16_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad, dil, bias
    (2, 8, 12, 12, 8, 3, 1, 1, 1, True),
    (2, 16, 13, 13, 31, 3, 1, 1, 1, True),     # ragged Cout: element-wise stores
    (1, 24, 5, 6, 33, 3, 1, 1, 1, False),      # plane smaller than a tile
    (2, 32, 7, 5, 64, 3, 1, 1, 1, True),       # odd W
    (1, 40, 2, 9, 65, 3, 1, 1, 1, False),      # H below the halo
    (2, 16, 11, 11, 127, 3, 2, 1, 1, True),    # stride 2 from an odd plane
    (2, 24, 14, 14, 129, 3, 1, 2, 2, False),   # dilation 2
    (1, 64, 13, 15, 136, 3, 1, 3, 3, True),    # dilation 3
    (2, 136, 9, 11, 256, 1, 1, 0, 1, True),    # 1x1
    (1, 8, 9, 9, 1, 3, 1, 1, 1, True),         # one output channel
    (2, 8, 10, 10, 3, 3, 1, 1, 1, False),
    (1, 16, 25, 25, 63, 3, 1, 1, 1, False),
    (2, 128, 25, 25, 128, 3, 1, 1, 1, False),
    (8, 640, 25, 25, 128, 3, 1, 1, 1, False),  # production
    (8, 576, 50, 50, 128, 3, 1, 1, 1, False),
    (8, 480, 100, 100, 128, 3, 1, 1, 1, False),
]


@pytest.mark.parametrize("case", BF16_CASES)
def test_conv2d_bf16_exact(case, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path)
    check_conv_bf16(case, seed=200, routes=routes)
    routes.verify()


@pytest.mark.parametrize("case", [BF16_CASES[0], BF16_CASES[1], BF16_CASES[5], BF16_CASES[8], BF16_CASES[12]])
def test_conv2d_bf16_exact_accumulate(case, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path, "acc")
    check_conv_bf16(case, seed=210, accumulate=True, xpad=16, ypad=8, parts=("y", "dx"), routes=routes)
    routes.verify()


@pytest.mark.parametrize("case", [(2, 64, 25, 25, 64, 3, 1, 1, 1, False), (3, 24, 100, 100, 32, 3, 1, 1, 1, False),
                                  (2, 128, 13, 13, 136, 3, 2, 1, 1, False), (2, 40, 50, 50, 24, 1, 1, 0, 1, False)])
@pytest.mark.parametrize("ws", ["full", "mid", "one"])
def test_conv2d_bf16_weight_gradient_workspaces(case, ws, request, tmp_path):
    """The split shrinks to fit the workspace: the full size, exactly one split's slice, and one in between."""
    _dev()
    routes = Routes(case_id(request), tmp_path)
    check_conv_bf16(case, seed=220, wgrad_ws=ws, parts=("dw",), routes=routes)
    routes.verify()


# Cases the route ledger (tests/contraction_routes.py) asked for: the smallest shapes that select an instantiation of
# cn_bconv_kernel<WN, NP, KSC, MPW> or cn_bwgrad_kernel<T, NQ, full> no other exact case reaches. WN follows the cout
# blocks (Cout <= 32: 1, <= 96: 2, else 4, halved with MPW 2 while a launch has <= 224 blocks -- hence the batches
# of 57 and 113 tiny planes for the full-tile WN 4 routes), KSC the input depth (Cin > 32, and > 64 for 1x1) and NP the
# halo image of one pixel tile; NQ and `full` follow the halo image and the tile of the weight gradient. Strides 3 and
# 4 are calls the model never makes; the C ABI accepts them and they are the only way to two 1x1 gradient kernels.
BF16_LEDGER_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad, dil, bias
    (2, 8, 5, 6, 8, 3, 1, 5, 5, False),        # <1,6,2,4>; gradient <9,16,false>
    (2, 40, 5, 6, 8, 1, 1, 0, 1, True),        # <1,6,4,4>
    (1, 8, 20, 25, 8, 1, 1, 0, 1, False),      # <1,10,2,4>
    (2, 40, 10, 10, 8, 1, 2, 0, 1, True),      # <1,10,4,4>
    (2, 72, 5, 6, 8, 1, 1, 0, 1, False),       # <1,10,8,4>
    (2, 8, 5, 6, 128, 1, 1, 0, 1, True),       # <2,4,2,2>
    (2, 8, 5, 6, 40, 1, 1, 0, 1, False),       # <2,4,2,4>
    (1, 8, 5, 6, 128, 3, 1, 5, 5, True),       # <2,6,2,2>
    (1, 8, 5, 6, 40, 3, 1, 5, 5, False),       # <2,6,2,4>
    (2, 40, 5, 6, 128, 1, 1, 0, 1, False),     # <2,6,4,2>
    (2, 40, 5, 6, 40, 1, 1, 0, 1, True),       # <2,6,4,4>
    (1, 8, 10, 50, 128, 1, 2, 0, 1, False),    # <2,10,2,2>; gradient <1,0,true>
    (1, 8, 10, 50, 40, 1, 2, 0, 1, True),      # <2,10,2,4>
    (1, 40, 10, 10, 128, 1, 2, 0, 1, True),    # <2,10,4,2>
    (1, 40, 10, 10, 40, 1, 2, 0, 1, False),    # <2,10,4,4>
    (2, 72, 5, 6, 128, 1, 1, 0, 1, True),      # <2,10,8,2>
    (2, 72, 5, 6, 40, 1, 1, 0, 1, False),      # <2,10,8,4>
    (113, 8, 5, 6, 256, 1, 1, 0, 1, False),    # <4,4,2,4>: 226 blocks
    (113, 8, 5, 6, 256, 3, 1, 5, 5, False),    # <4,6,2,4>
    (113, 40, 5, 6, 256, 1, 1, 0, 1, True),    # <4,6,4,4>, one tap
    (113, 40, 5, 6, 256, 3, 1, 1, 1, False),   # <4,6,4,4>, nine taps: the tower layers at batch 32
    (113, 8, 9, 49, 256, 1, 2, 0, 1, False),   # <4,10,2,4>
    (113, 40, 10, 10, 256, 1, 2, 0, 1, False), # <4,10,4,4>, one tap
    (57, 40, 5, 25, 512, 3, 1, 2, 2, False),   # <4,10,4,4>, nine taps, dilation 2: 228 blocks
    (113, 72, 5, 6, 256, 1, 1, 0, 1, False),   # <4,10,8,4>
    (2, 16, 1, 255, 24, 1, 2, 0, 1, False),    # gradient <1,8,true>: the 1 x 128 tile of a one-row plane
    (2, 16, 22, 22, 24, 1, 3, 0, 1, False),    # gradient <1,8,false>: stride 3
    (2, 16, 29, 29, 24, 1, 4, 0, 1, False),    # gradient <1,0,false>: stride 4
    (2, 16, 10, 25, 24, 3, 1, 4, 4, False),    # gradient <9,16,true>: dilation 4 on two 5 x 25 tiles
    (2, 16, 10, 25, 24, 3, 1, 5, 5, False),    # gradient <9,0,true>: dilation 5
    (2, 16, 15, 15, 24, 3, 2, 4, 4, False),    # gradient <9,0,false>: stride 2, dilation 4, one 8 x 8 tile
    # routes of the training step at batch 32 that no case above takes
    (2, 32, 26, 26, 64, 3, 2, 1, 1, False),    # strided gather, 64 couts
    (113, 40, 25, 25, 128, 3, 2, 1, 1, False), # strided gather, full-tile WN 4 (226 blocks)
    (57, 40, 17, 97, 128, 3, 4, 1, 1, False),  # stride 4 (final_c), full-tile WN 4 (228 blocks)
    (113, 9, 5, 25, 256, 3, 1, 1, 1, False),   # the first layer's 9 input channels: <4,4,2,4>
]


@pytest.mark.parametrize("case", BF16_LEDGER_CASES, ids=lambda c: "-".join(str(int(v)) for v in c))
def test_conv2d_bf16_exact_ledger_cases(case, request, tmp_path):
    _dev()
    routes = Routes(case_id(request), tmp_path)
    check_conv_bf16(case, seed=230, routes=routes)
    routes.verify()


def test_bf16_outputs_round_ties_to_even(request, tmp_path):
    """Outputs in [256, 512) have bf16 spacing 2: odd integers are ties. The exact tests reach them (checked here),
    so a store that truncates or rounds half up fails them."""
    case = (2, 64, 25, 25, 64, 3, 1, 1, 1, False)
    x = ints((2, 64, 25, 25), -4, 4, 200)
    w = ints((64, 64, 3, 3), -3, 3, 201)
    y64 = F.conv2d(x, w, padding=1)
    a = y64.abs()
    ties = (a >= 256) & (a < 512) & (torch.remainder(a, 2) == 1)
    assert int(ties.sum()) > 100, int(ties.sum())
    assert {float(v) % 4 for v in a[ties][:200]} == {1.0, 3.0}  # both directions of the tie
    _dev()
    routes = Routes(case_id(request), tmp_path)
    check_conv_bf16(case, seed=200, parts=("y",), routes=routes)
    routes.verify()


@pytest.mark.parametrize("G,B,Cin,H,W,Cout,dils,shared_in", [
    (1, 2, 16, 13, 13, 24, (1,), False),
    (2, 2, 32, 14, 14, 32, (1, 2), True),
    (3, 1, 24, 11, 9, 40, (1, 2, 3), False),
    (4, 2, 64, 25, 25, 64, (1, 2, 3, 4), True),
    # two convolutions of one input per launch as the training step groups them (route ledger): 64 and 128 couts, and
    # the full-tile WN 4 route (320 blocks)
    (2, 2, 64, 50, 50, 64, (1, 1), True),
    (2, 2, 40, 25, 25, 128, (1, 1), True),
    (2, 8, 40, 50, 50, 128, (1, 1), True),
])
def test_grouped_bf16_exact(G, B, Cin, H, W, Cout, dils, shared_in, request, tmp_path):
    """cn_conv2d_fwd_grouped_bf16 (+= too), cn_conv2d_fwd_grouped_bnstats_bf16 (outputs equal to the plain launch)
    and cn_conv2d_bwd_data_grouped_bf16, per group against float64."""
    dev = _dev()
    L, st = lib(), stream()
    k, T = 3, 9
    xs = [ints((B, Cin, H, W), -4, 4, 300 + (0 if shared_in else i)) for i in range(G)]
    wts = [ints((Cout, Cin, k, k), -3, 3, 310 + i) for i in range(G)]
    bs = [ints((Cout,), -8, 8, 320 + i) for i in range(G)]
    dys = [ints((B, Cout, H, W), -3, 3, 330 + i) for i in range(G)]
    premise("grouped bf16", term_bound(xs[0], wts[0], Cin * T), 16)
    premise("grouped bf16 dx", term_bound(dys[0], wts[0], Cout * T), 8)
    refs = [ref_conv(xs[i], wts[i], bs[i], dys[i], 1, dils[i], dils[i]) for i in range(G)]
    refs_nb = [F.conv2d(xs[i], wts[i], None, 1, dils[i], dils[i]) for i in range(G)]
    ld = lambda c: (c + 7) // 8 * 8 + 8
    xcs = [Canvas(xs[i].shape, BF, dev, pitch=ld(Cin), fill=GARB, data=xs[i]) for i in range(1 if shared_in else G)]
    xptr = [xcs[0 if shared_in else i].ptr for i in range(G)]
    wds = [w.float().to(dev) for w in wts]
    bds = [b.float().to(dev) for b in bs]
    wps = [pack_bf16(wd, T, Cin, Cout, T, Cin * T, 1) for wd in wds]
    wpts = [pack_bf16(wd, T, Cout, Cin, Cin * T, T, 1) for wd in wds]
    pads = _ints_c(list(dils))
    routes = Routes(case_id(request), tmp_path)
    ycs = [Canvas((B, Cout, H, W), BF, dev, pitch=ld(Cout)) for _ in range(G)]
    with routes.part("grouped y"):
        L.call("cn_conv2d_fwd_grouped_bf16", G, _tab(xptr), xcs[0].pitch, _tab([w.data_ptr() for w in wps]),
               _tab([b.data_ptr() for b in bds]), _tab([y.ptr for y in ycs]), ycs[0].pitch, B, Cin, H, W, Cout, k, k, 1,
               pads, pads, 0, None, st)
    y0s = [ints((B, Cout, H, W), -8, 8, 340 + i) for i in range(G)]
    yas = [Canvas((B, Cout, H, W), BF, dev, pitch=ld(Cout), data=y0) for y0 in y0s]
    with routes.part("grouped y +=", "acc"):
        L.call("cn_conv2d_fwd_grouped_bf16", G, _tab(xptr), xcs[0].pitch, _tab([w.data_ptr() for w in wps]),
               _tab([b.data_ptr() for b in bds]), _tab([y.ptr for y in yas]), yas[0].pitch, B, Cin, H, W, Cout, k, k, 1,
               pads, pads, 1, None, st)
    # bnstats: bias-free; outputs must equal the plain launch
    yps = [Canvas((B, Cout, H, W), BF, dev, pitch=ld(Cout)) for _ in range(G)]
    with routes.part("grouped y no bias"):
        L.call("cn_conv2d_fwd_grouped_bf16", G, _tab(xptr), xcs[0].pitch, _tab([w.data_ptr() for w in wps]), None,
               _tab([y.ptr for y in yps]), yps[0].pitch, B, Cin, H, W, Cout, k, k, 1, pads, pads, 0, None, st)
    rows = L.query("cn_conv2d_stats_rows_bf16", B, H, W, Cout, k, k, 1, 1, 1)
    stats = [torch.empty(rows * 2 * Cout, device=dev) for _ in range(G)]
    means = [torch.empty(Cout, device=dev) for _ in range(G)]
    rstds = [torch.empty(Cout, device=dev) for _ in range(G)]
    nbn = L.query("cn_bn_group_workspace_floats_bf16", G, Cout)
    bn_ws = torch.zeros(nbn, device=dev)
    fin = ctypes.c_int(-1)
    ybs = [Canvas((B, Cout, H, W), BF, dev, pitch=ld(Cout)) for _ in range(G)]
    with routes.part("grouped y bnstats", "stats rows and finalize requested"):
        L.call("cn_conv2d_fwd_grouped_bnstats_bf16", G, _tab(xptr), xcs[0].pitch, _tab([w.data_ptr() for w in wps]),
               _tab([y.ptr for y in ybs]), ybs[0].pitch, B, Cin, H, W, Cout, k, k, 1, pads, pads,
               _tab([s.data_ptr() for s in stats]), _tab([m.data_ptr() for m in means]),
               _tab([r.data_ptr() for r in rstds]), None, None, 0.1, 1e-5, bn_ws.data_ptr(), nbn, ctypes.addressof(fin), st)
    dycs = [Canvas((B, Cout, H, W), BF, dev, pitch=ld(Cout), fill=GARB, data=d) for d in dys]
    dxcs = [Canvas((B, Cin, H, W), BF, dev, pitch=ld(Cin)) for _ in range(G)]
    with routes.part("grouped dx"):
        L.call("cn_conv2d_bwd_data_grouped_bf16", G, _tab([d.ptr for d in dycs]), dycs[0].pitch,
               _tab([w.data_ptr() for w in wpts]), _tab([d.ptr for d in dxcs]), dxcs[0].pitch, B, Cin, H, W, Cout, k, k,
               1, pads, pads, 0, st)
    x0s = [ints((B, Cin, H, W), -8, 8, 350 + i) for i in range(G)]
    dxas = [Canvas((B, Cin, H, W), BF, dev, pitch=ld(Cin), data=x0) for x0 in x0s]
    with routes.part("grouped dx +=", "acc"):
        L.call("cn_conv2d_bwd_data_grouped_bf16", G, _tab([d.ptr for d in dycs]), dycs[0].pitch,
               _tab([w.data_ptr() for w in wpts]), _tab([d.ptr for d in dxas]), dxas[0].pitch, B, Cin, H, W, Cout, k, k,
               1, pads, pads, 1, st)
    torch.cuda.synchronize()
    assert fin.value in (0, 1)
    for i in range(G):
        assert_exact(ycs[i].t, rb(refs[i][0]), f"y{i}")
        ycs[i].assert_canary(f"y{i}")
        assert_exact(yas[i].t, bf16_store(refs[i][0], y0s[i], Cout, True), f"y{i} (+=)")
        yas[i].assert_canary(f"y{i} (+=)")
        assert_exact(yps[i].t, rb(refs_nb[i]), f"y{i} no bias")
        assert torch.equal(ybs[i].t.cpu().view(torch.int16), yps[i].t.cpu().view(torch.int16)), f"bnstats y{i}"
        ybs[i].assert_canary(f"bnstats y{i}")
        assert_exact(dxcs[i].t, rb(refs[i][1]), f"dx{i}")
        dxcs[i].assert_canary(f"dx{i}")
        assert_exact(dxas[i].t, bf16_store(refs[i][1], x0s[i], Cin, True), f"dx{i} (+=)")
    routes.verify()


@pytest.mark.parametrize("G,B,Cin,H,W,Cout,k,s,ws_ok", [
    (1, 2, 16, 26, 26, 128, 3, 2, True),    # strided, half-tile 128 couts: statistics finished inside the launch
    (1, 2, 16, 26, 26, 64, 3, 2, True),     # strided, 64 couts
    (1, 2, 72, 13, 13, 128, 1, 1, True),    # 1x1, deep chunks
    (2, 113, 40, 5, 6, 128, 3, 1, False),   # two groups on the full-tile WN 4 route, finalize refused: rows only
])
def test_bnstats_bf16_strided_1x1_refused_exact(G, B, Cin, H, W, Cout, k, s, ws_ok, request, tmp_path):
    """cn_conv2d_fwd_grouped_bnstats_bf16 at the routes of the training step that test_grouped_bf16_exact (3x3, stride
    1) does not take: y equals float64 rounded to nearest even; with the finalize granted the means are the float64
    means within 2^-20 (one fp32 division of an exact integer sum), and with the workspace withheld (ws_ok False) the
    launch reports finalized = 0 and its per-tile rows sum to the exact per-channel sums."""
    dev = _dev()
    L, st = lib(), stream()
    T, p = k * k, k // 2
    Ho, Wo = out_size(H, W, k, s, p, 1)
    xs = [ints((B, Cin, H, W), -4, 4, 360)] * G
    wts = [ints((Cout, Cin, k, k), -3, 3, 361 + i) for i in range(G)]
    premise("bnstats", term_bound(xs[0], wts[0], Cin * T), 16)
    y64 = [F.conv2d(xs[i], wts[i], None, s, p, 1) for i in range(G)]
    premise("bnstats channel sums", float(max(v.abs().max() for v in y64)) * B * Ho * Wo)
    ld = lambda c: (c + 7) // 8 * 8 + 8
    xc = Canvas(xs[0].shape, BF, dev, pitch=ld(Cin), fill=GARB, data=xs[0])
    wps = [pack_bf16(w.float().to(dev), T, Cin, Cout, T, Cin * T, 1) for w in wts]
    rows = L.query("cn_conv2d_stats_rows_bf16", B, H, W, Cout, k, k, s, p, 1)
    stats = [torch.full((rows * 2 * Cout,), float("nan"), device=dev) for _ in range(G)]
    means = [torch.full((Cout,), float("nan"), device=dev) for _ in range(G)]
    rstds = [torch.full((Cout,), float("nan"), device=dev) for _ in range(G)]
    nbn = L.query("cn_bn_group_workspace_floats_bf16", G, Cout)
    bn_ws = torch.zeros(nbn, device=dev)
    fin = ctypes.c_int(-1)
    ycs = [Canvas((B, Cout, Ho, Wo), BF, dev, pitch=ld(Cout)) for _ in range(G)]
    pads = _ints_c([p] * G)
    dils = _ints_c([1] * G)
    routes = Routes(case_id(request), tmp_path)
    with routes.part("y bnstats", "finalize workspace given" if ws_ok else "finalize workspace withheld"):
        L.call("cn_conv2d_fwd_grouped_bnstats_bf16", G, _tab([xc.ptr] * G), xc.pitch, _tab([w.data_ptr() for w in wps]),
               _tab([y.ptr for y in ycs]), ycs[0].pitch, B, Cin, H, W, Cout, k, k, s, pads, dils,
               _tab([t.data_ptr() for t in stats]), _tab([m.data_ptr() for m in means]),
               _tab([r.data_ptr() for r in rstds]), None, None, 0.1, 1e-5, bn_ws.data_ptr(), nbn if ws_ok else 0,
               ctypes.addressof(fin), st)
    torch.cuda.synchronize()
    assert fin.value == int(ws_ok), fin.value
    for i in range(G):
        assert_exact(ycs[i].t, rb(y64[i]), f"y{i}")
        ycs[i].assert_canary(f"y{i}")
        if ws_ok:
            m64 = y64[i].mean(dim=(0, 2, 3))
            err = (means[i].double().cpu() - m64).abs()
            assert bool((err <= 2.0 ** -20 * m64.abs().clamp_min(1.0)).all()), f"mean{i}: worst {float(err.max())}"
        else:
            got = stats[i].double().cpu().view(rows, 2, Cout)[:, 0].sum(0)
            assert_exact(got, y64[i].sum(dim=(0, 2, 3)), f"row sums {i}")
    routes.verify()


@pytest.mark.parametrize("B,Cin,H,W,Cout,k,s,p,d,res", [
    (2, 16, 13, 13, 32, 3, 1, 1, 1, True),
    (1, 24, 7, 5, 8, 3, 2, 1, 1, False),
    (2, 64, 25, 25, 128, 3, 1, 2, 2, True),
    (2, 40, 10, 10, 64, 1, 1, 0, 1, True),
])
def test_fused_bf16_exact(B, Cin, H, W, Cout, k, s, p, d, res, request, tmp_path):
    """cn_conv2d_fwd_fused_bf16, act 0: y = bf16(bf16(conv(x, W * scale) + bias) + res), with the weights packed by
    cn_pack_weights_scaled_bf16 under power-of-two scales (exact)."""
    dev = _dev()
    L, st = lib(), stream()
    T = k * k
    Ho, Wo = out_size(H, W, k, s, p, d)
    x = ints((B, Cin, H, W), -4, 4, 400)
    w = ints((Cout, Cin, k, k), -3, 3, 401)
    g = torch.Generator().manual_seed(402)
    scale = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], dtype=torch.float64)[torch.randint(0, 5, (Cout,), generator=g)]
    b = ints((Cout,), -8, 8, 403)
    r = ints((B, Cout, Ho, Wo), -8, 8, 404) if res else None
    ws = w * scale.view(-1, 1, 1, 1)
    premise("fused", term_bound(x, ws, Cin * T), 16)
    y64 = F.conv2d(x, ws, b, s, p, d)
    ref = rb(rb(y64) + r) if res else rb(y64)
    ld = lambda c: (c + 7) // 8 * 8 + 8
    xc = Canvas(x.shape, BF, dev, pitch=ld(Cin), fill=GARB, data=x)
    rc = Canvas(r.shape, BF, dev, pitch=ld(Cout) + 8, fill=GARB, data=r) if res else None
    yc = Canvas(y64.shape, BF, dev, pitch=ld(Cout))
    wp = pack_bf16(w.float().to(dev), T, Cin, Cout, T, Cin * T, 1, nscale=scale.float().to(dev))
    bd = b.float().to(dev)
    routes = Routes(case_id(request), tmp_path)
    with routes.part("fused y", "res" if res else "no res"):
        L.call("cn_conv2d_fwd_fused_bf16", xc.ptr, xc.pitch, wp.data_ptr(), bd.data_ptr(), rc.ptr if res else None,
               rc.pitch if res else 0, yc.ptr, yc.pitch, B, Cin, H, W, Cout, k, k, s, p, d, 0, st)
    torch.cuda.synchronize()
    assert_exact(yc.t, ref, "fused y")
    yc.assert_canary("fused y")
    if res:  # in place: res aliases y
        ya = Canvas(y64.shape, BF, dev, pitch=ld(Cout), data=r)
        with routes.part("fused y in place", "res"):
            L.call("cn_conv2d_fwd_fused_bf16", xc.ptr, xc.pitch, wp.data_ptr(), bd.data_ptr(), ya.ptr, ya.pitch, ya.ptr,
                   ya.pitch, B, Cin, H, W, Cout, k, k, s, p, d, 0, st)
        torch.cuda.synchronize()
        assert_exact(ya.t, ref, "fused y (res aliases y)")
        ya.assert_canary("fused y in place")
    routes.verify()


@pytest.mark.parametrize("B,Cin,H,W,Cout,s,acc", [
    (2, 16, 13, 13, 16, 2, False),
    (2, 32, 25, 25, 32, 2, True),
    (1, 128, 50, 50, 128, 2, False),   # 50 -> 99
    (2, 32, 7, 7, 24, 4, False),       # stride 4
    (1, 24, 5, 6, 31, 2, True),        # ragged couts, tiny plane
    (1, 128, 25, 25, 128, 4, False),   # 25 -> 97
    # interleaved parity classes at the block counts of the training step (route ledger): full-tile WN 4, 64 couts
    (4, 128, 25, 25, 128, 4, False),
    (32, 128, 13, 13, 128, 2, False),
    (2, 64, 50, 50, 64, 2, False),
])
def test_conv_transpose2d_bf16_exact(B, Cin, H, W, Cout, s, acc, request, tmp_path):
    dev = _dev()
    routes = Routes(case_id(request), tmp_path)
    facts = ("acc",) if acc else ()
    L, st = lib(), stream()
    k, p, T = 3, 1, 9
    Ho, Wo = (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
    x = ints((B, Cin, H, W), -4, 4, 500)
    w = ints((Cin, Cout, k, k), -3, 3, 501)
    b = ints((Cout,), -8, 8, 502)
    dy = ints((B, Cout, Ho, Wo), -3, 3, 503)
    y0 = ints((B, Cout, Ho, Wo), -8, 8, 504) if acc else None
    x0 = ints((B, Cin, H, W), -8, 8, 505) if acc else None
    w0 = ints(w.shape, -8, 8, 506)
    premise("convT bf16", term_bound(x, w, Cin * T), 16)
    premise("convT bf16 dx", term_bound(dy, w, Cout * T), 8)
    premise("convT bf16 dw", term_bound(x, dy, B * H * W), 8)
    y64, dx64, dw64 = ref_convT(x, w, b, dy, s, p)
    ld = lambda c: (c + 7) // 8 * 8 + 8
    wd = w.float().to(dev)
    xc = Canvas(x.shape, BF, dev, pitch=ld(Cin), fill=GARB, data=x)
    yc = Canvas(y64.shape, BF, dev, pitch=ld(Cout), data=y0)
    # (every device argument stays referenced until the launches are done: a temporary freed at data_ptr() can be
    # handed to the next allocation before the kernel reads it)
    wp, wpt, bd = pack_bf16(wd, T, Cin, Cout, Cout * T, T, 1), pack_bf16(wd, T, Cout, Cin, T, Cout * T, 1), b.float().to(dev)
    with routes.part("transposed y", *facts):
        L.call("cn_conv_transpose2d_fwd_bf16", xc.ptr, xc.pitch, wp.data_ptr(), bd.data_ptr(), yc.ptr, yc.pitch, B, Cin,
               H, W, Cout, k, k, s, p, int(acc), st)
    dyc = Canvas(dy.shape, BF, dev, pitch=ld(Cout), fill=GARB, data=dy)
    dxc = Canvas(x.shape, BF, dev, pitch=ld(Cin), data=x0)
    with routes.part("transposed dx", *facts):
        L.call("cn_conv_transpose2d_bwd_data_bf16", dyc.ptr, dyc.pitch, wpt.data_ptr(), dxc.ptr, dxc.pitch, B, Cin, H, W,
               Cout, k, k, s, p, int(acc), st)
    torch.cuda.synchronize()
    assert_exact(yc.t, bf16_store(y64, y0, Cout, acc), "y")
    yc.assert_canary("y")
    assert_exact(dxc.t, bf16_store(dx64, x0, Cin, acc), "dx")
    dxc.assert_canary("dx")
    for mode in ("full", "one"):
        n = bwgrad_ws_floats(B, Cin, H, W, Cout, k, s, p, 1, 1, mode)
        ws = torch.empty(n + 4, device=dev)
        dwc = Canvas(w.shape, F32, dev, data=w0)
        with routes.part(f"transposed dw ws {mode}"):
            L.call("cn_conv_transpose2d_bwd_weight_bf16", xc.ptr, xc.pitch, dyc.ptr, dyc.pitch, dwc.ptr, B, Cin, H, W,
                   Cout, k, k, s, p, ws.data_ptr(), n, st)
        torch.cuda.synchronize()
        assert_exact(dwc.t, dw64 + w0, f"dw ws={mode}")
        dwc.assert_canary("dw")
    routes.verify()


# ---------------------------------------------------------------------------------------------------------------------
# weight packs, autotune, the forced tile / split sweep
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout,cin,k", [(31, 9, 3), (129, 72, 3), (40, 136, 1)])
def test_pack_weights_batched_equal_single(cout, cin, k):
    """cn_pack_weights_batched_f32 / cn_pack_weights_batched_bf16 write what the single packs write, bit for bit."""
    from cultionet_amd import engine as E

    dev = _dev()
    L, st = lib(), stream()
    T = k * k
    w = ints((cout, cin, k, k), -3, 3, 600).float().to(dev)
    pats = [(T, cin, cout, T, cin * T, 1), (T, cout, cin, cin * T, T, 1)]
    singles, outs, buf, singles16, outs16, buf16 = [], [], bytearray(), [], [], bytearray()
    for (T_, K, N, sk, sn, s1) in pats:
        a = pack_f32(w, T_, K, N, sk, sn, s1)
        o = torch.full_like(a, float("nan"))
        buf += E.PACK_F32.record(w.data_ptr(), o.data_ptr(), T_, K, N, sk, sn, s1)
        singles.append(a)
        outs.append(o)
        a16 = pack_bf16(w, T_, K, N, sk, sn, s1)
        o16 = torch.full_like(a16, float("nan"))
        buf16 += E.PACK_BF16.record(w.data_ptr(), o16.data_ptr(), T_, K, N, sk, sn, s1)
        singles16.append(a16)
        outs16.append(o16)
    t32 = torch.frombuffer(buf, dtype=torch.uint8).clone().to(dev)
    t16 = torch.frombuffer(buf16, dtype=torch.uint8).clone().to(dev)
    L.call("cn_pack_weights_batched_f32", t32.data_ptr(), len(pats), st)
    L.call("cn_pack_weights_batched_bf16", t16.data_ptr(), len(pats), st)
    torch.cuda.synchronize()
    for a, o in zip(singles + singles16, outs + outs16):
        assert torch.equal(a.cpu().view(torch.int16 if a.dtype == BF else torch.int32),
                           o.cpu().view(torch.int16 if o.dtype == BF else torch.int32))


def test_autotune_exact():
    """cn_conv_set_autotune(1): the tuning launch (candidates timed, output rewritten), the cached-choice launch and an
    accumulating one all give the exact result."""
    dev = _dev()
    L, st = lib(), stream()
    B, Cin, H, W, Cout = 2, 88, 23, 23, 120  # a shape no other test launches: the first launch tunes
    x = ints((B, Cin, H, W), -4, 4, 700)
    w = ints((Cout, Cin, 3, 3), -3, 3, 701)
    b = ints((Cout,), -8, 8, 702)
    y0 = ints((B, Cout, H, W), -8, 8, 703)
    premise("autotune", term_bound(x, w, Cin * 9), 16)
    y64 = F.conv2d(x, w, b, 1, 1)
    wp = pack_f32(w.float().to(dev), 9, Cin, Cout, 9, Cin * 9, 1)
    bd = b.float().to(dev)
    xc = Canvas(x.shape, F32, dev, fill=GARB, data=x)
    try:
        with conv_workspace("ws"):
            L.call("cn_conv_set_autotune", 1)
            for i, acc in enumerate((0, 0, 1)):
                yc = Canvas(y64.shape, F32, dev, data=y0 if acc else None)
                L.call("cn_conv2d_fwd_f32", xc.ptr, xc.pitch, wp.data_ptr(), bd.data_ptr(), yc.ptr, yc.pitch, B, Cin, H,
                       W, Cout, 3, 3, 1, 1, 1, acc, st)
                torch.cuda.synchronize()
                assert_exact(yc.t, y64 + (y0 if acc else 0), f"launch {i} (accumulate {acc})")
                yc.assert_canary(f"launch {i}")
    finally:
        L.call("cn_conv_set_autotune", 0)


SWEEP_PAIRS = [(cfg, sp) for cfg in (0, 1, 2) for sp in (1, 2, 3, 5, 32)]


def test_forced_tile_split_sweep():
    """Every (pixel-tile config, K split) pair forced through CN_DBG_CFG / CN_DBG_SPLITS (read once per process, so
    one fresh child per pair; the kernel clamps both), exact against float64 in the child. Children run one at a
    time; the first failure -- an assertion, a crash or a timeout -- ends the sweep."""
    worker = os.path.join(ROOT, "tests", "conv_exact_worker.py")
    for cfg, sp in SWEEP_PAIRS:
        env = dict(os.environ, CN_DBG_CFG=str(cfg), CN_DBG_SPLITS=str(sp))
        try:
            r = subprocess.run([sys.executable, worker], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            pytest.fail(f"CN_DBG_CFG={cfg} CN_DBG_SPLITS={sp}: the child timed out")
        assert r.returncode == 0, (f"CN_DBG_CFG={cfg} CN_DBG_SPLITS={sp}: child exit {r.returncode}\n"
                                   f"{r.stdout[-2000:]}\n{r.stderr[-4000:]}")


# ---------------------------------------------------------------------------------------------------------------------
# layer 2: random inputs, per-element float64 bounds
# ---------------------------------------------------------------------------------------------------------------------

def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("case", [(2, 8, 13, 13, 32, 3, 1, 1, 1, True), (2, 24, 12, 12, 40, 3, 2, 1, 1, False),
                                  (1, 64, 9, 9, 136, 1, 1, 0, 1, True), (2, 16, 14, 14, 64, 3, 1, 2, 2, True)])
def test_conv2d_bf16_random_bound(case):
    """bf16 forward (bf16 and fp32 outputs) and backward-data on random inputs: fp32 weights packed to bf16 by the
    kernel; the reference rounds them to nearest even."""
    dev = _dev()
    L, st = lib(), stream()
    B, Cin, H, W, Cout, k, s, p, d, bias = case
    T = k * k
    Ho, Wo = out_size(H, W, k, s, p, d)
    x = rb(_randn((B, Cin, H, W), 800))
    w = _randn((Cout, Cin, k, k), 801, (Cin * T) ** -0.5).float().double()
    b = _randn((Cout,), 802).float().double() if bias else None
    dy = rb(_randn((B, Cout, Ho, Wo), 803))
    wr = rb(w)
    y64, dx64, _ = ref_conv(x, wr, b, dy, s, p, d)
    yabs, dxabs, _ = ref_conv(x.abs(), wr.abs(), None if b is None else b.abs(), dy.abs(), s, p, d)
    ld = lambda c: (c + 7) // 8 * 8 + 8
    wd = w.float().to(dev)
    xc = Canvas(x.shape, BF, dev, pitch=ld(Cin), fill=GARB, data=x)
    wp = pack_bf16(wd, T, Cin, Cout, T, Cin * T, 1)
    y32 = Canvas(y64.shape, F32, dev)
    yc = Canvas(y64.shape, BF, dev, pitch=ld(Cout))
    bd = None if b is None else b.float().to(dev)
    bp = None if bd is None else bd.data_ptr()
    wpt = pack_bf16(wd, T, Cout, Cin, Cin * T, T, 1)
    L.call("cn_conv2d_fwd_bf16", xc.ptr, xc.pitch, wp.data_ptr(), bp, y32.ptr, 0, y32.pitch, B, Cin, H, W, Cout, k, k,
           s, p, d, 0, 1, None, st)
    L.call("cn_conv2d_fwd_bf16", xc.ptr, xc.pitch, wp.data_ptr(), bp, yc.ptr, yc.pitch, 0, B, Cin, H, W, Cout, k, k, s,
           p, d, 0, 0, None, st)
    dyc = Canvas(dy.shape, BF, dev, pitch=ld(Cout), fill=GARB, data=dy)
    dx32 = Canvas(x.shape, BF, dev, pitch=ld(Cin))
    L.call("cn_conv2d_bwd_data_bf16", dyc.ptr, dyc.pitch, pack_bf16(wd, T, Cout, Cin, Cin * T, T, 1).data_ptr(),
           dx32.ptr, dx32.pitch, B, Cin, H, W, Cout, k, k, s, p, d, 0, st)
    torch.cuda.synchronize()
    e_y = (Cin * T + 4) * U32 * yabs
    _bounded(y32.t, y64, e_y, "bf16 conv fwd (fp32 out)")
    _bounded(yc.t, y64, e_y + _half_ulp_bf16(y64.abs() + e_y), "bf16 conv fwd (bf16 out)")
    e_dx = (Cout * T + 4) * U32 * dxabs
    _bounded(dx32.t, dx64, e_dx + _half_ulp_bf16(dx64.abs() + e_dx), "bf16 conv bwd-data")


@pytest.mark.parametrize("B,Cin,H,W,Cout,k,res", [(2, 16, 13, 13, 32, 3, True), (2, 24, 12, 12, 64, 1, False),
                                                   (1, 64, 25, 25, 128, 3, True)])
@pytest.mark.parametrize("act", [0, 1])
def test_fused_bf16_random_bound(B, Cin, H, W, Cout, k, res, act):
    """cn_conv2d_fwd_fused_bf16 with random (non power-of-two) scales in cn_pack_weights_scaled_bf16 and SiLU.
    SiLU is v / (1 + __expf(-v)): __expf evaluates exp2(-v * log2 e), whose argument rounding costs |v| u relative and
    the exp2 itself ~1 ulp; with the add and the division the activation is within (|v| + 8) u |silu(v)| of
    silu(fl(v)), and its slope is within [-0.1, 1.1]."""
    dev = _dev()
    L, st = lib(), stream()
    T = k * k
    p = k // 2
    x = rb(_randn((B, Cin, H, W), 900, 2.0))
    w = _randn((Cout, Cin, k, k), 901, (Cin * T) ** -0.5).float().double()
    scale = (_randn((Cout,), 902).abs() + 0.5).float().double()
    b = _randn((Cout,), 903).float().double()
    r = rb(_randn((B, Cout, H, W), 904)) if res else None
    wsd = rb((w.float() * scale.float().view(-1, 1, 1, 1)).double())  # the pack: fp32 product, rounded to bf16
    v64 = F.conv2d(x, wsd, b, 1, p)
    vabs = F.conv2d(x.abs(), wsd.abs(), b.abs(), 1, p)
    e_v = (Cin * T + 4) * U32 * vabs
    if act:
        a64 = F.silu(v64)
        e_a = 1.1 * e_v + (v64.abs() + e_v + 8) * U32 * (a64.abs() + e_v)
    else:
        a64, e_a = v64, e_v
    # bf16(act): half an ulp; then + res and a second rounding
    e1 = e_a + _half_ulp_bf16(a64.abs() + e_a)
    if res:
        ref = a64 + r
        e = e1 + _half_ulp_bf16(ref.abs() + e1)
    else:
        ref, e = a64, e1
    ld = lambda c: (c + 7) // 8 * 8 + 8
    xc = Canvas(x.shape, BF, dev, pitch=ld(Cin), fill=GARB, data=x)
    rc = Canvas(r.shape, BF, dev, pitch=ld(Cout), fill=GARB, data=r) if res else None
    yc = Canvas(v64.shape, BF, dev, pitch=ld(Cout))
    wp = pack_bf16(w.float().to(dev), T, Cin, Cout, T, Cin * T, 1, nscale=scale.float().to(dev))
    L.call("cn_conv2d_fwd_fused_bf16", xc.ptr, xc.pitch, wp.data_ptr(), b.float().to(dev).data_ptr(),
           rc.ptr if res else None, rc.pitch if res else 0, yc.ptr, yc.pitch, B, Cin, H, W, Cout, k, k, 1, p, 1, act, st)
    torch.cuda.synchronize()
    _bounded(yc.t, ref, e, f"fused bf16 act {act} res {res}")
    yc.assert_canary("fused y")


@pytest.mark.parametrize("case", [(2, 9, 13, 13, 33, 3, 1, 1, 1, True), (2, 64, 7, 7, 256, 3, 1, 1, 1, True),
                                  (4, 48, 100, 100, 129, 1, 1, 0, 1, True)])
@pytest.mark.parametrize("ws", ["ws", "none"])
def test_conv2d_f32_random_bound(case, ws):
    """fp32 forward / backward-data on random inputs: D = K terms + the split partials."""
    dev = _dev()
    L, st = lib(), stream()
    B, Cin, H, W, Cout, k, s, p, d, bias = case
    T = k * k
    Ho, Wo = out_size(H, W, k, s, p, d)
    x = _randn((B, Cin, H, W), 1000).float().double()
    w = _randn((Cout, Cin, k, k), 1001, (Cin * T) ** -0.5).float().double()
    b = _randn((Cout,), 1002).float().double()
    dy = _randn((B, Cout, Ho, Wo), 1003).float().double()
    y64, dx64, _ = ref_conv(x, w, b, dy, s, p, d)
    yabs, dxabs, _ = ref_conv(x.abs(), w.abs(), b.abs(), dy.abs(), s, p, d)
    wd = w.float().to(dev)
    with conv_workspace(ws):
        xc = Canvas(x.shape, F32, dev, fill=GARB, data=x)
        yc = Canvas(y64.shape, F32, dev)
        # both operands stay referenced until the launch is queued: a temporary pack would be freed as soon as its
        # pointer is taken, and the bias allocated next may land inside its block and overwrite the first weights
        wp, bd = pack_f32(wd, T, Cin, Cout, T, Cin * T, 1), b.float().to(dev)
        L.call("cn_conv2d_fwd_f32", xc.ptr, xc.pitch, wp.data_ptr(), bd.data_ptr(), yc.ptr, yc.pitch, B, Cin, H, W, Cout,
               k, k, s, p, d, 0, st)
        dyc = Canvas(dy.shape, F32, dev, fill=GARB, data=dy)
        dxc = Canvas(x.shape, F32, dev)
        L.call("cn_conv2d_bwd_data_f32", dyc.ptr, dyc.pitch, pack_f32(wd, T, Cout, Cin, Cin * T, T, 1).data_ptr(),
               dxc.ptr, dxc.pitch, B, Cin, H, W, Cout, k, k, s, p, d, 0, st)
        torch.cuda.synchronize()
    _bounded(yc.t, y64, (Cin * T + 32 + 4) * U32 * yabs, f"f32 conv fwd ws={ws}")
    _bounded(dxc.t, dx64, (Cout * T + 32 + 4) * U32 * dxabs, f"f32 conv bwd-data ws={ws}")
