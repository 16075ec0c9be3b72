"""The fp32 1x1 GEMM family (cn_gemm1x1_kernel behind cn_conv2d_fwd_f32 / cn_conv2d_bwd_data_f32) against float64.

Layer 1: integer inputs (tests/conv_exact_worker.py), every partial sum exact in fp32, so the result must EQUAL the
float64 reference. Layer 2: random inputs within a per-element bound: an output is a chain of Cin fused multiply-adds
in fp32 (the MFMA is an fp32 fma chain, and there is no K split whose partials would add roundings), then the bias and,
for the store, nothing more: |err| <= (Cin + 4) u * sum |terms|, u = 2^-24.

Outputs sit in sentinel-framed buffers, inputs in buffers whose gaps (padded batch strides, the slack behind the last
image) hold NaN: an operand read there reaches the result even through a zero weight. Every launch is made inside a
profiling window: the one kernel recorded must be the GEMM and the library's launch counter must move by
exactly one per convolution -- no K split, no slices, no reduce launch.
"""
from __future__ import annotations

import functools

import pytest
import torch

from conv_exact_worker import (F32, NAN, U32, Canvas, assert_exact, bounded, conv_workspace, ints, lib, pack_f32,
                               premise, ref_conv, stream, term_bound)
from route_ledger import Routes, case_id
from route_ledger import profile_top as _profile_top

pytestmark = pytest.mark.gpu

# (B, Cin, H, W, Cout, k, stride, pad, dil, bias)
CASES = [
    (2, 40, 12, 12, 129, 1, 1, 0, 1, True),    # Cin below a chunk boundary, ragged second cout tile, HW 144
    (2, 128, 16, 20, 300, 1, 1, 0, 1, False),  # three cout tiles, HW 320 = exact tiles
    (2, 130, 9, 12, 128, 1, 1, 0, 1, True),    # K loop, ragged last chunk
    (1, 161, 8, 8, 64, 1, 1, 0, 1, False),     # K loop, ragged last chunk, 64 couts
    (2, 8, 4, 4, 32, 1, 1, 0, 1, True),        # smallest tiles: Cout 32, 33, 65; HW 16, 36, 40
    (2, 7, 6, 6, 33, 1, 1, 0, 1, False),
    (1, 33, 5, 8, 65, 1, 1, 0, 1, True),
    (2, 40, 13, 13, 128, 1, 1, 0, 1, True),    # HW % 4 == 1
    (2, 24, 7, 6, 48, 1, 1, 0, 1, False),      # HW % 4 == 2
    (3, 130, 9, 11, 128, 1, 1, 0, 1, True),    # HW % 4 == 3
    (8, 128, 25, 25, 1152, 1, 1, 0, 1, True),  # production odd planes
    (8, 1152, 25, 25, 128, 1, 1, 0, 1, False),
    (8, 256, 13, 13, 256, 1, 1, 0, 1, True),
    (8, 576, 50, 50, 128, 1, 1, 0, 1, False),  # production 50x50: was K split 4 + reduce
    # the 128 x 160 tile is chosen only when its blocks fill the chip (>= 256): the smallest such launches, with ragged
    # Cin / Cout and a pixel tail, and with full 128-channel chunks and three cout tiles
    (8, 40, 63, 80, 129, 1, 1, 0, 1, True),
    (8, 128, 72, 72, 300, 1, 1, 0, 1, False),
    (8, 72, 12, 12, 256, 1, 1, 0, 1, True),    # the 32 x 64 tile on an aligned plane
]
IDS = ["x".join(str(v) for v in c[:5]) + ("b" if c[9] else "") for c in CASES]


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g, dtype=torch.float64) * scale).float().double()


@functools.lru_cache(maxsize=None)
def _problem(case, kind, accumulate):
    """Inputs and float64 references of one case, computed once and shared (never modified) by the tests."""
    B, Cin, H, W, Cout, k, s, p, d, bias = case
    assert (k, s, p, d) == (1, 1, 0, 1)
    if kind == "int":
        x = ints((B, Cin, H, W), -4, 4, 11)
        w = ints((Cout, Cin, 1, 1), -3, 3, 12)
        b = ints((Cout,), -8, 8, 13) if bias else None
        dy = ints((B, Cout, H, W), -3, 3, 14)
        y0 = ints((B, Cout, H, W), -8, 8, 15) if accumulate else None
        x0 = ints((B, Cin, H, W), -8, 8, 16) if accumulate else None
        premise(f"1x1 {case}", term_bound(x, w, Cin), 8 + 8)
        premise(f"1x1 {case} dx", term_bound(dy, w, Cout), 8)
    else:
        x = _randn((B, Cin, H, W), 21)
        w = _randn((Cout, Cin, 1, 1), 22, Cin ** -0.5)
        b = _randn((Cout,), 23) if bias else None
        dy = _randn((B, Cout, H, W), 24)
        y0 = x0 = None
    y64, dx64, _ = ref_conv(x, w, b, dy)
    yabs = dxabs = None
    if kind != "int":
        yabs, dxabs, _ = ref_conv(x.abs(), w.abs(), None if b is None else b.abs(), dy.abs())
    return x, w, b, dy, y0, x0, y64, dx64, yabs, dxabs


def _launch_counted(routes, label, name, *args):
    """One library call inside a profiling window (the part `label` of the test's route recorder, which always closes
    the window): (launches, [(kernel name, launches recorded)])."""
    L = lib()
    torch.cuda.synchronize()
    n0 = L.query("cn_launch_count", 0)
    with routes.part(label):
        L.call(name, *args)
        torch.cuda.synchronize()
    n1 = L.query("cn_launch_count", 0)
    return n1 - n0, _profile_top()


def _assert_one_gemm(launches, recs, what):
    assert launches == 1, f"{what}: {launches} launches for one convolution (K split / reduce?) {recs}"
    assert len(recs) == 1 and recs[0][0].startswith("cn_gemm1x1_kernel<") and recs[0][1] == 1, f"{what}: recorded {recs}"


def _check(case, kind, ws, request, tmp_path, accumulate=False, xpad=0, ypad=0):
    B, Cin, H, W, Cout, k, s, p, d, bias = case
    x, w, b, dy, y0, x0, y64, dx64, yabs, dxabs = _problem(case, kind, accumulate)
    dev = torch.device("cuda")
    st = stream()
    wd = w.float().to(dev)
    bd = b.float().to(dev) if bias else None
    acc = int(accumulate)
    routes = Routes(case_id(request), tmp_path, "ws" if ws == "ws" else "atomics", *(["acc"] if accumulate else []))
    with conv_workspace(ws):
        xc = Canvas(x.shape, F32, dev, pitch=Cin * H * W + xpad, fill=NAN, data=x)
        yc = Canvas(y64.shape, F32, dev, pitch=Cout * H * W + ypad, data=y0)
        wp = pack_f32(wd, 1, Cin, Cout, 1, Cin, 1)
        n, recs = _launch_counted(routes, "y", "cn_conv2d_fwd_f32", xc.ptr, xc.pitch, wp.data_ptr(),
                                  None if bd is None else bd.data_ptr(), yc.ptr, yc.pitch, B, Cin, H, W, Cout, 1,
                                  1, 1, 0, 1, acc, st)
        _assert_one_gemm(n, recs, f"y {case}")
        dyc = Canvas(dy.shape, F32, dev, pitch=Cout * H * W + ypad, fill=NAN, data=dy)
        dxc = Canvas(x.shape, F32, dev, pitch=Cin * H * W + xpad, data=x0)
        wpt = pack_f32(wd, 1, Cout, Cin, Cin, 1, 1)
        n, recs = _launch_counted(routes, "dx", "cn_conv2d_bwd_data_f32", dyc.ptr, dyc.pitch, wpt.data_ptr(), dxc.ptr,
                                  dxc.pitch, B, Cin, H, W, Cout, 1, 1, 1, 0, 1, acc, st)
        _assert_one_gemm(n, recs, f"dx {case}")
    if kind == "int":
        assert_exact(yc.t, y64 + (y0 if accumulate else 0), f"y {case} ws={ws}")
        assert_exact(dxc.t, dx64 + (x0 if accumulate else 0), f"dx {case} ws={ws}")
    else:
        bounded(yc.t, y64, (Cin + 4) * U32 * yabs, f"y {case} ws={ws}")
        bounded(dxc.t, dx64, (Cout + 4) * U32 * dxabs, f"dx {case} ws={ws}")
    yc.assert_canary(f"y {case}")
    dxc.assert_canary(f"dx {case}")
    if kind == "int":  # (the random-input twins run the same launches: the exact tests hold the route)
        routes.verify()


@pytest.mark.parametrize("ws", ["ws", "none"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv1x1_gemm_exact(case, ws, request, tmp_path):
    _check(case, "int", ws, request, tmp_path)


@pytest.mark.parametrize("ws", ["ws", "none"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv1x1_gemm_random_bound(case, ws, request, tmp_path):
    _check(case, "rand", ws, request, tmp_path)


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3], CASES[7], CASES[9], CASES[12], CASES[14]],
                         ids=[IDS[i] for i in (0, 1, 3, 7, 9, 12, 14)])
def test_conv1x1_gemm_exact_accumulate(case, request, tmp_path):
    """accumulate=True adds to integer-prefilled outputs."""
    _check(case, "int", "ws", request, tmp_path, accumulate=True)


@pytest.mark.parametrize("case,xpad,ypad", [(CASES[0], 1, 3), (CASES[7], 1, 3), (CASES[1], 4, 8), (CASES[1], 2, 5),
                                            (CASES[9], 3, 1), (CASES[12], 1, 3), (CASES[13], 1, 3)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_conv1x1_gemm_exact_padded_batch_strides(case, xpad, ypad, accumulate, request, tmp_path):
    """Padded batch strides of inputs and outputs, including ones that break the 16-byte alignment of every image but
    the first: such launches stage their pixel rows with 4-byte pieces and stay one launch."""
    _check(case, "int", "ws", request, tmp_path, accumulate=accumulate, xpad=xpad, ypad=ypad)


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[7], CASES[10]], ids=[IDS[i] for i in (0, 4, 7, 10)])
def test_conv1x1_gemm_exact_bias_off_and_on(case, request, tmp_path):
    """The same shape with the bias flag flipped (the case list fixes one setting per shape)."""
    _check(case[:9] + (not case[9],), "int", "ws", request, tmp_path)
