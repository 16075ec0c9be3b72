"""The tiled fp32 neighborhood-attention kernels (cn_na2d_*_tiled_kernel of cn_na2d.hip) through the C ABI against the
float64 reference and the per-element bounds of tests/attention_ref.py, which hold for any summation order. The
launcher's rule (na_tile_rows) is restated here, so that every case is known to run the tiled kernels or the
one-lane-per-(pixel, head) ones, and with how many rows per block. Every tensor sits in a NaN-guarded buffer as in
tests/test_attention_gpu.py; `pad` adds floats to the batch stride, so that planes whose size is a multiple of 4 still
start off a 16-byte boundary in the second batch item (the dword staging path)."""
import numpy as np
import pytest
import torch

import attention_ref as R
from test_attention_gpu import PAT32, SEED, Flat32, _check_all, _dev, _problem, _s, _step_word

pytestmark = pytest.mark.gpu

THREADS, PPT, CH, MIN_PIXELS = 256, 2, 8, 512


def tile_rows(case):
    """na_tile_rows of cn_na2d.hip: rows per block of the tiled kernels, 0 for the per-pixel kernels."""
    B, heads, D, H, W, dil = case
    if D not in (16, 32) or W > 256 or H * W < MIN_PIXELS:
        return 0
    rows = min(H, THREADS * PPT // W)
    while rows > 1 and -(-H // rows) * heads * B < 512 and ((rows + 1) // 2) * W >= THREADS * 3 // 4:
        rows = (rows + 1) // 2
    if CH * min(H, rows + 4 * dil) * W * 4 > 65536:
        return 0
    return rows


# (B, heads, D, H, W, dilation) -> rows per block the rule must give (0: the per-pixel kernels)
CASES = {
    "odd_plane_dil2": ((2, 4, 32, 37, 41, 2), 6),     # H = 6 * 6 + 1, W % 4 = 1, odd batch stride, two pixels per lane
    "site_c_25x25": ((1, 8, 16, 25, 25, 1), 10),       # D = 16, 8 heads; strips of 10, 10 and 5 rows
    "aligned_33x64": ((2, 4, 32, 33, 64, 1), 4),       # 16-byte staging; H = 8 * 4 + 1
    "h_3dil_wide": ((1, 2, 32, 9, 70, 3), 4),          # the smallest legal H at dilation 3; strips of 4, 4 and 1 rows
    "h_3dil_w100": ((1, 4, 32, 6, 100, 2), 2),         # H = 3 * dilation, W = 100: 16-byte staging
    "site_b_50x50": ((2, 4, 32, 50, 50, 1), 5),       # 16-byte and dword staging by the strip's row count
    "just_tiled_512px": ((1, 4, 32, 16, 32, 1), 8),    # exactly NAT_MIN_PIXELS; halved once: one pixel per lane, no second
    "just_small_511px": ((1, 4, 32, 7, 73, 1), 0),
    "w256": ((1, 1, 16, 3, 256, 1), 1),
    "w257": ((1, 1, 16, 3, 257, 1), 0),
    "d8_big_plane": ((1, 2, 8, 23, 23, 1), 0),         # a head dimension without a tiled kernel
    "lds_too_large": ((1, 1, 16, 30, 250, 10), 0),     # 8 channels of 30 rows of 250 floats: 240 KB
}


class Padded32:
    """[B, C, H, W] channel slice (offset `lead`) of a flat fp32 buffer of B items of (C + extra) planes + `pad` floats,
    filled with the NaN pattern."""

    def __init__(self, shape, data=None, lead=1, extra=3, pad=0):
        B, C, H, W = shape
        HW = H * W
        self.stride = (C + extra) * HW + pad
        self.flat = torch.empty(B * self.stride, dtype=torch.float32, device=_dev())
        self.flat.view(torch.int32).fill_(PAT32)
        self.t = self.flat.as_strided((B, C, H, W), (self.stride, HW, W, 1), lead * HW)
        self.guard = torch.ones(B * self.stride, dtype=torch.bool, device=_dev())
        self.guard.as_strided((B, C, H, W), (self.stride, HW, W, 1), lead * HW).fill_(False)
        if data is not None:
            self.t.copy_(data.to(_dev()))
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.flat.view(torch.int32)[self.guard] == PAT32).all())

    def get(self):
        return self.t.cpu().contiguous()


def _run(case, qkv, dout, pad=0, p=0.0, seed=0, step=None, save_attn=True):
    from cultionet_amd import _lib

    B, heads, D, H, W, dil = case
    C = heads * D
    q, g = Padded32((B, 3 * C, H, W), qkv, pad=pad), Padded32((B, C, H, W), dout, pad=pad)
    out, dq = Padded32((B, C, H, W), pad=pad), Padded32((B, 3 * C, H, W), pad=pad)
    attn, dattn = Flat32((B, heads, 9, H, W)), Flat32((B, heads, 9, H, W))
    word, wp = _step_word(step)
    _lib.call("cn_na2d_fwd_f32", q.ptr, q.stride, out.ptr, out.stride, attn.ptr if save_attn else None, B, C, heads, H,
              W, 3, dil, float(p), seed, wp, _s())
    res = {}
    if save_attn:
        _lib.call("cn_na2d_bwd_f32", q.ptr, q.stride, g.ptr, g.stride, attn.ptr, dattn.ptr, dq.ptr, dq.stride, B, C,
                  heads, H, W, 3, dil, float(p), seed, wp, _s())
        res.update(attn=attn.get(), dattn=dattn.get(), dqkv=dq.get())
    torch.cuda.synchronize()
    res["out"] = out.get()
    for name, buf in (("qkv", q), ("dout", g), ("out", out), ("dqkv", dq), ("attn", attn), ("dattn", dattn)):
        assert buf.intact(), f"{name}: the padding around the tensor was written"
    return res


def test_the_restated_rule_sorts_the_cases_as_intended():
    for name, (case, rows) in CASES.items():
        assert tile_rows(case) == rows, name
    # the benchmark's three sites: strips of 5 rows at 100 x 100 and 50 x 50, of 10 at 25 x 25
    assert [tile_rows(c) for c in ((8, 4, 32, 100, 100, 2), (8, 4, 32, 50, 50, 1), (8, 8, 16, 25, 25, 1))] == [5, 5, 10]


@pytest.mark.parametrize("name", list(CASES))
def test_na2d_f32_tiled(name):
    case = CASES[name][0]
    qkv, dout, _, ref, bnd = _problem(case, False)
    _check_all(f"na2d f32 tiled {name} rows={tile_rows(case)}", _run(case, qkv, dout), ref, bnd)


@pytest.mark.parametrize("name", ["aligned_33x64", "site_b_50x50"])
def test_na2d_f32_tiled_batch_stride_off_16_bytes(name):
    """Planes of a multiple of 4 floats, a batch stride that is not: the second item takes the dword staging path."""
    case = CASES[name][0]
    assert case[0] == 2 and (case[3] * case[4]) % 4 == 0
    qkv, dout, _, ref, bnd = _problem(case, False)
    _check_all(f"na2d f32 tiled {name} batch stride + 1", _run(case, qkv, dout, pad=1), ref, bnd)


def test_na2d_f32_tiled_attention_dropout_with_a_step_word():
    case = CASES["odd_plane_dil2"][0]
    B, heads, D, H, W, dil = case
    C = heads * D
    p, step = 0.3, 1
    qkv, dout, keep, ref, bnd = _problem(case, False, (p, SEED, step))
    got = _run(case, qkv, dout, p=p, seed=SEED, step=step)
    _check_all("na2d f32 tiled drop 0.3 step1", got, ref, bnd)  # `attn`: the undropped probabilities are saved
    dead = (keep == 0).all(dim=-1)  # [B, heads, H, W]
    rows = dead[:, :, None].expand(B, heads, D, H, W).reshape(B, C, H, W)
    assert bool((got["out"][rows] == 0).all()) and bool((got["dqkv"][:, :C][rows] == 0).all())
    # dropout was on: without the mask the output leaves the undropped reference's bound by far
    _, _, _, ref0, bnd0 = _problem(case, False)
    assert float(((got["out"].double() - ref0["out"]).abs() / bnd0["out"]).max()) > 1e3


@pytest.mark.parametrize("name", ["aligned_33x64", "odd_plane_dil2"])
def test_na2d_f32_tiled_without_saved_probabilities(name):
    """attn = None (inference): the same `out`, bit for bit, as the run that saves the probabilities."""
    case = CASES[name][0]
    qkv, dout, _, ref, bnd = _problem(case, False)
    a = _run(case, qkv, dout, save_attn=False)["out"]
    b = _run(case, qkv, dout)["out"]
    assert torch.equal(a, b)
    R.within(a, ref["out"], bnd["out"], f"na2d f32 tiled {name} attn=None out")
