"""The premises of tests/test_conv_exact_gpu.py, proven on the CPU: integer convolutions are exact in fp32, torch rounds
bf16 ties to even, the premise check rejects inputs whose partial sums could leave fp32's exact integers, and every
convolution entry point of the C ABI is exercised by the exact GPU tests."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from conv_exact_worker import BF, LIMIT, bf16_store, ints, premise, rb, ref_conv, ref_convT, term_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", [
    # B, Cin, H, W, Cout, k, stride, pad, dil
    (2, 9, 13, 11, 33, 3, 1, 1, 1),
    (2, 24, 11, 11, 64, 3, 2, 1, 1),
    (1, 16, 14, 14, 31, 3, 1, 3, 3),
    (2, 130, 9, 11, 128, 1, 1, 0, 1),
    (8, 64, 25, 25, 32, 3, 1, 1, 1),
])
def test_integer_convolutions_are_exact_in_fp32(case):
    B, Cin, H, W, Cout, k, s, p, d = case
    x = ints((B, Cin, H, W), -4, 4, 1)
    w = ints((Cout, Cin, k, k), -3, 3, 2)
    b = ints((Cout,), -8, 8, 3)
    y64 = F.conv2d(x, w, b, s, p, d)
    dy = ints(y64.shape, -3, 3, 4)
    premise("cpu", term_bound(x, w, Cin * k * k), 8)
    premise("cpu dw", term_bound(x, dy, B * y64.shape[-1] * y64.shape[-2]))
    y64, dx64, dw64 = ref_conv(x, w, b, dy, s, p, d)
    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    yf = F.conv2d(xf, wf, b.float(), s, p, d)
    dxf, dwf = torch.autograd.grad(yf, (xf, wf), dy.float())
    assert torch.equal(yf.detach().double(), y64)
    assert torch.equal(dxf.double(), dx64)
    assert torch.equal(dwf.double(), dw64)
    # bf16 operands hold these integers exactly
    assert torch.equal(x.to(BF).double(), x) and torch.equal(w.to(BF).double(), w)


def test_integer_transposed_convolution_is_exact_in_fp32():
    x = ints((2, 16, 13, 13), -4, 4, 5)
    w = ints((16, 24, 3, 3), -3, 3, 6)
    y64 = F.conv_transpose2d(x, w, None, 2, 1, output_padding=1)
    dy = ints(y64.shape, -3, 3, 7)
    y64, dx64, dw64 = ref_convT(x, w, None, dy, 2, 1, 1)
    xf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
    yf = F.conv_transpose2d(xf, wf, None, 2, 1, output_padding=1)
    dxf, dwf = torch.autograd.grad(yf, (xf, wf), dy.float())
    assert torch.equal(yf.detach().double(), y64)
    assert torch.equal(dxf.double(), dx64)
    assert torch.equal(dwf.double(), dw64)


def test_torch_rounds_bf16_ties_to_even():
    v = torch.tensor([255, 256, 257, 258, 259, 261, 263, 511, -257, -259, 513, 515], dtype=torch.float64)
    want = torch.tensor([255, 256, 256, 258, 260, 260, 264, 512, -256, -260, 512, 516], dtype=torch.float64)
    assert torch.equal(rb(v), want)
    # not truncation, not half-up: 257 -> 256 (half-up gives 258), 259 -> 260 (truncation gives 258)
    assert float(rb(torch.tensor([257.0]))) == 256.0 and float(rb(torch.tensor([259.0]))) == 260.0
    # values between the ties round to nearest
    assert float(rb(torch.tensor([256.9]))) == 256.0 and float(rb(torch.tensor([257.1]))) == 258.0


def test_bf16_store_restates_the_double_rounding_of_accumulate():
    v = torch.tensor([257.0, 300.0])
    old = torch.tensor([1.0, 3.0], dtype=torch.float64)
    # Cout % 8 == 0: bf16(bf16(257) + 1) = bf16(257) = 256; ragged: bf16(258) = 258
    assert bf16_store(v.double(), old, 8, True)[0] == 256.0
    assert bf16_store(v.double(), old, 9, True)[0] == 258.0
    assert torch.equal(bf16_store(v.double(), None, 8, False), rb(v.double()))


def test_premise_rejects_sums_beyond_2_24():
    x = ints((1, 640, 5, 5), -4, 4, 8)
    w = ints((1, 640, 3, 3), -3, 3, 9)
    assert premise("ok", term_bound(x, w, 640 * 9)) < LIMIT
    big = torch.full((1, 1, 1, 1), 2048.0, dtype=torch.float64)
    with pytest.raises(AssertionError, match="2\\^24"):
        premise("overflow", term_bound(big, big, 5))  # 2048 * 2048 * 5 > 2^24
    with pytest.raises(AssertionError, match="2\\^24"):
        premise("overflow", float(LIMIT) - 1, 1.0)
    # and a sum that really is not exact in fp32 once past it
    t = torch.tensor([2.0 ** 24, 1.0], dtype=torch.float32)
    assert float(t.sum()) != 2.0 ** 24 + 1


FAMILY = re.compile(r"\b(cn_conv2d_\w+|cn_conv_transpose2d_\w+|cn_thin_conv3x3_\w+|cn_convt_taps_\w+|cn_pack_weights\w*|"
                    r"cn_pack_timeconv_f32|cn_fold_timeconv_grad_f32)\s*\(")


def test_every_conv_entry_point_is_covered_by_the_exact_tests():
    """New conv-family entry points of include/cultionet_hip.h cannot drift in untested: each must be named by the
    exact GPU tests (tests/test_conv_exact_gpu.py and the checks it shares with tests/conv_exact_worker.py). The
    engine-driven routes (cn_convt_taps_*, cn_pack_timeconv_f32, cn_fold_timeconv_grad_f32) are named in the docstrings
    of the tests that reach them."""
    with open(os.path.join(ROOT, "include", "cultionet_hip.h")) as f:
        header = f.read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(FAMILY.findall(header))
    assert len(names) >= 30, sorted(names)
    text = ""
    for fn in ("test_conv_exact_gpu.py", "conv_exact_worker.py"):
        with open(os.path.join(ROOT, "tests", fn)) as f:
            text += f.read()
    missing = sorted(n for n in names if not re.search(r"\b" + n + r"\b", text))
    assert not missing, f"conv entry points without an exact test: {missing}"
