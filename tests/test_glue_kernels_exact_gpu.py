"""The glue kernels between the compute kernels, through the C ABI, held exactly:

    cn_copy_f32, cn_add_f32, cn_fill_f32                               (cn_pointwise.hip)
    cn_copy_bf16 (modes 0 and 1), cn_add_bf16, cn_zero_bf16            (cn_bops.hip)
    cn_convert_f32nchw_to_bf16nhwc, cn_convert_bf16nhwc_to_f32nchw     (cn_bops.hip)
    cn_channel_sum_bf16                                                (cn_bnorm.hip)

Every output sits in a sentinel-filled canvas with padded strides and slack behind it, and the sentinels must survive;
the gaps of every input hold a finite garbage value that no result may pick up. Copies, adds and converters are compared
for EQUALITY: integers against float64, random data against a reference that restates the kernel's own roundings (one
fp32 add, one round-to-nearest-even into bf16), which IEEE arithmetic on the CPU reproduces bit for bit. Only the
channel sum has a bounded layer, with the bound counted from the kernel (tape_ref.channel_sum_depth) and no floor.

Shapes sit on the kernels' own thresholds: the 1024-element blocks and the 2048-block cap of the fp32 kernels, the
256- / 512-piece steps of cn_bcopy_kernel's two-piece loop and its 16384-block cap, the 8192-block cap of the fill, the
64 x 64 tiles of the converters, and bbn_grid's thread rows, second block and 512-block cap.

NOT run: the 64-bit index instantiation of cn_bcopy_kernel. It is chosen from 2^31 pieces of 16 bytes on, 34 GB per
buffer, which no test of a few seconds can afford; the 32-bit instantiation runs the same body.
"""
import time

import pytest
import torch

import tape_ref as R
from conv_exact_worker import BF, F32, GARB, SENT, Canvas, Flat, assert_exact, bounded, dev, ints, lib, premise, stream

pytestmark = pytest.mark.gpu

I16 = torch.int16


def sync():
    torch.cuda.synchronize()


def randf(shape, seed, scale=3.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale


def canary_outside(cv, c0, C, what):
    """Everything of the canvas' buffer but channels [c0, c0 + C) of its tensor still holds the fill."""
    c = cv.buf.clone()
    cv.view(c)[:, c0:c0 + C].fill_(cv.fill)
    assert bool((c == cv.fill).all()), f"{what}: written outside the destination"


# ---------------------------------------------------------------------------------------------------------------------
# cn_copy_f32 / cn_add_f32 / cn_fill_f32
# ---------------------------------------------------------------------------------------------------------------------

def f32_canvas(x, pad, fill, d):
    """[B, n] float64 -> Canvas with batch stride n + pad."""
    B, n = x.shape
    return Canvas((B, 1, 1, n), F32, d, pitch=n + pad, fill=fill, data=x.view(B, 1, 1, n))


BIG_F32 = 2048 * 1024 + 1025  # past the 2048-block cap: every thread loops 4 times, the first 1025 a fifth time


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 1024, 1025])
def test_copy_add_f32(n, B):
    _copy_add_f32(n, B, seed=n + B)


def test_copy_add_f32_past_the_block_cap():
    _copy_add_f32(BIG_F32, 2, seed=5)


def _copy_add_f32(n, B, seed):
    d, L, st = dev(), lib(), stream()
    a, c, old = (ints((B, n), -100, 100, seed + i) for i in range(3))
    premise(f"copy/add f32 n={n}", 300)
    ac, cc = f32_canvas(a, 3, GARB, d), f32_canvas(c, 7, GARB, d)
    for acc in (0, 1):
        dc = f32_canvas(old, 5, SENT, d)
        L.call("cn_copy_f32", ac.ptr, ac.pitch, dc.ptr, dc.pitch, B, n, acc, st)
        sync()
        assert_exact(dc.t.view(B, n), a + old if acc else a, f"cn_copy_f32 n={n} B={B} acc={acc}")
        dc.assert_canary(f"cn_copy_f32 n={n} B={B} acc={acc}")
    dc = f32_canvas(old, 5, SENT, d)
    L.call("cn_add_f32", ac.ptr, ac.pitch, cc.ptr, cc.pitch, dc.ptr, dc.pitch, B, n, st)
    sync()
    assert_exact(dc.t.view(B, n), a + c, f"cn_add_f32 n={n} B={B}")
    dc.assert_canary(f"cn_add_f32 n={n} B={B}")
    # the engine's add(x, x) backward: source and destination are the same buffer
    dc = f32_canvas(a, 5, SENT, d)
    L.call("cn_copy_f32", dc.ptr, dc.pitch, dc.ptr, dc.pitch, B, n, 1, st)
    sync()
    assert_exact(dc.t.view(B, n), 2 * a, f"cn_copy_f32 in place n={n} B={B}")
    dc.assert_canary(f"cn_copy_f32 in place n={n}")


@pytest.mark.parametrize("n", [1, 1025, 2048 * 1024 + 3])
def test_fill_f32(n):
    d = dev()
    f = Flat((n,), d, fill=SENT)
    lib().call("cn_fill_f32", f.ptr, n, 3.25, stream())
    sync()
    assert bool((f.t == 3.25).all()), f"cn_fill_f32 n={n}"
    f.assert_slack(f"cn_fill_f32 n={n}")
    lib().call("cn_fill_f32", f.ptr, n, 0.0, stream())
    sync()
    assert bool((f.t.view(torch.int32) == 0).all()), f"cn_fill_f32 n={n}: not +0"
    f.assert_slack(f"cn_fill_f32 0 n={n}")


# ---------------------------------------------------------------------------------------------------------------------
# cn_copy_bf16 / cn_add_bf16 / cn_zero_bf16: [P][C] rows with a pitch
# ---------------------------------------------------------------------------------------------------------------------

def rows_canvas(x, P, Cw, ldr, fill, d):
    """bf16 [P][ldr] rows whose first Cw columns are the tensor; x: [P, Cw] or None."""
    data = None if x is None else x.t()[None, :, :, None]
    return Canvas((1, Cw, P, 1), BF, d, pitch=ldr, fill=fill, data=data)


def rows_of(cv, c0, C):
    return cv.t[0, c0:c0 + C, :, 0].t()


def piece_rows(C):
    """P values whose piece counts P * C / 8 hit 1, 255, 256, 257, 511, 512, 513 where C allows it, and otherwise lie
    on both sides of the 256- and 512-piece steps (one block of 256 threads takes two pieces per thread)."""
    C8 = C // 8
    ps = {1}
    for t in (255, 256, 257, 511, 512, 513):
        if t % C8 == 0:
            ps.add(t // C8)
    for t in (256, 512):
        ps.update({max(1, t // C8), t // C8 + 1, max(1, (t - 1) // C8)})
    return sorted(ps)


def test_piece_rows_reach_the_steps():
    assert [p * 1 for p in piece_rows(8)] == [1, 255, 256, 257, 511, 512, 513]
    for C in (24, 64, 480):
        n = [p * C // 8 for p in piece_rows(C)]
        assert min(n) <= 256 < max(n) and any(256 < v <= 512 for v in n) and any(v > 512 for v in n), (C, n)


# lda, ldc, destination width, channel offset of the destination slice, ldd -- all as increments over C
PITCHES = {"dense": (0, 0, 0, 0, 0), "slice": (8, 24, 16, 8, 16), "slice-wide": (24, 0, 16, 8, 40)}


def bf16_ref(op, a, c, old):
    """float64 values of the kernel's result: a copy, or ONE fp32 add rounded to nearest even into bf16."""
    if op == "copy":
        return a.double()
    other = old if op == "accumulate" else c
    return (a.float() + other.float()).to(BF).double()


def run_bcopy(op, a, c, old, C, pitch, d, what):
    P = a.shape[0]
    da, dc_, dw, c0, dd = PITCHES[pitch]
    L, st = lib(), stream()
    ac = rows_canvas(a, P, C, C + da, GARB, d)
    cc = rows_canvas(c, P, C, C + dc_, GARB, d)
    wide = torch.full((P, C + dw), SENT, dtype=torch.float64)
    wide[:, c0:c0 + C] = old
    dst = rows_canvas(wide, P, C + dw, C + dd, SENT, d)
    ptr = dst.ptr + 2 * c0
    if op == "add":
        L.call("cn_add_bf16", ac.ptr, ac.pitch, cc.ptr, cc.pitch, ptr, dst.pitch, P, C, st)
    else:
        L.call("cn_copy_bf16", ac.ptr, ac.pitch, ptr, dst.pitch, P, C, int(op == "accumulate"), st)
    sync()
    assert_exact(rows_of(dst, c0, C), bf16_ref(op, a, c, old), what)
    canary_outside(dst, c0, C, what)


@pytest.mark.parametrize("op", ["copy", "accumulate", "add"])
@pytest.mark.parametrize("pitch", list(PITCHES))
@pytest.mark.parametrize("C", [8, 24, 64, 480])
def test_copy_add_bf16(C, pitch, op):
    d = dev()
    for P in piece_rows(C):
        seed = C + 7 * P
        # integers: sums within +-256 are exact in bf16, the result equals float64
        a, c, old = (ints((P, C), -100, 100, seed + i) for i in range(3))
        assert float(a.abs().max() + c.abs().max()) <= 256 and float(a.abs().max() + old.abs().max()) <= 256
        what = f"cn_{op}_bf16 C={C} P={P} {pitch} integers"
        run_bcopy(op, a, c, old, C, pitch, d, what)
        if op != "copy":
            other = old if op == "accumulate" else c
            assert torch.equal(bf16_ref(op, a, c, old), a + other)
        # random bf16-representable data: the reference restates the fp32 add and the rounding
        a, c, old = (randf((P, C), seed + 10 + i).to(BF).double() for i in range(3))
        run_bcopy(op, a, c, old, C, pitch, d, what.replace("integers", "random"))


@pytest.mark.parametrize("P", [(1 << 20) + 67, 3 * (1 << 19) + 67], ids=["pair-then-tail", "two-pairs-then-tail"])
def test_copy_add_bf16_past_the_block_cap(P):
    """C = 64 past the cap of 16384 blocks, where the stride of the two-piece loop stays 16384 x 256 = 4,194,304 pieces.
    P = 1,048,576 + 67 is 8,389,144 pieces, between 2 and 3 strides: every thread runs the pair loop once and 536
    threads then take the single-piece tail. P = 1,572,864 + 67 is 12,583,448 pieces, just over 3 strides: the first
    536 threads run the pair loop a SECOND time, the others take the tail after one pair (production: a batch-32 cat of
    480 channels at 100 x 100 is 19.2M pieces, two pair iterations). 134 and 201 MB per buffer, so for these cases only
    the data is built on the device (integers in -100..100) and the reference is plain torch on the device: a copy is
    torch.equal to its source, an add is the fp32 sum of two integers within +-256, exact in bf16."""
    d = dev()
    C = 64
    n, stride = P * (C // 8), 16384 * 256
    assert 2 * stride < n < 3 * stride or 3 * stride < n < 4 * stride
    L, st = lib(), stream()
    g = torch.Generator(device=d).manual_seed(3)
    mk = lambda: torch.randint(-100, 101, (P, C), device=d, generator=g).to(BF)
    a, c, old = mk(), mk(), mk()
    t0 = time.time()
    ac = rows_canvas(a, P, C, C + 8, GARB, d)
    cc = rows_canvas(c, P, C, C, GARB, d)
    for op in ("copy", "accumulate", "add"):
        dst = rows_canvas(old, P, C, C + 16, SENT, d)
        if op == "add":
            L.call("cn_add_bf16", ac.ptr, ac.pitch, cc.ptr, cc.pitch, dst.ptr, dst.pitch, P, C, st)
        else:
            L.call("cn_copy_bf16", ac.ptr, ac.pitch, dst.ptr, dst.pitch, P, C, int(op == "accumulate"), st)
        sync()
        ref = a if op == "copy" else (a.float() + (old if op == "accumulate" else c).float()).to(BF)
        got = rows_of(dst, 0, C)
        assert torch.equal(got, ref), f"cn_{op}_bf16 past the cap: {int((got != ref).sum())} elements differ"
        dst.assert_canary(f"cn_{op}_bf16 past the cap")
        del dst
    print(f"TIME bf16 copy/add past the block cap, P={P}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("pitch", [0, 8, 40])
@pytest.mark.parametrize("C", [8, 24, 64, 480])
def test_zero_bf16(C, pitch):
    d = dev()
    for P in piece_rows(C):
        _zero_bf16(C, P, C + pitch, d)


def test_zero_bf16_past_the_block_cap():
    """C = 64, P = 262,144 + 3: 2,097,176 pieces against 8192 blocks x 256 threads."""
    assert ((1 << 18) + 3) * 8 > 8192 * 256
    _zero_bf16(64, (1 << 18) + 3, 72, dev())


def _zero_bf16(C, P, ldr, d):
    cv = rows_canvas(None, P, C, ldr, SENT, d)
    lib().call("cn_zero_bf16", cv.ptr, cv.pitch, P, C, stream())
    sync()
    what = f"cn_zero_bf16 C={C} P={P} ld={ldr}"
    assert bool((rows_of(cv, 0, C).contiguous().view(I16) == 0).all()), f"{what}: not +0 everywhere"
    cv.assert_canary(what)  # columns [C, ld) and the slack still hold the sentinel


# ---------------------------------------------------------------------------------------------------------------------
# converters (64 pixels x 64 channels per tile)
# ---------------------------------------------------------------------------------------------------------------------

HWS = [1, 63, 64, 65, 625]
CPADS = [(3, 8), (5, 16), (63, 64), (64, 64), (65, 72), (130, 136)]
FMAX = torch.finfo(torch.float32).max
SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -0.0, 0.0, 1e-40, -1e-40, 2.0 ** -133, 2.0 ** -134,
            float("inf"), -float("inf"), FMAX, -FMAX, 3.3895313892515355e38, float("nan"), 2.0 ** -126, 1.0000001, 255.5,
            256.5, 257.0]


def test_specials_are_what_they_claim():
    t = torch.tensor(SPECIALS, dtype=F32)
    r = t.to(BF).float()
    assert float(r[0]) == 1.0 and float(r[1]) == 1 + 2.0 ** -6 and float(r[2]) == -1.0  # ties to even, both ways
    assert r[3].view(torch.int32) == -(2 ** 31) and r[4].view(torch.int32) == 0  # -0 stays -0
    assert float(r[5]) != 0 and abs(float(r[5])) < 2.0 ** -126  # an fp32 subnormal becomes a bf16 subnormal
    assert float(r[8]) == 0.0 or float(r[8]) == 2.0 ** -133  # half the smallest bf16 subnormal: a tie
    assert float(r[11]) == float("inf") and float(r[12]) == -float("inf")  # the largest finite fp32 rounds to inf
    assert bool(r[14].isnan())


def _f32_plane(B, C, HW, seed, special):
    x = randf((B, C, HW, 1), seed).float()
    if special:
        flat = x.view(-1)
        s = torch.tensor(SPECIALS, dtype=F32)
        k = min(flat.numel(), s.numel())
        flat[:k] = s[:k]
        if flat.numel() >= 2 * s.numel():
            flat[-s.numel():] = s.flip(0)
    return x


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,Cpad", CPADS)
def test_convert_f32nchw_to_bf16nhwc(C, Cpad, B):
    d, L, st = dev(), lib(), stream()
    for HW in HWS:
        for ldr in (Cpad, Cpad + 8):
            for special in (False, True):
                x = _f32_plane(B, C, HW, C + HW + B, special)
                src = Canvas((B, C, HW, 1), F32, d, pitch=C * HW + 3, fill=GARB)
                src.t.copy_(x.to(d))  # bit for bit (NaN, -0, subnormals)
                dst = Canvas((B, Cpad, HW, 1), BF, d, pitch=ldr)
                L.call("cn_convert_f32nchw_to_bf16nhwc", src.ptr, src.pitch, dst.ptr, dst.pitch, B, C, Cpad, HW, st)
                sync()
                what = f"f32->bf16 C={C} Cpad={Cpad} HW={HW} ld={ldr} B={B} special={special}"
                got = dst.t.cpu().contiguous()
                ref = x.to(BF)  # the CPU's round to nearest even
                nan = ref.isnan()
                assert torch.equal(got[:, :C].isnan(), nan), f"{what}: NaN placement"
                gb = got[:, :C].contiguous().view(I16).masked_fill(nan, 0)
                rb_ = ref.contiguous().view(I16).masked_fill(nan, 0)
                if not torch.equal(gb, rb_):
                    i = tuple((gb != rb_).nonzero()[0].tolist())
                    raise AssertionError(f"{what}: {int((gb != rb_).sum())} elements differ in bits; first at {i}: "
                                         f"x {float(x[i])!r} got {float(got[i])!r} want {float(ref[i])!r}")
                assert bool((got[:, C:].contiguous().view(I16) == 0).all()), f"{what}: padding channels are not +0"
                dst.assert_canary(what)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C,Cpad", CPADS)
def test_convert_bf16nhwc_to_f32nchw(C, Cpad, B):
    d, L, st = dev(), lib(), stream()
    for HW in HWS:
        for ldr in (Cpad, Cpad + 8):
            seed = C + HW + B
            what = f"bf16->f32 C={C} HW={HW} ld={ldr} B={B}"
            # overwrite: random bf16 values arrive bit for bit
            x = randf((B, C, HW, 1), seed).to(BF)
            x.view(-1)[0] = -0.0
            src = Canvas((B, C, HW, 1), BF, d, pitch=ldr, fill=GARB, data=x)
            dst = Canvas((B, C, HW, 1), F32, d, pitch=C * HW + 3)
            L.call("cn_convert_bf16nhwc_to_f32nchw", src.ptr, src.pitch, dst.ptr, dst.pitch, B, C, HW, 0, st)
            sync()
            assert torch.equal(dst.t.cpu().contiguous().view(torch.int32), x.float().view(torch.int32)), what
            dst.assert_canary(what)
            # accumulate into an integer canvas
            xi, old = ints((B, C, HW, 1), -200, 200, seed + 1), ints((B, C, HW, 1), -1000, 1000, seed + 2)
            premise(what, 1200)
            src = Canvas((B, C, HW, 1), BF, d, pitch=ldr, fill=GARB, data=xi)
            dst = Canvas((B, C, HW, 1), F32, d, pitch=C * HW + 3, data=old)
            L.call("cn_convert_bf16nhwc_to_f32nchw", src.ptr, src.pitch, dst.ptr, dst.pitch, B, C, HW, 1, st)
            sync()
            assert_exact(dst.t, xi + old, what + " accumulate")
            dst.assert_canary(what + " accumulate")


# ---------------------------------------------------------------------------------------------------------------------
# cn_channel_sum_bf16
# ---------------------------------------------------------------------------------------------------------------------

sum_rows = R.channel_sum_rows


def test_sum_rows_reach_the_grid_steps():
    assert R.bbn_grid(8 * 85 + 1, 24) == (2, 425, 85) and R.bbn_grid(8 * 85, 24)[0] == 1
    assert R.bbn_grid(73723, 128) == (512, 144, 16) and 73723 > 512 * 8 * 16
    assert R.bbn_grid(9, 2048) == (2, 5, 1)
    assert 256 - 85 * 3 == 1  # C = 24: one idle thread


def _channel_sum(x, old, C, P, what):
    """Two calls on one zero-initialised workspace; returns the results of both and checks tickets and slack."""
    d, L, st = dev(), lib(), stream()
    xc = rows_canvas(x, P, C, C + 8, GARB, d)
    ws = torch.zeros(L.query("cn_bn_workspace_floats_bf16", C), device=d)
    outs = []
    for _ in range(2):
        o = Flat((C,), d, fill=SENT, data=old)
        L.call("cn_channel_sum_bf16", xc.ptr, xc.pitch, P, C, o.ptr, int(old is not None), ws.data_ptr(), st)
        sync()
        o.assert_slack(what)
        assert bool((ws[:64].view(torch.int32) == 0).all()), f"{what}: ticket words are not zero after the call"
        outs.append(o.t.cpu().double())
    assert torch.equal(outs[0], outs[1]), f"{what}: two calls on one workspace differ"
    return outs[0]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("C", [8, 24, 128, 2048])
def test_channel_sum_bf16_exact(C, accumulate):
    """Integers in -3..3: every partial sum is an integer below 2^24, so the result equals float64 whatever the order."""
    for P in sum_rows(C):
        x = ints((P, C), -3, 3, C + P)
        old = ints((C,), -1000, 1000, C + P + 1) if accumulate else None
        premise(f"channel sum C={C} P={P}", 3 * P, 1000)
        what = f"cn_channel_sum_bf16 C={C} P={P} acc={accumulate} integers"
        got = _channel_sum(x, old, C, P, what)
        assert_exact(got, x.sum(0) + (old if accumulate else 0), what)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("C", [8, 24, 128, 2048])
def test_channel_sum_bf16_bounded(C, accumulate):
    """Random bf16 data with a mean: |out - float64 sum| <= D * 2^-24 * sum|x| per channel, plus one rounding of
    |old| + |sum x| when accumulating. D = rows / R + R + 1 (tape_ref.channel_sum_depth): a thread's chain over its
    rows / R pixels, the column sum over the R thread rows and the final cast; the block rows are combined in fp64.
    No floor; tests/test_tape_ref.py shows that a sequential fp32 restatement of the kernel's order passes this bound,
    overwriting and accumulating, and that a sum without its last row fails it."""
    for P in sum_rows(C):
        x = (randf((P, C), C + P) + 0.5).to(BF).double()
        old = randf((C,), C + P + 1, 50.0).float().double() if accumulate else None
        what = f"cn_channel_sum_bf16 C={C} P={P} acc={accumulate} D={R.channel_sum_depth(P, C)}"
        got = _channel_sum(x, old, C, P, what)
        ref = x.sum(0) + (old if accumulate else 0)
        bounded(got, ref, R.channel_sum_bound(x, P, C, old), what)
