"""The neighborhood-attention kernels (cn_na2d.hip; cn_bna_* of cn_bops.hip) and the dropout kernels (cn_dropout_f32,
cn_dropout_bf16) through the C ABI against the float64 references of tests/attention_ref.py: per-element bounds (derived
in that module's docstring, pinned on the CPU by tests/test_attention_ref.py), the dropout masks restated outside the
kernels, shapes at the edges of the window rule and of the launch geometry (attention_ref.NA_CASES). Every tensor a
kernel writes sits in a wider buffer whose padding holds a NaN pattern: it must come back bit for bit, and no output may
hold a NaN (dqkv, which the kernels promise to overwrite, starts as NaN). Each check prints its worst err/bound; run
with -s to read the margins."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import attention_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
PAT32 = 0x7FC0BEEF  # a quiet NaN with a payload, as int32
PAT16 = 0x7FC1      # the same for bf16, as int16
M64 = R.MASK64
STEPS = {"nostep": None, "step0": 0, "step1": 1, "step2p63": (1 << 63) + 5}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------------
# NaN-guarded buffers
# ---------------------------------------------------------------------------------------------------------------------

class Slice32:
    """[B, C, ...] channel slice (offset `lead`) of an fp32 [B, C + extra, ...] buffer filled with the NaN pattern."""

    def __init__(self, shape, data=None, lead=1, extra=3):
        B, C = shape[0], shape[1]
        self.full = torch.empty((B, C + extra) + tuple(shape[2:]), dtype=torch.float32, device=_dev())
        self.full.view(torch.int32).fill_(PAT32)
        self.lead, self.C = lead, C
        self.t = self.full[:, lead:lead + C]
        if data is not None:
            self.t.copy_(data.to(_dev()))
        self.ptr, self.stride = self.t.data_ptr(), self.full.stride(0)

    def intact(self):
        i = self.full.view(torch.int32)
        return bool((i[:, :self.lead] == PAT32).all()) and bool((i[:, self.lead + self.C:] == PAT32).all())

    def get(self):
        return self.t.float().cpu().contiguous()


class Slice16:
    """Logical [B, C, H, W] view of a bf16 NHWC buffer with pixel stride C + extra, channel offset `lead` (both multiples
    of 8, as the engine's slices of concat buffers), padding filled with the NaN pattern."""

    def __init__(self, shape, data=None, lead=8, extra=16):
        B, C, H, W = shape
        self.full = torch.empty((B, H, W, C + extra), dtype=BF, device=_dev())
        self.full.view(torch.int16).fill_(PAT16)
        self.lead, self.C = lead, C
        if data is not None:
            self.full[..., lead:lead + C] = data.permute(0, 2, 3, 1).to(BF).to(_dev())
        self.t = self.full[..., lead:lead + C].permute(0, 3, 1, 2)
        self.ptr, self.stride = self.t.data_ptr(), C + extra

    def intact(self):
        i = self.full.view(torch.int16)
        return bool((i[..., :self.lead] == PAT16).all()) and bool((i[..., self.lead + self.C:] == PAT16).all())

    def get(self):
        return self.t.float().cpu().contiguous()


class Flat32:
    """A dense fp32 tensor between two guard runs of 32 floats."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.flat = torch.empty(n + 64, dtype=torch.float32, device=_dev())
        self.flat.view(torch.int32).fill_(PAT32)
        self.t = self.flat[32:32 + n].view(shape)
        self.ptr, self.n = self.t.data_ptr(), n

    def intact(self):
        i = self.flat.view(torch.int32)
        return bool((i[:32] == PAT32).all()) and bool((i[32 + self.n:] == PAT32).all())

    def get(self):
        return self.t.cpu().clone()


def _step_word(value):
    """None, or the pointer of a device word set to `value` through cn_rng_advance_u64 (kept alive by the caller)."""
    from cultionet_amd import _lib

    if value is None:
        return None, None
    w = torch.zeros(1, dtype=torch.int64, device=_dev())
    _lib.call("cn_rng_advance_u64", w.data_ptr(), 12345, 1, _s())
    _lib.call("cn_rng_advance_u64", w.data_ptr(), value, 1, _s())
    return w, w.data_ptr()


def _na2d(prec, case, qkv, dout, p=0.0, seed=0, step=None, save_attn=True):
    """Forward and backward of one precision's kernels on padded, NaN-guarded buffers -> CPU tensors."""
    from cultionet_amd import _lib

    B, heads, D, H, W, dil = case
    C = heads * D
    S = Slice32 if prec == "f32" else Slice16
    q, g = S((B, 3 * C, H, W), qkv), S((B, C, H, W), dout)
    out, dq = S((B, C, H, W)), S((B, 3 * C, H, W))
    attn, dattn = Flat32((B, heads, 9, H, W)), Flat32((B, heads, 9, H, W))
    word, wp = _step_word(step)
    sfx = "f32" if prec == "f32" else "bf16"
    _lib.call(f"cn_na2d_fwd_{sfx}", q.ptr, q.stride, out.ptr, out.stride, attn.ptr if save_attn else None, B, C, heads, H,
              W, 3, dil, float(p), seed, wp, _s())
    res = {}
    if save_attn:
        _lib.call(f"cn_na2d_bwd_{sfx}", q.ptr, q.stride, g.ptr, g.stride, attn.ptr, dattn.ptr, dq.ptr, dq.stride, B, C,
                  heads, H, W, 3, dil, float(p), seed, wp, _s())
        res.update(attn=attn.get(), dattn=dattn.get(), dqkv=dq.get())
    torch.cuda.synchronize()
    res["out"] = out.get()
    for name, buf in (("qkv", q), ("dout", g), ("out", out), ("dqkv", dq), ("attn", attn), ("dattn", dattn)):
        assert buf.intact(), f"{name}: the padding around the tensor was written"
    return res


@functools.lru_cache(maxsize=None)
def _problem(case, bf16, drop=None, qk_scale=1.0, zero_q=False):
    """Inputs, float64 reference and bounds of one configuration (shared by the tests that need it, never modified)."""
    B, heads, D, H, W, dil = case
    qkv, dout = R.na2d_inputs(case, bf16=bf16, qk_scale=qk_scale)
    if zero_q:
        qkv[:, :heads * D] = 0
    keep = R.na2d_keep(B, heads, H, W, *drop) if drop else None
    ref = R.na2d_reference(qkv, dout, heads, dil, keep=keep)
    bnd = R.na2d_bounds(qkv, dout, heads, dil, ref, keep=keep, bf16=bf16)
    return qkv, dout, keep, ref, bnd


def _check_all(tag, got, ref, bnd):
    for name in ("out", "attn", "dattn", "dqkv"):
        R.within(got[name], ref[name], bnd[name], f"{tag} {name}")


# ---------------------------------------------------------------------------------------------------------------------
# NA2D without dropout
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.NA_CASES))
def test_na2d_f32(name):
    case = R.NA_CASES[name]
    qkv, dout, _, ref, bnd = _problem(case, False)
    _check_all(f"na2d f32 {name}", _na2d("f32", case, qkv, dout), ref, bnd)


@pytest.mark.parametrize("name", R.BF16_NA_CASES)
def test_na2d_bf16(name):
    case = R.NA_CASES[name]
    qkv, dout, _, ref, bnd = _problem(case, True)
    _check_all(f"na2d bf16 {name}", _na2d("bf16", case, qkv, dout), ref, bnd)


def test_na2d_f32_without_saved_probabilities():
    """attn = None (inference): the same `out`, bit for bit, as the run that saves the probabilities."""
    case = R.NA_CASES["d4"]
    qkv, dout, _, ref, bnd = _problem(case, False)
    a = _na2d("f32", case, qkv, dout, save_attn=False)["out"]
    b = _na2d("f32", case, qkv, dout)["out"]
    assert torch.equal(a, b)
    R.within(a, ref["out"], bnd["out"], "na2d f32 d4 attn=None out")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("kind", ["logits60", "q0"])
def test_na2d_softmax_extremes(prec, kind):
    """Logits of +-60 (one-hot probabilities, subnormal tails) and q = 0 (all nine probabilities 1/9)."""
    case = R.NA_CASES["d8"]
    qkv, dout, _, ref, bnd = _problem(case, prec == "bf16", None, 4.5 if kind == "logits60" else 1.0, kind == "q0")
    if kind == "logits60":
        assert float(ref["attn"].max()) > 0.999999 and float(ref["attn"].min()) < 1e-40
    else:
        assert float((ref["attn"] - 1.0 / 9).abs().max()) < 1e-15
    _check_all(f"na2d {prec} {kind}", _na2d(prec, case, qkv, dout), ref, bnd)


# ---------------------------------------------------------------------------------------------------------------------
# attention dropout
# ---------------------------------------------------------------------------------------------------------------------

SEED = M64 - 1000  # seed + counter wraps past 2^64 inside the tensor when the launch has no step pointer


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("step", list(STEPS))
def test_na2d_attention_dropout(prec, p, step):
    case = R.DROP_CASE
    B, heads, D, H, W, dil = case
    C = heads * D
    qkv, dout, keep, ref, bnd = _problem(case, prec == "bf16", (p, SEED, STEPS[step]))
    got = _na2d(prec, case, qkv, dout, p=p, seed=SEED, step=STEPS[step])
    tag = f"na2d {prec} drop {p} {step}"
    # ref["attn"] is the softmax before the mask: _check_all's `attn` line is the check that the kernels save the
    # undropped probabilities (a dropped tap saved as 0 or a kept one scaled by 1 / (1 - p) leaves that bound)
    _check_all(tag, got, ref, bnd)
    # a (pixel, head) whose nine taps all drop is exactly zero forward (out) and backward (dS, dq); any other is not
    dead = (keep == 0).all(dim=-1)  # [B, heads, H, W]
    frac = float(dead.double().mean())
    print(f"{tag}: {frac:.3f} of the (pixel, head) pairs lose all nine taps")
    assert (frac > 0.2) if p == 0.9 else (frac < 0.05)
    rows = dead[:, :, None].expand(B, heads, D, H, W).reshape(B, C, H, W)
    assert bool((got["out"][rows] == 0).all()) and bool((got["dqkv"][:, :C][rows] == 0).all())
    assert bool((got["dattn"][dead[:, :, None].expand(B, heads, 9, H, W)] == 0).all())
    alive = ~dead
    assert bool(((got["out"].reshape(B, heads, D, H, W) != 0).any(dim=2) == alive).all())


# ---------------------------------------------------------------------------------------------------------------------
# cn_dropout_f32 / cn_dropout_bf16
# ---------------------------------------------------------------------------------------------------------------------

def _dropout_case(prec, shape, p, seed, step, channelwise):
    """y = dropout(x) into a NaN-filled destination, then the same launch accumulating into a non-zero one; exact keep
    pattern; kept values one fp32 rounding from x * keep_scale(p) (plus one for the accumulation, plus half a bf16 ulp
    when stored as bf16)."""
    from cultionet_amd import _lib

    B, C, H, W = shape
    L = H * W
    bf16 = prec == "bf16"
    S = Slice16 if bf16 else Slice32
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(B, C, H, W, generator=gen) + 0.5) * (torch.randint(0, 2, (B, C, H, W), generator=gen) * 2 - 1)
    base = torch.randn(B, C, H, W, generator=gen)
    if bf16:
        x, base = x.bfloat16().float(), base.bfloat16().float()
    keep = R.dropout_keep(B, C, L, p, seed, step, channelwise).reshape(B, C, H, W)
    xs, y, acc = S(shape, x), S(shape), S(shape, base)
    word, wp = _step_word(step)
    fn = "cn_dropout_bf16" if bf16 else "cn_dropout_f32"
    cw = 1 if channelwise else 0
    _lib.call(fn, xs.ptr, xs.stride, y.ptr, y.stride, B, C, L, float(p), seed, wp, cw, 0, _s())
    _lib.call(fn, xs.ptr, xs.stride, acc.ptr, acc.stride, B, C, L, float(p), seed, wp, cw, 1, _s())
    torch.cuda.synchronize()
    for name, buf in (("x", xs), ("y", y), ("accumulated", acc)):
        assert buf.intact(), f"{name}: the padding around the tensor was written"
    gy, ga = y.get(), acc.get()
    tag = f"dropout {prec} {'channel' if channelwise else 'element'}wise p={p}"
    assert torch.equal(gy != 0, keep != 0), f"{tag}: keep pattern differs from the restated mask"
    frac = float((keep != 0).double().mean())
    if not channelwise:
        assert abs(frac - (1 - p)) < 4 * (p * (1 - p) / keep.numel()) ** 0.5 + 1e-12, frac
    yr = x.double() * keep
    by = R.U * yr.abs()
    R.within(gy, yr, by + (R.half_ulp16(yr, by) if bf16 else 0.0), f"{tag} y")
    ar = base.double() + yr
    ba = by + R.U * ar.abs()
    R.within(ga, ar, ba + (R.half_ulp16(ar, ba) if bf16 else 0.0), f"{tag} accumulated")


@pytest.mark.parametrize("channelwise", [False, True])
@pytest.mark.parametrize("step", ["nostep", "step2p63"])
def test_dropout_f32(channelwise, step):
    # L = 1030: the launcher starts ceil(L / 1024) = 2 blocks of 256 threads per plane, so 512 threads stride over 1030
    # elements (three rounds, the last one ragged); 12 planes so that channelwise masks have both outcomes
    _dropout_case("f32", (2, 6, 10, 103), 0.3, SEED, STEPS[step], channelwise)


@pytest.mark.parametrize("channelwise", [False, True])
@pytest.mark.parametrize("step", ["nostep", "step1"])
def test_dropout_bf16(channelwise, step):
    # 2 * 99 pixels x 3 groups of 8 channels = 594 lanes: three blocks, the last one ragged
    _dropout_case("bf16", (2, 24, 9, 11), 0.3, SEED, STEPS[step], channelwise)


def test_dropout_bf16_past_the_grid_cap():
    """cn_dropout_bf16 caps its grid at 16384 blocks of 256 lanes, one lane per 8 channels of a pixel: 4 194 304 lanes.
    4 194 304 + 300 pixels of 8 channels (33 556 832 elements) make the first 300 lanes take a second round. The mask is
    restated on the host; the comparison itself runs on the device, for the size."""
    from cultionet_amd import _lib

    dev = _dev()
    P, C, p, seed, step = 16384 * 256 + 300, 8, 0.3, 0xABCDEF12345, 1
    keep = torch.from_numpy(R.kept(R.dropout_index(1, C, P, False), p, seed, step)[0]).to(dev)  # [C, P]
    x, y = Slice16((1, C, 1, P)), Slice16((1, C, 1, P))
    gen = torch.Generator().manual_seed(6)
    x.full[..., x.lead:x.lead + C] = (torch.rand((1, 1, P, C), generator=gen) + 0.5).to(BF).to(dev)
    word, wp = _step_word(step)
    _lib.call("cn_dropout_bf16", x.ptr, x.stride, y.ptr, y.stride, 1, C, P, p, seed, wp, 0, 0, _s())
    torch.cuda.synchronize()
    assert x.intact() and y.intact()
    got = y.t[0, :, 0, :].double()
    assert torch.equal(got != 0, keep), "keep pattern differs from the restated mask"
    yr = x.t[0, :, 0, :].double() * keep * R.keep_scale(p)
    bound = R.U * yr.abs()
    bound = bound + R.half_ulp16(yr, bound)
    err = (got - yr).abs()
    worst = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print(f"dropout bf16 past the grid cap ({P * C} elements) y: worst err/bound {worst:.3f}")
    assert worst <= 1.0
    # the lanes of the second round are pixels 4 194 304 .. 4 194 603
    assert bool(keep[:, 16384 * 256:].any()) and not bool(keep[:, 16384 * 256:].all())


def test_dropout_high_p_and_p_zero():
    _dropout_case("f32", (1, 5, 3, 111), 0.9, 77, None, False)
    _dropout_case("f32", (1, 5, 3, 111), 0.0, 77, 1, False)
    _dropout_case("bf16", (1, 8, 3, 37), 0.9, 77, None, False)


# ---------------------------------------------------------------------------------------------------------------------
# head dimensions the bf16 kernels are not compiled for
# ---------------------------------------------------------------------------------------------------------------------

def _engine_na2d(prec, case, qkv, dout, p=0.0, second=None):
    """E.na2d under a recording tape (after E.begin_rng_step when p > 0) -> out, dqkv on the CPU. second: the inputs of
    another training forward run between this forward and its backward."""
    from cultionet_amd import engine as E

    B, heads, D, H, W, dil = case
    dev = _dev()

    def put(t):
        if prec == "bf16":
            return t.to(dev).to(BF).contiguous(memory_format=torch.channels_last)
        return t.to(dev).contiguous()

    store = E.ParamStore(nn.Linear(1, 1).to(dev))
    with E.using_store(store), E.recording(True) as tape:
        if p > 0:
            E.begin_rng_step(dev)
        x = E.Var(put(qkv), True)
        o = E.na2d(x, heads, 3, dil, attn_drop=p)
        if second is not None:
            E.begin_rng_step(dev)
            E.na2d(E.Var(put(second), True), heads, 3, dil, attn_drop=p)
        o.grad = put(dout)
        tape.backward()
    torch.cuda.synchronize()
    return o.t.float().cpu().contiguous(), x.grad.float().cpu().contiguous()


def test_na2d_bf16_refuses_head_dimension_6_and_the_engine_takes_the_fp32_kernels():
    from cultionet_amd import _lib

    case = (1, 4, 6, 9, 8, 2)
    B, heads, D, H, W, dil = case
    C = heads * D
    qkv, dout, _, ref, bnd = _problem(case, True)
    q, g, out, dq = (Slice16(s, d) for s, d in (((B, 3 * C, H, W), qkv), ((B, C, H, W), dout), ((B, C, H, W), None),
                                                   ((B, 3 * C, H, W), None)))
    attn, dattn = Flat32((B, heads, 9, H, W)), Flat32((B, heads, 9, H, W))
    with pytest.raises(_lib.HipKernelError):
        _lib.call("cn_na2d_fwd_bf16", q.ptr, q.stride, out.ptr, out.stride, attn.ptr, B, C, heads, H, W, 3, dil, 0.0, 0,
                  None, _s())
    with pytest.raises(_lib.HipKernelError):
        _lib.call("cn_na2d_bwd_bf16", q.ptr, q.stride, g.ptr, g.stride, attn.ptr, dattn.ptr, dq.ptr, dq.stride, B, C,
                  heads, H, W, 3, dil, 0.0, 0, None, _s())
    torch.cuda.synchronize()
    assert all(b.intact() for b in (out, dq, attn, dattn))
    eo, edq = _engine_na2d("bf16", case, qkv, dout)
    R.within(eo, ref["out"], bnd["out"], "engine na2d bf16 D=6 out")
    R.within(edq, ref["dqkv"], bnd["dqkv"], "engine na2d bf16 D=6 dqkv")


# ---------------------------------------------------------------------------------------------------------------------
# the engine's seed plumbing: <dy, out> = <dv, v> for whatever mask the step drew
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("second_forward", [False, True])
def test_engine_na2d_backward_redraws_the_forward_mask(prec, second_forward):
    """For a fixed mask `out` is linear in v, so sum(dy * out) = sum(dv * v) when the backward launch hashes with the
    seed and step word of ITS forward (the engine compensates on the host when another training forward has advanced the
    word in between). The slack is the two sides' bounds summed, with every tap kept (attention_ref.na2d_identity_slack).
    In fp32 a mask of any other step word leaves that slack; with the bf16 half ulps in it, it is too wide to tell
    (tests/test_attention_ref.py measures both), so the test below reads the two masks exactly."""
    from cultionet_amd import engine as E

    case = R.DROP_CASE
    B, heads, D, H, W, dil = case
    C = heads * D
    p = 0.3
    bf16 = prec == "bf16"
    qkv, dout, _, ref, bnd = _problem(case, bf16)
    slack = R.na2d_identity_slack(qkv, dout, heads, dil, p, bf16)
    E.manual_seed(20240607)
    other = R.na2d_inputs(case, seed=9, bf16=bf16)[0] if second_forward else None
    out, dq = _engine_na2d(prec, case, qkv, dout, p=p, second=other)
    v, dy = qkv[:, 2 * C:].double(), dout.double()
    lhs, rhs = float((dy * out.double()).sum()), float((dq[:, 2 * C:].double() * v).sum())
    print(f"engine na2d {prec} second_forward={second_forward}: <dy,out> {lhs!r} <dv,v> {rhs!r} "
          f"diff/slack {abs(lhs - rhs) / slack:.3f}")
    # dropout was on: the output differs from the undropped reference far beyond its bound
    assert float(((out.double() - ref["out"]).abs() / bnd["out"]).max()) > 1e3
    assert abs(lhs - rhs) <= slack


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("second_forward", [False, True])
def test_engine_na2d_backward_keeps_the_taps_the_forward_kept(prec, second_forward):
    """The exact form of the check above, still without the seed: on attention_ref.mask_probe's inputs `out` spells the
    taps the forward kept at one query of every (batch, head) and dv is non-zero exactly at the key pixels of the taps
    the backward kept. The two sets must be equal, and dropout must have dropped some taps and kept others."""
    from cultionet_amd import engine as E

    case = R.DROP_CASE
    C = case[1] * case[2]
    p = 0.3
    qkv, dout, _ = R.mask_probe(case)
    E.manual_seed(20240607)
    other = R.na2d_inputs(case, seed=9, bf16=prec == "bf16")[0] if second_forward else None
    out, dq = _engine_na2d(prec, case, qkv, dout, p=p, second=other)
    fwd, bwd = R.probe_taps(case, p, out, dq[:, 2 * C:])
    print(f"engine na2d {prec} second_forward={second_forward}: the forward kept {int(fwd.sum())} of {fwd.numel()} "
          f"probed taps, the backward {int(bwd.sum())}")
    assert 0 < int(fwd.sum()) < fwd.numel()
    assert torch.equal(fwd, bwd)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("channelwise", [False, True])
@pytest.mark.parametrize("second_forward", [False, True])
def test_engine_dropout_backward_redraws_the_forward_mask(prec, channelwise, second_forward):
    """The same identity for E.dropout: y = x * keep, dx = dy * keep, so sum(dy * y) = sum(dx * x). Each side is off by
    one fp32 rounding per element (plus half a bf16 ulp when stored as bf16), bounded with every element kept."""
    from cultionet_amd import engine as E

    dev = _dev()
    B, C, H, W = 2, 16, 9, 11
    p = 0.3
    bf16 = prec == "bf16"
    gen = torch.Generator().manual_seed(11)
    x, dy, x2 = (torch.randn(B, C, H, W, generator=gen) for _ in range(3))
    if bf16:
        x, dy, x2 = (t.bfloat16().float() for t in (x, dy, x2))

    def put(t):
        return t.to(dev).to(BF).contiguous(memory_format=torch.channels_last) if bf16 else t.to(dev).contiguous()

    E.manual_seed(777)
    store = E.ParamStore(nn.Linear(1, 1).to(dev))
    with E.using_store(store), E.recording(True) as tape:
        E.begin_rng_step(dev)
        xv = E.Var(put(x), True)
        yv = E.dropout(xv, p, channelwise, True)
        if second_forward:
            E.begin_rng_step(dev)
            E.dropout(E.Var(put(x2), True), p, channelwise, True)
        yv.grad = put(dy)
        tape.backward()
    torch.cuda.synchronize()
    y, dx = yv.t.float().cpu().double(), xv.grad.float().cpu().double()
    xd, dyd = x.double(), dy.double()
    s = R.keep_scale(p)
    by, bdx = R.U * s * xd.abs(), R.U * s * dyd.abs()
    if bf16:
        by, bdx = by + R.half_ulp16(s * xd, by), bdx + R.half_ulp16(s * dyd, bdx)
    lhs, rhs = float((dyd * y).sum()), float((dx * xd).sum())
    slack = float((dyd.abs() * by).sum() + (xd.abs() * bdx).sum())
    print(f"engine dropout {prec} channelwise={channelwise} second_forward={second_forward}: diff/slack "
          f"{abs(lhs - rhs) / slack:.3f}")
    kept = float((y != 0).double().mean())
    assert 0.0 < kept < 1.0 and torch.equal(y != 0, dx != 0)
    assert abs(lhs - rhs) <= slack
