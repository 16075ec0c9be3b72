"""The optimizer kernels behind --optimizer Adam / SGD / RAdam and gradient_clip_algorithm value (cn_optim_step_f32,
cn_optim_step_seg_f32; Adam with norm clipping through cn_adamw_step_f32) against the float64 rules of
tests/optim_ref.py, which tests/test_optim_ref.py pins to torch.optim. Every kernel step is compared with one reference
step started from the kernel's own state, as tests/test_loss_optim_gpu.py::_adamw_run does for AdamW."""
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -23
GRAD_REL = 1e-5  # the tolerance of tests/test_loss_optim_gpu.py::_adamw_run
N_OPT = 2048 * 1024 + 2053  # past the 2048-block grid cap: the grid-stride loop iterates; not a multiple of 4
EPS = 1e-4


def _f(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _launch(name, mode, p, g, m, v, n, lr, b1, wd, step, scale, sumsq, clip, seg=None):
    """The launches HipTrainer issues for (optimizer, clip mode). seg = (table, nseg, nchunks, step_add)."""
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    s = E._stream()
    kind, b2 = R.KINDS[name], R.BETA2[name]
    wd = wd if R.TAKES_WD[name] else 0.0
    seg_args = () if seg is None else seg[:3]
    sq = None
    if mode == R.CLIP_NORM:
        _lib.call("cn_grad_sumsq_f32" if seg is None else "cn_grad_sumsq_seg_f32", g.data_ptr(), n, *seg_args,
                  sumsq.data_ptr(), s)
        sq = sumsq.data_ptr()
    vp = v.data_ptr() if v is not None else None
    steps = (step,) if seg is None else ()
    tail = (float(scale), sq, float(clip), s)
    head = (p.data_ptr(), g.data_ptr(), m.data_ptr(), vp, n) + (() if seg is None else seg)
    if kind == 0 and mode != R.CLIP_VALUE:
        _lib.call("cn_adamw_step_f32" if seg is None else "cn_adamw_step_seg_f32", *head, float(lr), float(b1), b2, EPS,
                  float(wd), *steps, *tail)
    else:
        _lib.call("cn_optim_step_f32" if seg is None else "cn_optim_step_seg_f32", kind, mode, *head, float(lr),
                  float(b1), b2, EPS, float(wd), *steps, *tail)
    torch.cuda.synchronize()


def _grad(n, gen, gnorm):
    g = torch.randn(n, generator=gen)
    g[torch.rand(n, generator=gen) < 0.1] = 0.0  # exact zeros
    return g * (gnorm / float(g.norm()))


def _compare(what, worst, got, ref, p0, idx=None):
    """got / ref: (p, m, v) after the step (v None for SGD); p0 the parameters before it."""
    sel = (lambda t: t) if idx is None else (lambda t: t[idx])
    pr = sel(ref[0])
    dp = pr - sel(p0)
    # p is stored in fp32: its own rounding (and that of the decay product) is allowed on top of 1e-5 of max|dp|
    perr = ((sel(got[0].cpu().double()) - pr).abs() - 2 * F32_EPS * pr.abs()).clamp(min=0).max()
    items = [("dp", float(perr), float(dp.abs().max())),
             ("m", float((sel(got[1].cpu().double()) - sel(ref[1])).abs().max()), float(sel(ref[1]).abs().max()))]
    if got[2] is not None:
        items.append(("v", float((sel(got[2].cpu().double()) - sel(ref[2])).abs().max()), float(sel(ref[2]).abs().max())))
    for k, err, sc in items:
        r = err / (GRAD_REL * max(sc, 1e-30))
        worst[k] = max(worst.get(k, 0.0), r)
        assert r <= 1.0, f"{what} {k}: err {err:.3e} > {GRAD_REL:.0e} * {sc:.3e}"


def _run(name, n, steps, sched, scale, mode, clip, wd, gnorm, what):
    gen = torch.Generator().manual_seed(1300 + n % 97)
    p = (torch.randn(n, generator=gen) * 0.02).cuda()
    m = torch.zeros(n, device="cuda")
    v = torch.zeros(n, device="cuda") if name != "SGD" else None  # SGD: no second state buffer exists
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    worst = {}
    for t in range(1, steps + 1):
        lr, b1 = sched(t)
        g = _grad(n, gen, gnorm)
        p0, m0 = p.cpu().double(), m.cpu().double()
        v0 = v.cpu().double() if v is not None else torch.zeros(n, dtype=torch.float64)
        if mode == R.CLIP_VALUE:  # some elements beyond the bound, some inside
            beyond = float(((g * _f(scale)).abs() > clip).double().mean())
            assert 0.05 < beyond < 0.95, beyond
        _launch(name, mode, p, g.cuda(), m, v, n, lr, b1, wd, t, scale, sumsq, clip)
        gc = R.clipped(g.double(), _f(scale), mode, clip)  # (the fp32 values the kernel received)
        ref = R.step(name, p0, gc, m0, v0, _f(lr), _f(b1), _f(EPS), _f(wd), t, b2=_f(R.BETA2[name]))
        _compare(f"{what} step {t}", worst, (p, m, v), ref, p0)
    print(f"{what}: worst err/tol " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


# per-element gradient scale of a unit-normal gradient normalised to norm 7 over N_OPT elements (0.9 of them non-zero)
ELEM = 7.0 / (0.9 * N_OPT) ** 0.5

CASES = {
    # id: (grad_scale, clip mode, max_norm / clip_value, weight_decay, norm of the (summed) gradient)
    "norm_clip_active": (1.0, R.CLIP_NORM, 1.0, 1e-3, 7.0),
    "norm_clip_inactive": (1.0, R.CLIP_NORM, 1.0, 0.0, 0.4),
    "value_clip": (1.0, R.CLIP_VALUE, ELEM, 1e-3, 7.0),             # |g| > one sigma is clamped: ~32 % of the elements
    "no_clip": (1.0, R.CLIP_NONE, 0.0, 1e-3, 7.0),
    "scale_half_clip_active": (0.5, R.CLIP_NORM, 1.0, 1e-3, 10.0),   # averaged norm 5: coefficient 0.2
    "scale_eighth_clip_inactive": (0.125, R.CLIP_NORM, 1.0, 0.0, 4.0),  # averaged norm 0.5: no clip
    "scale_eighth_value_clip": (0.125, R.CLIP_VALUE, ELEM, 1e-3, 56.0),  # the bound applies to the AVERAGED gradient
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["SGD", "RAdam", "Adam"])
def test_optimizer_regimes(name, case):
    scale, mode, clip, wd, gnorm = CASES[case]
    _run(name, N_OPT, 3, lambda t: (0.01, 0.9), scale, mode, clip, wd, gnorm, f"{name} {case}")


def test_adamw_value_clip():
    """AdamW itself keeps its own entry point; value clipping is what takes it through the new one."""
    scale, mode, clip, wd, gnorm = CASES["value_clip"]
    _run("AdamW", N_OPT, 3, lambda t: (0.01, 0.9), scale, mode, clip, wd, gnorm, "AdamW value_clip")


@pytest.mark.parametrize("name", ["SGD", "RAdam", "Adam"])
def test_one_cycle_steps(name):
    """12 steps under the project's OneCycleLR ((lr, beta1 / momentum) per step); RAdam crosses its step-5/6 switch."""
    from cultionet_amd.schedules import OneCycleLR

    assert R.radam_rect(5, R.BETA2["RAdam"]) is None and R.radam_rect(6, R.BETA2["RAdam"]) is not None
    _run(name, 300_007, 12, OneCycleLR(max_lr=0.01, total_steps=12), 1.0, R.CLIP_NORM, 1.0, 1e-3, 3.0,
         f"{name} one_cycle")


@pytest.mark.parametrize("name", ["SGD", "RAdam", "Adam"])
def test_no_elements_is_a_no_op(name):
    p = torch.full((8,), 3.0, device="cuda")
    g, m, v = torch.ones(8, device="cuda"), torch.ones(8, device="cuda"), torch.ones(8, device="cuda")
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    for mode in (R.CLIP_NONE, R.CLIP_NORM, R.CLIP_VALUE):
        _launch(name, mode, p, g, m, v, 0, 0.01, 0.9, 1e-3, 1, 1.0, sumsq, 1.0)
    assert bool((p == 3.0).all()) and bool((m == 1.0).all()) and bool((v == 1.0).all())


def test_bad_kind_and_missing_buffers_are_refused():
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    p = torch.zeros(8, device="cuda")
    args = (p.data_ptr(), p.data_ptr(), p.data_ptr())
    rest = (8, 0.01, 0.9, 0.99, EPS, 0.0, 1, 1.0)
    with pytest.raises(_lib.HipKernelError):  # unknown optimizer kind
        _lib.call("cn_optim_step_f32", 3, 0, *args, p.data_ptr(), *rest, None, 0.0, E._stream())
    with pytest.raises(_lib.HipKernelError):  # RAdam without exp_avg_sq
        _lib.call("cn_optim_step_f32", 2, 0, *args, None, *rest, None, 0.0, E._stream())
    with pytest.raises(_lib.HipKernelError):  # norm clipping without the reduced norm
        _lib.call("cn_optim_step_f32", 1, 1, *args, None, *rest, None, 1.0, E._stream())


# ---- segmented ---------------------------------------------------------------------------------------------------------

def _mixed_segments(n, gen):
    """One 300 K run (not aligned to 16 bytes at either end), then many 1-element runs with gaps, every run with its
    own step count (1..11: both RAdam branches)."""
    segs = [(3, 300_001, 7)]
    o, k = 300_010, 0
    while o < n - 20 and len(segs) < 320:
        ln = 1 if k % 5 else [2, 3, 17, 4099][(k // 5) % 4]
        segs.append((o, ln, 1 + (k * 7) % 11))
        o += ln + 1 + int(torch.randint(0, 9, (1,), generator=gen))
        k += 1
    return segs


N_SEG = 420_000

SEG_CASES = {
    "norm_clip_active": (1.0, R.CLIP_NORM, 1.0, 7.0),
    "value_clip": (1.0, R.CLIP_VALUE, 7.0 / (0.9 * N_SEG) ** 0.5, 7.0),
    "no_clip_scaled": (0.5, R.CLIP_NONE, 0.0, 7.0),
}


@pytest.mark.parametrize("case", list(SEG_CASES))
@pytest.mark.parametrize("name", ["SGD", "RAdam", "Adam"])
def test_segmented_step(name, case):
    from cultionet_amd import engine as E

    scale, mode, clip, gnorm = SEG_CASES[case]
    n = N_SEG
    gen = torch.Generator().manual_seed(31 + len(case))
    segs = _mixed_segments(n, gen)
    assert len(segs) >= 300 and sum(1 for _, ln, _ in segs if ln == 1) >= 200
    assert len({st for _, _, st in segs}) >= 10
    p = (torch.randn(n, generator=gen) * 0.02).cuda()
    m = (torch.randn(n, generator=gen) * 1e-3).cuda()
    v = (torch.rand(n, generator=gen) * 1e-5).cuda()
    g = _grad(n, gen, gnorm)
    step_add = 2  # the table holds the steps at its build; the kernel adds the steps taken since
    raw, chunks = E.segment_table([(o, ln, st - step_add) for o, ln, st in segs])
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    p0, m0, v0 = p.cpu().double(), m.cpu().double(), v.cpu().double()
    lr, b1, wd = 3e-3, 0.9, 1e-3
    _launch(name, mode, p, g.cuda(), m, v, n, lr, b1, wd, None, scale, sumsq, clip,
            seg=(table.data_ptr(), len(segs), chunks, step_add))
    idx = torch.cat([torch.arange(o, o + ln) for o, ln, _ in segs])
    gc = R.clipped(g.double(), _f(scale), mode, clip, norm_of=lambda t: t[idx])
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    for o, ln, st in segs:
        sl = slice(o, o + ln)
        pr[sl], mr[sl], vr[sl] = R.step(name, p0[sl], gc[sl], m0[sl], v0[sl], _f(lr), _f(b1), _f(EPS), _f(wd), st,
                                        b2=_f(R.BETA2[name]))
    out = torch.ones(n, dtype=torch.bool)
    out[idx] = False
    # outside the segments nothing moves, bit for bit (SGD: exp_avg_sq nowhere)
    assert torch.equal(p.cpu()[out], p0.float()[out]) and torch.equal(m.cpu()[out], m0.float()[out])
    assert torch.equal(v.cpu()[out], v0.float()[out])
    if name == "SGD":
        assert torch.equal(v.cpu(), v0.float())
    worst = {}
    _compare(f"{name} {case}", worst, (p, m, v if name != "SGD" else None), (pr, mr, vr), p0, idx)
    print(f"segmented {name} {case}: worst err/tol " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))
