"""The loss-scaler step kernel (cn_optim_step_amp_f32, cn_amp_count_skip) against the float64 rules of tests/optim_ref.py,
and cultionet_amd.optim.NativeOptimizer as the optimizer of the Lightning route and as the state of HipTrainer: in-place
gradient, equivalence with the native route, state_dict interop with torch.optim both ways, GradScaler, schedulers, the
clipping hook and resume.

Kernel checks use tests/test_optim_kinds_gpu.py as it stands: one reference step started from the kernel's own state,
GRAD_REL = 1e-5 with the two-ulp rule (``_compare``), and its ``_grad`` recipe."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import optim_ref as R
from test_optim_kinds_gpu import EPS, F32_EPS, GRAD_REL, _compare, _f, _grad

pytestmark = pytest.mark.gpu

TORCH_VS_RULE = 1e-14  # torch.optim against the float64 rule: the bound of tests/test_optim_ref.py
KINDS = ["Adam", "AdamW", "RAdam", "SGD"]
LOSS_SCALE = 1024.0

# ---- kernel ------------------------------------------------------------------------------------------------------------

N_BIG = 2048 * 4096 + 4096 + 5  # one segment: 2050 chunks pass the 2048-block cap (the chunk loop iterates); tail of 5


def _short_segments(gen):
    """~300 runs of 1..9 elements at odd offsets with gaps (unaligned heads and tails), every run its own step count
    (1..11: both RAdam branches), as tests/test_optim_kinds_gpu.py::_mixed_segments builds its short runs."""
    segs, o = [], 3
    for k in range(300):
        ln = 1 + k % 9
        segs.append((o, ln, 1 + (k * 7) % 11))
        o += ln + 1 + 2 * int(torch.randint(0, 4, (1,), generator=gen))  # odd and even starts
    return segs, o + 8


def _shape(which, gen):
    if which == "one_long":
        return [(0, N_BIG, 7)], N_BIG
    return _short_segments(gen)


def _word(value, dtype=torch.float32):
    return torch.tensor([value], dtype=dtype, device="cuda")


def _amp_launch(name, mode, p, g, m, v, n, table, nseg, chunks, step_add, lr, b1, wd, scale, sumsq, clip, loss_scale=None,
                found_inf=None, skipped=None, entry="cn_optim_step_amp_f32"):
    """sum of squares over the (still scaled) gradient when norm clipping, the step, the skip counter."""
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    s = E._stream()
    kind, b2 = R.KINDS[name], R.BETA2[name]
    wd = wd if R.TAKES_WD[name] else 0.0
    sq = None
    if mode == R.CLIP_NORM:
        _lib.call("cn_grad_sumsq_seg_f32", g.data_ptr(), n, table.data_ptr(), nseg, chunks, sumsq.data_ptr(), s)
        sq = sumsq.data_ptr()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    words = (ptr(loss_scale), ptr(found_inf), ptr(skipped)) if entry == "cn_optim_step_amp_f32" else ()
    _lib.call(entry, kind, mode, p.data_ptr(), g.data_ptr(), m.data_ptr(), ptr(v), n, table.data_ptr(), nseg, chunks,
              step_add, float(lr), float(b1), b2, EPS, float(wd), float(scale), *words, sq, float(clip), s)
    if found_inf is not None:
        _lib.call("cn_amp_count_skip", found_inf.data_ptr(), skipped.data_ptr(), s)
    torch.cuda.synchronize()


def _state(n, gen):
    return ((torch.randn(n, generator=gen) * 0.02).cuda(), (torch.randn(n, generator=gen) * 1e-3).cuda(),
            (torch.rand(n, generator=gen) * 1e-5).cuda())


def _table(segs, step_add):
    from cultionet_amd import engine as E

    raw, chunks = E.segment_table([(o, ln, st - step_add) for o, ln, st in segs])
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda(), chunks


def _reference(name, segs, idx, p0, m0, v0, g, scale, mode, clip, lr, b1, wd, t_of=lambda st: st):
    gc = R.clipped(g.double(), _f(scale), mode, clip, norm_of=lambda t: t[idx])
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    for o, ln, st in segs:
        sl = slice(o, o + ln)
        pr[sl], mr[sl], vr[sl] = R.step(name, p0[sl], gc[sl], m0[sl], v0[sl], _f(lr), _f(b1), _f(EPS), _f(wd), t_of(st),
                                        b2=_f(R.BETA2[name]))
    return pr, mr, vr


# id: (grad_scale, clip mode, bound (None: one sigma of the averaged gradient), weight_decay, norm of the gradient)
REGIMES = {
    "scaled_norm_clip_active": (1.0, R.CLIP_NORM, 1.0, 1e-3, 7.0),
    "scaled_norm_clip_inactive": (1.0, R.CLIP_NORM, 1.0, 0.0, 0.4),
    "scaled_value_clip": (1.0, R.CLIP_VALUE, None, 1e-3, 7.0),
    "grad_scale_half": (0.5, R.CLIP_NORM, 1.0, 1e-3, 10.0),  # averaged norm 5: coefficient 0.2
}


@pytest.mark.parametrize("which", ["one_long", "short_runs"])
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("name", KINDS)
def test_amp_step_matches_float64(name, regime, which):
    """loss_scale 1024 and the gradient pre-multiplied by 1024 (exact in fp32): the reference sees g."""
    scale, mode, clip, wd, gnorm = REGIMES[regime]
    gen = torch.Generator().manual_seed(500 + len(regime) + len(which))
    segs, n = _shape(which, gen)
    idx = torch.cat([torch.arange(o, o + ln) for o, ln, _ in segs])
    p, m, v = _state(n, gen)
    g = _grad(n, gen, gnorm)
    g = g * (gnorm / float(g[idx].norm()))  # the norm of what the segments hold
    if clip is None:
        clip = scale * gnorm / (0.9 * idx.numel()) ** 0.5  # |g| beyond one sigma is clamped
        beyond = float(((g[idx] * _f(scale)).abs() > clip).double().mean())
        assert 0.05 < beyond < 0.95, beyond
    step_add = 2
    table, chunks = _table(segs, step_add)
    if which == "one_long":
        assert chunks > 2048 and n % 4 != 0
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    p0, m0, v0 = p.cpu().double(), m.cpu().double(), v.cpu().double()
    lr, b1 = 3e-3, 0.9
    skipped = _word(0, torch.int32)
    _amp_launch(name, mode, p, (g * LOSS_SCALE).cuda(), m, v if name != "SGD" else None, n, table, len(segs), chunks,
                step_add, lr, b1, wd, scale, sumsq, clip, loss_scale=_word(LOSS_SCALE), found_inf=_word(0.0),
                skipped=skipped)
    assert int(skipped.item()) == 0
    ref = _reference(name, segs, idx, p0, m0, v0, g, scale, mode, clip, lr, b1, wd)
    out = torch.ones(n, dtype=torch.bool)
    out[idx] = False
    assert torch.equal(p.cpu()[out], p0.float()[out]) and torch.equal(m.cpu()[out], m0.float()[out])
    assert torch.equal(v.cpu()[out], v0.float()[out])
    worst = {}
    _compare(f"{name} {regime} {which}", worst, (p, m, v if name != "SGD" else None), ref, p0, idx)
    print(f"amp {name} {regime} {which}: worst err/tol " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("name", KINDS)
def test_found_inf_skips_and_the_next_step_counts_one_less(name):
    """found_inf = 1: p, m, v keep their bits and ``skipped`` goes 0 -> 1; the next step (host count t) matches the
    reference at t - 1. The long run holds step 4: the skipped step is host count 5, the next one host count 6 =
    effective 5 (RAdam not yet rectified), the one after host count 7 = effective 6 (rectified): the switch is crossed
    one step later."""
    b2 = R.BETA2["RAdam"]
    assert R.radam_rect(5, b2) is None and R.radam_rect(6, b2) is not None
    gen = torch.Generator().manual_seed(77)
    short, end = _short_segments(gen)
    segs = short + [(end + 1, 9001, 4)]  # (counts at the table's build; a 9001-element run: three chunks, odd start)
    n = end + 1 + 9001 + 6
    idx = torch.cat([torch.arange(o, o + ln) for o, ln, _ in segs])
    p, m, v = _state(n, gen)
    vv = v if name != "SGD" else None
    table, chunks = _table(segs, 0)
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    skipped, scale_word = _word(0, torch.int32), _word(LOSS_SCALE)
    lr, b1, wd = 3e-3, 0.9, 1e-3
    before = (p.clone(), m.clone(), v.clone())
    g = _grad(n, gen, 7.0)
    g[idx[5]] = float("inf")
    _amp_launch(name, R.CLIP_NORM, p, (g * LOSS_SCALE).cuda(), m, vv, n, table, len(segs), chunks, 1, lr, b1, wd, 1.0,
                sumsq, 1.0, loss_scale=scale_word, found_inf=_word(1.0), skipped=skipped)
    assert torch.equal(p, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2])
    assert int(skipped.item()) == 1
    worst = {}
    for step_add in (2, 3):  # host counts st + 2, st + 3; effective st + 1, st + 2
        g = _grad(n, gen, 7.0)
        p0, m0, v0 = p.cpu().double(), m.cpu().double(), v.cpu().double()
        _amp_launch(name, R.CLIP_NORM, p, (g * LOSS_SCALE).cuda(), m, vv, n, table, len(segs), chunks, step_add, lr, b1,
                    wd, 1.0, sumsq, 1.0, loss_scale=scale_word, found_inf=_word(0.0), skipped=skipped)
        assert int(skipped.item()) == 1  # (counts only the steps that were skipped)
        ref = _reference(name, segs, idx, p0, m0, v0, g, 1.0, R.CLIP_NORM, 1.0, lr, b1, wd,
                         t_of=lambda st, a=step_add: st + a - 1)
        _compare(f"{name} after a skipped step, step_add {step_add}", worst, (p, m, vv), ref, p0, idx)
    print(f"skip {name}: worst err/tol " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


@pytest.mark.parametrize("which", ["one_long", "short_runs"])
@pytest.mark.parametrize("name", KINDS)
def test_null_words_are_the_plain_segmented_step(name, which):
    gen = torch.Generator().manual_seed(91)
    segs, n = _shape(which, gen)
    state = _state(n, gen)
    g = _grad(n, gen, 7.0).cuda()
    table, chunks = _table(segs, 1)
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    got = []
    for entry in ("cn_optim_step_seg_f32", "cn_optim_step_amp_f32"):
        p, m, v = (t.clone() for t in state)
        _amp_launch(name, R.CLIP_NORM, p, g, m, v if name != "SGD" else None, n, table, len(segs), chunks, 1, 3e-3, 0.9,
                    1e-3, 0.5, sumsq, 1.0, entry=entry)
        got.append((p, m, v))
    assert not torch.equal(got[0][0], state[0])
    for a, b in zip(*got):
        assert torch.equal(a, b)


# ---- the optimizer object ----------------------------------------------------------------------------------------------

KW = dict(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0)
CONSTANT = dict(lr_scheduler="StepLR", steplr_step_size=1000)  # a constant rate through the real scheduler path
VALUE_CLIP = 1e-4  # (tests/test_optim_train_gpu.py: clamps some elements of this model's gradient and spares others)


def _lit(**kw):
    from cultionet_amd import synthetic as S
    from cultionet_amd.lightning import CultionetLitModel

    lit = CultionetLitModel(**KW, **{**CONSTANT, **kw})
    mm = lit.cultionet_model.mask_model
    mm.load_state_dict(S.seeded_state_dict(mm.state_dict()))
    return lit.to("cuda:0").train()


@pytest.fixture(scope="module")
def batch(golden_dir):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data

    hidden, B, H, W, with_mask, seed = (int(v) for v in np.load(os.path.join(golden_dir, "train_h8_b2_28.npz"))["meta"])
    assert hidden == KW["hidden_channels"]
    x, y, bd = S.seeded_batch(B, height=H, width=W, seed=seed, with_mask=bool(with_mask))
    return Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())


def _batches(n):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data

    out = []
    for k in range(n):
        x, y, bd = S.seeded_batch(2, height=28, width=28, seed=70 + k, with_mask=True)
        out.append(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()))
    return out


def _configure(lit, native, total_steps=12):
    lit.native_optimizer = native
    lit.__dict__["trainer"] = types.SimpleNamespace(max_epochs=1, estimated_stepping_batches=total_steps)
    try:
        out = lit.configure_optimizers()
    except (AttributeError, RuntimeError):  # a LightningModule base that guards `.trainer`
        lit._trainer = lit.__dict__.pop("trainer")
        out = lit.configure_optimizers()
    return out["optimizer"], out["lr_scheduler"]["scheduler"]


def _backward(lit, batch, scaler=None):
    loss, _ = lit.calc_loss(batch, lit(batch))
    (loss if scaler is None else scaler.scale(loss)).backward()


def _params(lit):
    return list(lit.cultionet_model.parameters())


def _store(lit):
    return lit.cultionet_model.mask_model.param_store()


def _give_grads(dst, src):
    """dst's parameters get clones of src's gradients (None where src has none)."""
    for pd, ps in zip(_params(dst), _params(src)):
        pd.grad = None if ps.grad is None else ps.grad.clone()


def _freeze_final_a(lit):
    frozen = 0
    for n, p in lit.cultionet_model.mask_model.named_parameters():
        if n.startswith("final_a."):
            p.requires_grad_(False)
            frozen += 1
    assert frozen > 0


def _flat_state(opt):
    return [opt.exp_avg] + ([opt.exp_avg_sq] if opt.exp_avg_sq is not None else [])


def test_step_runs_on_autograds_buffer_in_place(batch):
    """After a drop-in backward the step must not copy the gradient: the fast path is taken and store.flat_grad is not
    written. With the gradients replaced by clones the gather path is taken, with the same bits as a result."""
    from cultionet_amd.optim import NativeOptimizer

    a, b = _lit(), _lit()
    oa, ob = _configure(a, True)[0], _configure(b, True)[0]
    assert type(oa) is NativeOptimizer and oa.kind == "AdamW"
    oa.set_clip(1.0, "norm"), ob.set_clip(1.0, "norm")
    _backward(a, batch)
    sa, sb = _store(a), _store(b)
    base = {p.grad.data_ptr() - 4 * o for p, o in zip(sa.params, sa.offsets)}
    assert len(base) == 1 and sa.flat_grad.data_ptr() not in base  # one buffer, handed over whole; the store has a new one
    _give_grads(b, a)
    sa.flat_grad.fill_(123.0)
    grads = [p.grad.clone() for p in sa.params]
    p_before = sa.flat.clone()
    oa.step()
    ob.step()
    torch.cuda.synchronize()
    assert oa.in_place and not ob.in_place
    assert bool((sa.flat_grad == 123.0).all())                                    # not written
    assert all(torch.equal(p.grad, g) for p, g in zip(sa.params, grads))           # nor the gradient
    assert not torch.equal(sa.flat, p_before)
    assert torch.equal(sa.flat, sb.flat)
    for x, y in zip(_flat_state(oa), _flat_state(ob)):
        assert torch.equal(x, y)
    assert sa._sig == sa._signature() and sa.version > 0


CLIPS = {"norm": (1.0, "norm"), "value": (VALUE_CLIP, "value"), "none": (None, "norm")}


# every kind under every clip mode on the whole model; a frozen subset (final_a) under norm clipping for every kind
SAME_BITS = [(n, c, False) for n in KINDS for c in CLIPS] + [(n, "norm", True) for n in KINDS]


@pytest.mark.parametrize("name,clip,frozen", SAME_BITS)
def test_same_bits_as_the_native_route(batch, name, clip, frozen):
    """Given the same flat gradient, NativeOptimizer.step() and HipTrainer.optimizer_step() leave store.flat, exp_avg
    and exp_avg_sq equal bit for bit (two steps: the second one runs on a segment table built a step earlier)."""
    from cultionet_amd.lightning import HipTrainer

    a, b = _lit(optimizer=name), _lit(optimizer=name)
    if frozen:
        _freeze_final_a(a), _freeze_final_a(b)
    clip_val, algorithm = CLIPS[clip]
    trainer = HipTrainer(a, gradient_clip_val=clip_val, gradient_clip_algorithm=algorithm)
    ob = _configure(b, True)[0]
    b.configure_gradient_clipping(ob, clip_val, algorithm)
    sa, sb = _store(a), _store(b)
    assert sa.offsets == sb.offsets
    for k in range(2):
        trainer.forward_backward(batch)
        flat = sa.flat_grad.clone()
        for p, o in zip(sb.params, sb.offsets):  # views of one buffer at the store's offsets, set by hand
            p.grad = flat[o:o + p.numel()].view(p.shape) if p.requires_grad else None
        trainer.optimizer_step()
        ob.step()
        torch.cuda.synchronize()
        assert ob.in_place
        assert torch.equal(sa.flat, sb.flat), (name, clip, k)
        assert torch.equal(trainer.exp_avg, ob.exp_avg)
        if name != "SGD":
            assert torch.equal(trainer.exp_avg_sq, ob.exp_avg_sq)
    assert trainer.param_steps == ob.param_steps
    assert float(trainer.exp_avg.abs().max()) > 0


def _within_both_tolerances(pa, pb, p_before, what):
    """|pa - pb| within torch-vs-rule (tests/test_optim_ref.py) + kernel-vs-rule (GRAD_REL of max |dp| and the two-ulp
    rule of tests/test_optim_kinds_gpu.py), pb the torch optimizer's result."""
    pa, pb, p0 = pa.double().cpu(), pb.double().cpu(), p_before.double().cpu()
    err = float(((pa - pb).abs() - 2 * F32_EPS * pb.abs()).clamp(min=0).max())
    bound = GRAD_REL * float((pb - p0).abs().max()) + TORCH_VS_RULE
    print(f"{what}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _cat(tensors):
    return torch.cat([t.detach().flatten() for t in tensors])


def _state_equal(sd_a, sd_b):
    assert sd_a["state"].keys() == sd_b["state"].keys() and len(sd_a["state"]) > 0
    for i, st in sd_a["state"].items():
        assert st.keys() == sd_b["state"][i].keys(), i
        for k, t in st.items():
            u = sd_b["state"][i][k]
            assert t.dtype == u.dtype and t.shape == u.shape, (i, k)
            assert torch.equal(t.cpu(), u.cpu()), (i, k)
    ga, gb = dict(sd_a["param_groups"][0]), dict(sd_b["param_groups"][0])
    assert ga == gb


@pytest.mark.parametrize("name", KINDS)
def test_state_dict_interop_with_torch_both_ways(batch, name):
    a, b = _lit(optimizer=name), _lit(optimizer=name)
    oa, ob = _configure(a, True)[0], _configure(b, False)[0]
    assert type(ob) is getattr(torch.optim, name)
    for _ in range(3):
        oa.zero_grad(set_to_none=True)
        _backward(a, batch)
        _give_grads(b, a)
        oa.step()
        ob.step()
    # torch -> native
    sd_t = copy.deepcopy(ob.state_dict())
    oa.load_state_dict(sd_t)
    _state_equal(oa.state_dict(), sd_t)
    if name != "SGD":
        assert oa.param_steps == [3] * len(_params(a))
    # native -> torch (a fresh torch optimizer over b's parameters)
    fresh = _configure(b, False)[0]
    fresh.load_state_dict(copy.deepcopy(oa.state_dict()))  # (a copy: torch's load keeps same-device tensors as they are)
    _state_equal(fresh.state_dict(), oa.state_dict())
    # one more step from the identical state
    with torch.no_grad():
        torch._foreach_copy_(_params(a), [p.detach() for p in _params(b)])
    oa.zero_grad(set_to_none=True)
    _backward(a, batch)
    _give_grads(b, a)
    before = _cat(_params(b)).clone()
    oa.step()
    fresh.step()
    torch.cuda.synchronize()
    assert not torch.equal(_cat(_params(b)), before)
    _within_both_tolerances(_cat(_params(a)), _cat(_params(b)), before, f"{name} step 4 after interop")
    sd_a, sd_f = oa.state_dict(), fresh.state_dict()
    if name != "SGD":
        assert all(float(sd_a["state"][i]["step"]) == float(sd_f["state"][i]["step"]) == 4.0 for i in sd_a["state"])


def _copy_state_from_torch(native, stock, lit_native, lit_stock):
    """Parameters and moments of the native side <- the torch side, bit for bit; the step counts stay the native
    optimizer's own."""
    with torch.no_grad():
        torch._foreach_copy_(_params(lit_native), [p.detach() for p in _params(lit_stock)])
        for pn, ps in zip(_params(lit_native), _params(lit_stock)):
            for k in ("exp_avg", "exp_avg_sq"):
                native.state[pn][k].copy_(stock.state[ps][k])


def test_gradscaler_skips_without_host_sync_and_counts_like_torch(batch):
    """GradScaler(init_scale=1024, growth_interval=2) drives native and stock AdamW on the same scaled gradients for 6
    steps with an inf at step 3: both skip it, both scales halve, the step counts agree in the end, and every step, taken
    from equal state, agrees within the two tolerances."""
    a, b = _lit(), _lit()
    oa, ob = _configure(a, True)[0], _configure(b, False)[0]
    sc_a = torch.amp.GradScaler("cuda", init_scale=1024, growth_interval=2)
    sc_b = torch.amp.GradScaler("cuda", init_scale=1024, growth_interval=2)
    scales = []
    for k in range(1, 7):
        oa.zero_grad(set_to_none=True)
        _backward(a, batch, sc_a)
        sc_b.scale(torch.zeros((), device="cuda"))  # (the stock side's scaler sees its gradients ready-made)
        scale = sc_a.get_scale()
        assert scale == sc_b.get_scale()
        if k == 1:  # a bound the clip is active under: half the norm of the first (unscaled) gradient
            clip = float(torch.linalg.vector_norm(_cat([p.grad for p in _params(a)]).double())) / scale / 2
            a.configure_gradient_clipping(oa, clip, "norm")
        if k == 3:
            _params(a)[0].grad.view(-1)[0] = float("inf")
        _give_grads(b, a)
        before = _cat(_params(b)).clone()
        before_a = _store(a).flat.clone()
        m_before = oa.exp_avg.clone()
        sc_a.step(oa)
        sc_a.update()
        assert oa.in_place
        # the stock side as Lightning runs it: unscale, clip, step
        sc_b.unscale_(ob)
        if k != 3:
            torch.nn.utils.clip_grad_norm_(_params(b), clip)
        sc_b.step(ob)
        sc_b.update()
        torch.cuda.synchronize()
        scales.append((scale, sc_a.get_scale(), sc_b.get_scale()))
        if k == 3:
            assert torch.equal(_store(a).flat, before_a) and torch.equal(oa.exp_avg, m_before)
            assert torch.equal(_cat(_params(b)), before)
            assert sc_a.get_scale() == sc_b.get_scale() == scale / 2
        else:
            assert not torch.equal(_cat(_params(b)), before)
            _within_both_tolerances(_cat(_params(a)), _cat(_params(b)), before, f"scaler step {k}")
            _copy_state_from_torch(oa, ob, a, b)
    print("scales (before, native after, torch after):", scales)
    assert scales[0][0] == 1024.0 and scales[2][0] == 2048.0 and scales[2][1] == 1024.0
    assert int(oa.skipped.item()) == 1 and oa.step_count == 6
    sd_a, sd_b = oa.state_dict(), ob.state_dict()
    assert int(oa.skipped.item()) == 0 and oa.step_count == 5  # folded at state_dict()
    assert sd_a["state"].keys() == sd_b["state"].keys()
    for i in sd_a["state"]:
        assert float(sd_a["state"][i]["step"]) == float(sd_b["state"][i]["step"]) == 5.0, i


def test_gradscaler_step_raises_nothing_under_sync_debug_mode(batch):
    a = _lit()
    oa = _configure(a, True)[0]
    oa.set_clip(1.0, "norm")
    scaler = torch.amp.GradScaler("cuda", init_scale=1024, growth_interval=2)
    for _ in range(2):  # (the segment table is built and uploaded at the first step)
        oa.zero_grad(set_to_none=True)
        _backward(a, batch, scaler)
        scaler.step(oa)
        scaler.update()
    oa.zero_grad(set_to_none=True)
    _backward(a, batch, scaler)
    torch.cuda.synchronize()
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            enforced = False
        except RuntimeError:
            enforced = True
        if enforced:
            scaler.step(oa)  # a host synchronisation in here raises
            scaler.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not enforced:
        pytest.skip("the installed torch does not enforce set_sync_debug_mode('error') on this device")
    assert oa.in_place and oa.step_count == 3


def test_one_cycle_steers_the_launches(batch, monkeypatch):
    """OneCycleLR over 12 steps on the native optimizer: the (lr, beta1) the step launches received equal
    cultionet_amd.schedules.OneCycleLR(step) to fp32 rounding."""
    from cultionet_amd import _lib
    from cultionet_amd.schedules import OneCycleLR

    a = _lit(lr_scheduler="OneCycleLR", learning_rate=0.01)
    oa, sched = _configure(a, True, total_steps=12)
    assert type(sched) is torch.optim.lr_scheduler.OneCycleLR and sched.total_steps == 12
    oa.set_clip(1.0, "norm")
    _backward(a, batch)
    seen, call = [], _lib.call

    def spy(name, *args):
        if name == "cn_adamw_step_f32":  # (p, g, m, v, n, lr, beta1, ...)
            seen.append((args[5], args[6]))
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    for _ in range(12):
        oa.step()
        sched.step()
    monkeypatch.undo()
    mine = OneCycleLR(0.01, 12)
    assert len(seen) == 12
    for k, (lr, b1) in enumerate(seen, start=1):
        want_lr, want_b1 = mine(k)
        assert abs(_f(lr) - _f(want_lr)) <= F32_EPS * abs(want_lr), (k, lr, want_lr)
        assert abs(_f(b1) - _f(want_b1)) <= F32_EPS * abs(want_b1), (k, b1, want_b1)
    assert len({lr for lr, _ in seen}) == 12 and len({b1 for _, b1 in seen}) > 6


def test_clipping_hook_sets_the_fused_clip_and_touches_no_gradient(batch):
    a, b = _lit(), _lit()
    oa, ob = _configure(a, True)[0], _configure(b, False)[0]
    _backward(a, batch)
    _give_grads(b, a)
    grads = [p.grad.clone() for p in _params(a)]
    a.configure_gradient_clipping(oa, 1.0, "norm")
    assert (oa.clip, oa.clip_algorithm) == (1.0, "norm")
    assert all(torch.equal(p.grad, g) for p, g in zip(_params(a), grads))
    norm = float(torch.linalg.vector_norm(_cat(grads).double()))
    assert norm > 0
    b.configure_gradient_clipping(ob, norm / 2, "norm")  # a stock optimizer: the base class clips the gradients themselves
    clipped = float(torch.linalg.vector_norm(_cat([p.grad for p in _params(b)]).double()))
    assert abs(clipped - norm / 2) <= 1e-4 * norm, (clipped, norm)


# ---- resume ----------------------------------------------------------------------------------------------------------------

def _train(lit, trainer, batches):
    for bt in batches:
        trainer.training_step(bt)
    torch.cuda.synchronize()
    return _store(lit).flat.clone()


@pytest.mark.parametrize("mode", ["eager", "replay", "accumulate2"])
def test_resume_continues_the_run(mode):
    """HipTrainer: 4 steps, state_dict(), 3 more steps -> A. A fresh model loaded from the module's step-4 state_dict and
    the trainer's state_dict, run on the same 3 batches -> B. Dropout 0, fixed batches, OneCycleLR (the schedule must
    resume from step_count). A and B agree within twice the run-to-run spread of A itself (the split-K atomics of the
    backward are not ordered), measured here by running A twice; a spread of zero requires equality.

    Measured on MI355X (hidden 8, batch 2, 28 x 28, max |dp| over the flat buffer after 7 steps): run-to-run spread
    4.8e-07 eager, 2.9e-07 replay, 3.9e-07 with accumulate_grad_batches=2; resumed against straight 1.2e-07 in all three,
    and the same for the trainer reloaded in place under its recorded plans."""
    from cultionet_amd.lightning import HipTrainer

    kw = dict(total_steps=20, replay=(mode == "replay"), accumulate_grad_batches=2 if mode == "accumulate2" else 1)
    per = kw["accumulate_grad_batches"]
    batches = _batches(3)
    head = [batches[k % 3] for k in range(4 * per)]
    tail = [batches[(k + 1) % 3] for k in range(3 * per)]

    def run_a():
        lit = _lit(lr_scheduler="OneCycleLR")
        tr = HipTrainer(lit, **kw)
        _train(lit, tr, head)
        module_sd = copy.deepcopy(lit.state_dict())
        sd = tr.state_dict()
        return lit, tr, module_sd, sd, _train(lit, tr, tail)

    lit_a, tr_a, module_sd, sd, flat_a = run_a()
    *_, flat_a2 = run_a()
    spread = float((flat_a - flat_a2).abs().max())
    assert sd["step_count"] == 4 and sd["micro"] == 0 and sd["param_steps"] == [4] * len(_store(lit_a).params)
    assert set(sd) == {"optimizer", "step_count", "micro", "param_steps"}
    assert all(float(st["step"]) == 4.0 for st in sd["optimizer"]["state"].values())

    lit_b = _lit(lr_scheduler="OneCycleLR")
    lit_b.load_state_dict(module_sd)
    tr_b = HipTrainer(lit_b, **kw)
    tr_b.load_state_dict(sd)
    assert tr_b.step_count == 4
    flat_b = _train(lit_b, tr_b, tail)
    assert tr_b.step_count == tr_a.step_count == 7
    err = float((flat_a - flat_b).abs().max())
    print(f"resume {mode}: run-to-run spread {spread:.3e}, resumed-vs-straight {err:.3e}")
    if spread == 0.0:
        assert torch.equal(flat_a, flat_b)
    else:
        assert err <= 2 * spread, (err, spread)
    assert torch.equal(tr_a.exp_avg, tr_a.opt.exp_avg)

    if mode == "replay":  # loading into the trainer that recorded its plans: buffers are written in place, plans stay valid
        assert tr_a._plan is not None
        ptrs = (tr_a.exp_avg.data_ptr(), tr_a.exp_avg_sq.data_ptr(), _store(lit_a).flat.data_ptr())
        lit_a.load_state_dict(module_sd)
        tr_a.load_state_dict(sd)
        plan = tr_a._plan
        flat_c = _train(lit_a, tr_a, tail)
        assert tr_a._plan is plan and ptrs == (tr_a.exp_avg.data_ptr(), tr_a.exp_avg_sq.data_ptr(),
                                               _store(lit_a).flat.data_ptr())
        err_c = float((flat_a - flat_c).abs().max())
        print(f"resume {mode}: reloaded in place vs straight {err_c:.3e}")
        assert torch.equal(flat_a, flat_c) if spread == 0.0 else err_c <= 2 * spread


def test_loading_inside_a_group_of_micro_batches_raises():
    from cultionet_amd.lightning import HipTrainer

    lit = _lit()
    tr = HipTrainer(lit, accumulate_grad_batches=2)
    batches = _batches(2)
    tr.training_step(batches[0])
    tr.training_step(batches[1])
    sd = tr.state_dict()
    tr.training_step(batches[0])  # the first micro-batch of the next group
    assert tr._micro == 1
    with pytest.raises(RuntimeError, match="micro-batches"):
        tr.load_state_dict(sd)
    tr.training_step(batches[1])
    tr.load_state_dict(sd)
    assert tr.step_count == 1


def test_hiptrainer_resumes_from_a_torch_optimizer_state(batch):
    """``d["optimizer"]`` may be ``optimizer_states[0]`` of a Lightning checkpoint written with the torch optimizer."""
    from cultionet_amd.lightning import HipTrainer

    a, b = _lit(), _lit()
    ob = _configure(b, False)[0]
    tr0 = HipTrainer(a)
    for _ in range(2):
        tr0.forward_backward(batch)
        for pb, pa in zip(_params(b), _params(a)):
            pb.grad = _store(a).grad_of(pa).clone()
        torch.nn.utils.clip_grad_norm_(_params(b), 1.0)
        ob.step()
        tr0.optimizer_step()
    tr = HipTrainer(_lit())
    tr.load_state_dict({"optimizer": ob.state_dict()})
    assert tr.step_count == 2 and tr.param_steps == [2] * len(_params(b))
    for p, q in zip(_params(b), _params(tr.lit)):
        st = tr.opt.state[q]
        assert torch.equal(st["exp_avg"], ob.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ob.state[p]["exp_avg_sq"])


@pytest.mark.parametrize("frozen", [False, True], ids=["all", "final_a_frozen"])
def test_dropin_training_matches_the_torch_optimizer(frozen):
    """The Lightning sequence by hand (zero_grad, training_step, backward, clipping hook, step, scheduler) on twin models,
    one with the NativeOptimizer and one with the torch optimizer, OneCycleLR on both: losses and parameters stay within
    the tolerance tests/test_optim_train_gpu.py holds the native route to against the drop-in route (both sides share
    the gradient kernels; the summation order of the float atomics separates them). Every native step runs in place,
    with frozen parameters too (their ``grad`` stays None)."""
    from test_optim_train_gpu import STEPS, TOL, _compare_params

    a, b = _lit(lr_scheduler="OneCycleLR"), _lit(lr_scheduler="OneCycleLR")
    if frozen:
        _freeze_final_a(a), _freeze_final_a(b)
    (oa, sa), (ob, sb) = _configure(a, True, total_steps=STEPS), _configure(b, False, total_steps=STEPS)
    batches = _batches(3)
    frozen_before = [p.detach().clone() for p in _params(a) if not p.requires_grad]
    worst = [0.0]
    for k in range(STEPS):
        losses = []
        for lit, opt, sched in ((a, oa, sa), (b, ob, sb)):
            opt.zero_grad(set_to_none=True)
            loss = lit.training_step(batches[k % 3])
            loss.backward()
            lit.configure_gradient_clipping(opt, 1.0, "norm")
            opt.step()
            sched.step()
            losses.append(float(loss.detach()))
        assert oa.in_place
        assert abs(losses[0] - losses[1]) <= TOL, (k, losses)
        _compare_params(a.cultionet_model.mask_model, b.cultionet_model.mask_model, f"step {k + 1}", TOL, worst)
    print(f"drop-in native vs torch optimizer ({'frozen final_a' if frozen else 'all'}): worst err/tol {worst[0]:.3f}")
    assert all(torch.equal(p.detach(), q) for p, q in zip([p for p in _params(a) if not p.requires_grad], frozen_before))
    assert len(frozen_before) > 0 if frozen else not frozen_before
    sd_a, sd_b = oa.state_dict(), ob.state_dict()
    assert sd_a["state"].keys() == sd_b["state"].keys()  # state for the parameters that stepped, as torch keeps it
    assert all(float(sd_a["state"][i]["step"]) == float(sd_b["state"][i]["step"]) == STEPS for i in sd_a["state"])
