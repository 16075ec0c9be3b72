"""Every BatchNorm buffer of the whole model, and the train-to-eval handover, end to end on the GPU.

Part 2: all running_mean / running_var / num_batches_tracked of the HIP TowerUNet after a few train-mode forwards
(HipTrainer.forward_backward: the parameters never move, asserted bitwise) against the float64 oracle of
tests/state_ref.py, per element (ratio = |got - ref64| / S, S = |m64| + sqrt(v64) or v64; no floor, no maximum).
  fp32: ratio <= state_ref.F32_BOUND = 4 x the worst ratio measured on the MI355X over all cases.
  bf16: per buffer tensor, max ratio(HIP) <= state_ref.BF16_K x max ratio(autocast bf16 oracle) of that tensor; K is
        2 x the worst quotient measured. And no tensor further out than twice the autocast oracle's worst element
        anywhere in the model (state_ref.bf16_tensor_bounds says why). tests/test_state_ref.py shows that a skipped or
        doubled step breaks these bounds in every tensor; momentum and the variance's n / (n - 1) are not claimed in
        bf16 by this check (part 3 holds the momentum, tests/test_norm_gpu.py the variance).
Measured on the MI355X (hidden 8, B=2, 28x28, three steps of seeds 50..52 unless said otherwise):
  case                      fp32 worst ratio   bf16 worst ratio (autocast oracle's worst)   bf16 worst quotient
  eager default             5.377e-7           3.731e-3 (6.738e-3)                          3.967
  eager spatial_channel     5.682e-7           3.731e-3 (6.738e-3)                          2.255
  eager res                 3.032e-7           3.098e-3 (4.015e-3)                          8.222  <- K = 2 x 8.222
  eager batchnorm_first     4.578e-7           4.457e-3 (6.747e-3)                          2.057
  eager dilations [1, 3]    5.916e-7           3.023e-3 (5.603e-3)                          1.881
  eager pool_by_max         9.617e-7           1.333e-2 (2.175e-2)                          2.041  <- F32_BOUND = 4 x 9.617e-7
  replay, six steps         8.214e-7           4.615e-3 (9.489e-3)                          3.721
  accumulate 2              5.377e-7           3.731e-3 (6.738e-3)                          3.967
  unfused PreTimeReduction  6.111e-7           3.476e-3 (6.738e-3)                          5.813
  100x100, two steps        4.061e-7           1.688e-3 (2.072e-3)                          6.520
(The fp32 oracle is itself 9.49e-7 from float64 with pool_by_max and 8.21e-7 after six steps: the fp32 figures are the
rounding of the network, not of the running update. The large quotients all sit in 3-channel head layers where the
autocast oracle happens to land within 2e-5 .. 4e-5 of float64. The autocast oracle's figures depend on the CPU's bf16
kernels: 7.03e-3 instead of 6.74e-3 for the default model on another host.)
Part 3: the same batch every step => r2 = (2 - m) r1 - (1 - m) r0 per element, whatever the batch statistic is, within
c * u * (|r0| + 2 |r1| + |r2|), c = 16, u = 2^-24 (state_ref.recurrence_residual), through eager and replayed steps.
The statistics are bit-reproducible in both precisions (fixed summation order), so the bound is not widened. Measured
worst residual / bound: fp32 0.054 (eager and replay), bf16 0.051 (eager) and 0.055 (replay); every one of the 2580
elements moves in the first step.
Part 4: the statistics-rows route that no whole-model test reaches (more than 1008 rows: the convolution writes the
rows, the BatchNorm call finishes them) at module level, against float64 on the bf16-rounded inputs and weights, with
the bound forms of tests/test_norm_gpu.py (worst error / bound measured: 0.051). 8 -> 128 channels at 100x100 has 80
rows per image: batch 13 is the first with more than 1008 (1040), batch 2 has 160.
Part 5: after every event that must invalidate the folded bf16 weights, the inference launch plans and the packed
weights, the trained model evaluates bitwise like a model built fresh from its state_dict.

Routes (from the wrapped _lib.call; ROUTES below lists what each case reached, and is asserted):
  pretime_f32         cn_pretime_fwd_f32 in training mode (its four BatchNorm layers; fp32 in both precisions)
  bn3d_view_f32       cn_bn_act_fwd_f32 on the BatchNorm3d view (the unfused PreTimeReduction)
  bn_act_f32          cn_bn_act_fwd_f32, batch statistics
  bn_act_group_f32    cn_bn_act_group_fwd_f32, batch statistics
  group_bf16_own      cn_bn_act_group_fwd_bf16 with 0 rows: its own reduction
  group_bf16_rows     cn_bn_act_group_fwd_bf16 with a row count: finishes the convolution's rows (> 1008 rows)
  group_bf16_prefin   cn_bn_act_group_fwd_bf16 with -1: the convolution finished mean, rstd and the running update
  bnstats_finished    cn_conv2d_fwd_grouped_bnstats_bf16 that finished by its last-block ticket
  bnstats_rows_only   cn_conv2d_fwd_grouped_bnstats_bf16 that wrote the rows only
  single_bf16         cn_bn_act_fwd_bf16, the single-layer bf16 entry point: the engine reaches it from nowhere. A bf16
                      view that is one run of pixel rows (a channel slice included) is the G = 1 case of the grouped
                      kernel, and a view that is not has no kernel and is refused (the last test of part 4).
The whole model at hidden 8 never has more than 1008 statistics rows (nor at hidden 32, batch 32), so group_bf16_rows
and bnstats_rows_only are reached at module level only (part 4); bn3d_view_f32 only with the fused PreTimeReduction
switched off; group_bf16_own only with batchnorm_first. In mixed precision the PreTimeReduction and the 3-channel
heads stay fp32, hence the fp32 routes there.
"""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

import state_ref as S

pytestmark = pytest.mark.gpu

PRECISIONS = ["32-true", "bf16-mixed"]
KEYS = ("distance", "edge", "crop")
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------

def _lit(kw=None):
    from cultionet_amd import synthetic as Sy
    from cultionet_amd.lightning import CultionetLitModel

    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0, **(kw or {}))
    m = lit.cultionet_model.mask_model
    m.load_state_dict(Sy.seeded_state_dict(m.state_dict()))
    return lit.to("cuda:0")


def _on_gpu(seq):
    from cultionet_amd.data import Data

    return [Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()) for x, y, bd in seq]


class _Log:
    """The C-ABI calls of the eager steps (a replayed step calls the recorded entry points directly)."""

    def __init__(self, monkeypatch):
        from cultionet_amd import engine as E

        self.calls = []
        orig = E._lib.call

        def call(name, *args):
            rc = orig(name, *args)
            self.calls.append((name, args))
            return rc

        monkeypatch.setattr(E._lib, "call", call)

    def routes(self, hw=None):
        out = set()
        for n, a in self.calls:
            if n == "cn_pretime_fwd_f32" and a[12] == 1:
                out.add("pretime_f32")
            elif n == "cn_bn_act_fwd_f32" and a[-5] == 1:
                view3d = hw is not None and a[-7] == 3 and a[-6] > hw
                out.add("bn3d_view_f32" if view3d else "bn_act_f32")
            elif n == "cn_bn_act_group_fwd_f32" and a[-6] == 1:
                out.add("bn_act_group_f32")
            elif n == "cn_bn_act_fwd_bf16":
                out.add("single_bf16")
            elif n == "cn_bn_act_group_fwd_bf16" and a[-8] == 1:
                rows = a[-2]
                out.add("group_bf16_prefin" if rows == -1 else "group_bf16_rows" if rows > 0 else "group_bf16_own")
            elif n == "cn_conv2d_fwd_grouped_bnstats_bf16":
                out.add("bnstats_finished" if a[-2]._obj.value else "bnstats_rows_only")
        return out

    def group_rows(self):
        return [a[-2] for n, a in self.calls if n == "cn_bn_act_group_fwd_bf16"]


ALL_ROUTES = {"pretime_f32", "bn3d_view_f32", "bn_act_f32", "bn_act_group_f32", "group_bf16_own", "group_bf16_rows",
              "group_bf16_prefin", "bnstats_finished", "bnstats_rows_only"}

# what the call log of each case shows on the MI355X (asserted by the case itself)
_F32 = {"pretime_f32", "bn_act_f32", "bn_act_group_f32"}
_BF16 = _F32 | {"bnstats_finished", "group_bf16_prefin"}
ROUTES = {f"{name}-32-true": _F32 for name in S.CONFIGS}
ROUTES.update({f"{name}-bf16-mixed": _BF16 for name in S.CONFIGS})
ROUTES.update({
    "bnfirst-bf16-mixed": _F32 | {"group_bf16_own"},  # BatchNorm in front of the convolution: no rows to finish
    "100x100-32-true": _F32,
    "100x100-bf16-mixed": _BF16,
    "unfused-32-true": {"bn3d_view_f32", "bn_act_f32", "bn_act_group_f32"},
    "unfused-bf16-mixed": {"bn3d_view_f32", "bn_act_f32", "bn_act_group_f32", "bnstats_finished", "group_bf16_prefin"},
    "convblock-rows": {"bnstats_rows_only", "group_bf16_rows"},
    "convblock-prefin": {"bnstats_finished", "group_bf16_prefin"},
    "aconv-rows": {"bnstats_rows_only", "group_bf16_rows"},
    "aconv-prefin": {"bnstats_finished", "group_bf16_prefin"},
    "slice-own": {"group_bf16_own"},
    "slice-rows": {"bnstats_rows_only", "group_bf16_rows"},
    "slice-prefin": {"bnstats_finished", "group_bf16_prefin"},
})


def _train(lit, precision, batches, monkeypatch, **trainer_kw):
    """``forward_backward`` over the batches; returns the trainer and the call log. Every parameter must come out bitwise
    what it was: nothing but the BatchNorm buffers is allowed to move."""
    from cultionet_amd.lightning import HipTrainer

    lit.train()
    tr = HipTrainer(lit, precision=precision, **trainer_kw)
    before = {n: p.detach().clone() for n, p in tr.model.named_parameters()}
    log = _Log(monkeypatch)
    for b in batches:
        tr.forward_backward(b)
    torch.cuda.synchronize()
    moved = [n for n, p in tr.model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert not moved, moved[:4]
    return tr, log


def _check_state(tag, lit, precision, kw, n, H=28, W=28):
    """Buffers of the HIP model after ``n`` train-mode forwards against the float64 oracle (bounds: module docstring)."""
    ref = S.trajectory(kw, "f64", n=n, H=H, W=W)[0][-1]
    got = S.snapshot(lit.cultionet_model.mask_model)
    assert set(got) == set(ref)
    wrong = [(k, int(got[k])) for k in ref if k.endswith("num_batches_tracked") and int(got[k]) != n]
    assert not wrong, wrong[:4]
    rat = S.ratios(got, ref)
    worst, wk = max((float(v.max()), k) for k, v in rat.items())
    if precision == "32-true":
        print(f"MEASURE fp32 {tag}: worst ratio {worst:.3e} at {wk}")
        bad = [(k, float(v.max())) for k, v in rat.items() if not float(v.max()) <= S.F32_BOUND]
        assert not bad, (len(bad), bad[:4])
    else:
        r16 = S.ratios(S.trajectory(kw, "bf16", n=n, H=H, W=W)[0][-1], ref)
        q = {k: float(rat[k].max()) / float(r16[k].max()) for k in rat}
        qw, qk = max((v, k) for k, v in q.items())
        print(f"MEASURE bf16 {tag}: worst ratio {worst:.3e} at {wk} (autocast oracle's worst {S.worst(r16):.3e}); worst "
              f"quotient to the autocast oracle {qw:.3f} at {qk} (HIP {float(rat[qk].max()):.3e}, autocast "
              f"{float(r16[qk].max()):.3e})")
        bounds = S.bf16_tensor_bounds(r16)
        bad = [(k, float(rat[k].max()), bounds[k]) for k in rat if not float(rat[k].max()) <= bounds[k]]
        assert not bad, (len(bad), bad[:4])


def _check_routes(tag, log, hw=28 * 28):
    got = log.routes(hw)
    print(f"MEASURE routes {tag}: {sorted(got)}")
    assert got == ROUTES[tag], (tag, sorted(got))


# ---------------------------------------------------------------------------------------------------------------------
# part 2: whole-model buffers against float64
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(S.CONFIGS))
def test_buffers_after_eager_steps(name, precision, monkeypatch):
    kw = S.CONFIGS[name]
    lit = _lit(kw)
    _, log = _train(lit, precision, _on_gpu(S.batch_sequence(3)), monkeypatch)
    _check_routes(f"{name}-{precision}", log)
    _check_state(f"eager {name}", lit, precision, kw, 3)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_buffers_after_replayed_steps(precision, monkeypatch):
    """replay=True: two eager steps, the recorded one, three from the plan -- which run no Python of the model."""
    from cultionet_amd import replay as R

    replays = []
    orig = R.replay_step
    monkeypatch.setattr(R, "replay_step", lambda plan, batch: (replays.append(plan), orig(plan, batch))[1])
    lit = _lit()
    tr, _ = _train(lit, precision, _on_gpu(S.batch_sequence(6)), monkeypatch, replay=True)
    assert tr._plan is not None and tr._plan.n_calls > 100
    assert len(replays) == 3 and all(p is tr._plan for p in replays)
    _check_state("replay default", lit, precision, {}, 6)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_buffers_after_accumulated_micro_batches(precision, monkeypatch):
    """accumulate_grad_batches=2: every micro-batch is a train-mode forward, so counters and statistics advance per
    micro-batch (the second and third accumulate into the first one's gradients; no optimizer step is taken)."""
    lit = _lit()
    tr, _ = _train(lit, precision, _on_gpu(S.batch_sequence(3)), monkeypatch, accumulate_grad_batches=2)
    assert tr._micro == 3 and tr.step_count == 0
    _check_state("accumulate default", lit, precision, {}, 3)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_buffers_with_unfused_pretime(precision, monkeypatch):
    """The layer-by-layer PreTimeReduction the engine falls back to when the fused family declines a call."""
    from cultionet_amd import engine as E

    monkeypatch.setattr(E, "pretime_reduction", lambda *a, **k: None)
    lit = _lit()
    _, log = _train(lit, precision, _on_gpu(S.batch_sequence(3)), monkeypatch)
    _check_routes(f"unfused-{precision}", log)
    _check_state("unfused pretime", lit, precision, {}, 3)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_buffers_at_100x100(precision, monkeypatch):
    """Planes of 100, 50, 25 and 13 pixels a side (odd planes, more than one block per reduction), two steps."""
    lit = _lit()
    _, log = _train(lit, precision, _on_gpu(S.batch_sequence(2, H=100, W=100)), monkeypatch)
    _check_routes(f"100x100-{precision}", log, hw=100 * 100)
    _check_state("eager default 100x100", lit, precision, {}, 2, H=100, W=100)


def test_route_table_covers_every_route():
    """The cases above and the module-level cases of part 4 reach, between them, every route that writes running
    statistics."""
    reached = set().union(*ROUTES.values())
    assert reached == ALL_ROUTES, sorted(ALL_ROUTES - reached)


# ---------------------------------------------------------------------------------------------------------------------
# part 3: the update recurrence
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("replay", [False, True], ids=["eager", "replay"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_running_update_recurrence(precision, replay, monkeypatch):
    """One batch, frozen parameters: the batch statistic b is the same at every step, so three consecutive states of any
    buffer obey r2 = (2 - m) r1 - (1 - m) r0. A second update in one step leaves (m^2 - m)(r1 - r0), another momentum
    m' leaves (m - m')(r1 - r0): thousands of times the rounding bound wherever r1 != r0."""
    from cultionet_amd.lightning import HipTrainer

    steps = 6 if replay else 3
    lit = _lit().train()
    model = lit.cultionet_model.mask_model
    batch = _on_gpu(S.batch_sequence(1, same=True))[0]
    tr = HipTrainer(lit, precision=precision, replay=replay)
    flat0 = tr.store.flat.clone()
    traj = [S.snapshot(model)]
    for _ in range(steps):
        tr.forward_backward(batch)
        torch.cuda.synchronize()
        traj.append(S.snapshot(model))
    assert torch.equal(tr.store.flat, flat0)
    if replay:
        assert tr._plan is not None and tr._plan.n_calls > 100
    worst, moved, total = (0.0, ""), 0, 0
    for k in traj[0]:
        if not S.is_stat(k):
            assert [int(t[k]) for t in traj] == list(range(steps + 1)), k
            continue
        moved += int((traj[1][k] != traj[0][k]).sum())
        total += traj[0][k].numel()
        for i in range(steps - 1):
            res, bound = S.recurrence_residual(traj[i][k], traj[i + 1][k], traj[i + 2][k])
            ratio = float((res / bound).max())
            worst = max(worst, (ratio, f"{k} steps {i}..{i + 2}"))
    print(f"MEASURE recurrence {precision} {'replay' if replay else 'eager'}: worst residual / bound {worst[0]:.3f} at "
          f"{worst[1]}; {moved} of {total} elements moved in step one")
    assert moved >= 0.99 * total
    assert worst[0] <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# part 4: the rows-only route at module level
# ---------------------------------------------------------------------------------------------------------------------

CIN, COUT, PLANE = 8, 128, 100
ROWS_LIMIT = 1008
C_ROUND, D_ROWS = 16.0, 128  # tests/test_norm_gpu.py: c of an element's own chain; tile rows of <= 128 pixels


def _rows(B):
    from cultionet_amd import _lib

    return int(_lib.query("cn_conv2d_stats_rows_bf16", B, PLANE, PLANE, COUT, 3, 3, 1, 1, 1))


def _first_batch_over_the_limit():
    B = next(b for b in range(1, 64) if _rows(b) > ROWS_LIMIT)
    assert _rows(B - 1) <= ROWS_LIMIT < _rows(B)
    return B


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed_module(mod, seed):
    """bf16-representable convolution weights (the packed bf16 copies are then exact) and random running statistics."""
    g = _gen(seed)
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.Conv2d):
                fan = m.weight[0].numel()
                m.weight.copy_((torch.randn(m.weight.shape, generator=g) / math.sqrt(fan)).to(BF).float())
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=g))
    return mod


def _nhwc16(t):
    return t.to(BF).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _stat_step(old_m, old_v, err_m, err_v, c64, depth):
    """One running update in float64 from the float64 input of the BatchNorm layer (the convolution output), and the bound
    of tests/test_norm_gpu.py for it: c*u*(|old| + m*|batch|) + m*(dm or dv), dm = D*u*(|m| + s),
    dv = 3*D*u*(m^2 + var), D = ``depth`` (128 for the convolution's tile rows); the error the buffers already carry
    decays by (1 - m)."""
    m, u = S.MOMENTUM, S.U
    n = c64.numel() // c64.shape[1]
    mean, var = c64.mean(dim=(0, 2, 3)), c64.var(dim=(0, 2, 3), unbiased=False)
    unb = var * n / (n - 1)
    dm = depth * u * (mean.abs() + var.sqrt())
    dv = 3 * depth * u * (mean ** 2 + var)
    new_m = (1 - m) * old_m + m * mean
    new_v = (1 - m) * old_v + m * unb
    err_m = (1 - m) * err_m + C_ROUND * u * (old_m.abs() + m * mean.abs()) + m * dm
    err_v = (1 - m) * err_v + C_ROUND * u * (old_v.abs() + m * unb) + m * dv
    return new_m, new_v, err_m, err_v


def _check_bn(tag, bn, old, c64s, depth=D_ROWS):
    """``bn``'s buffers after one forward per entry of ``c64s`` (the float64 outputs of the convolution in front)."""
    rm, rv = old[0].double(), old[1].double()
    em, ev = torch.zeros_like(rm), torch.zeros_like(rv)
    for c64 in c64s:
        rm, rv, em, ev = _stat_step(rm, rv, em, ev, c64, depth)
    for what, got, ref, bound in (("running_mean", bn.running_mean, rm, em), ("running_var", bn.running_var, rv, ev)):
        err = (got.detach().double().cpu() - ref).abs()
        ratio = err / bound
        print(f"MEASURE rows {tag} {what}: worst err/bound {float(ratio.max()):.3f}")
        assert torch.isfinite(got).all()
        i = int(ratio.argmax())
        assert float(ratio.max()) <= 1.0, (tag, what, i, float(err[i]), float(bound[i]))


@pytest.mark.parametrize("big", [True, False], ids=["rows_only", "finished_in_launch"])
def test_conv_block_running_statistics_by_route(big, monkeypatch):
    """ConvBlock2d(8 -> 128) at 100x100 in bf16 through the engine, two forwards. At the smallest batch with more than
    1008 statistics rows the BatchNorm call gets the row count and finishes them; at batch 2 the convolution finished
    them and the BatchNorm call gets -1."""
    from cultionet_amd import engine as E
    from cultionet_amd.convolution import ConvBlock2d

    B = _first_batch_over_the_limit() if big else 2
    mod = _seed_module(ConvBlock2d(CIN, COUT, 3, padding=1), 401).to("cuda:0").train()
    bn = mod.seq[1]
    old = (bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone())
    xs = [torch.randn((B, CIN, PLANE, PLANE), generator=_gen(410 + i)).to(BF).float() for i in range(2)]
    store = E.ParamStore(mod)
    log = _Log(monkeypatch)
    with E.using_store(store), E.recording(True):
        for x in xs:
            mod(E.Var(_nhwc16(x).cuda(), True))
    torch.cuda.synchronize()
    tag = "convblock-rows" if big else "convblock-prefin"
    assert log.group_rows() == ([_rows(B)] * 2 if big else [-1] * 2), log.group_rows()
    _check_routes(tag, log)
    w = mod.seq[0].weight.detach().double().cpu()
    _check_bn(tag, bn, old, [F.conv2d(x.double(), w, padding=1) for x in xs])


@pytest.mark.parametrize("big", [True, False], ids=["rows_only", "finished_in_launch"])
def test_residual_aconv_pair_running_statistics_by_route(big, monkeypatch):
    """ResidualAConv(8 -> 128, dilations 1 and 2): both levels of the grouped pair (G = 2) through the engine in bf16, two
    forwards. First level against the float64 convolutions of the input; second level against the float64 convolutions
    of the first level's stored bf16 activations (read back from the engine). A swapped pair, a skipped or a doubled
    update shows in every buffer."""
    from cultionet_amd import engine as E
    from cultionet_amd.convolution import ResidualAConv

    B = _first_batch_over_the_limit() if big else 2
    mod = _seed_module(ResidualAConv(CIN, COUT, dilations=[1, 2], attention_weights=None), 402).to("cuda:0").train()
    blocks = [[m.block[lv] for m in mod.res_modules] for lv in range(2)]
    olds = [[(b.seq[1].running_mean.detach().cpu().clone(), b.seq[1].running_var.detach().cpu().clone()) for b in lv]
            for lv in blocks]
    xs = [torch.randn((B, CIN, PLANE, PLANE), generator=_gen(420 + i)).to(BF).float() for i in range(2)]
    hidden = []  # per forward: the G first-level activations, as the second-level convolutions read them
    orig = E.bn_act_group

    def spy(vs, bns, act, **kw):
        out = orig(vs, bns, act, **kw)
        if not kw.get("sum_outputs", False):
            hidden.append([v.t.float().cpu() for v in out])
        return out

    monkeypatch.setattr(E, "bn_act_group", spy)
    store = E.ParamStore(mod)
    log = _Log(monkeypatch)
    with E.using_store(store), E.recording(True):
        for x in xs:
            mod(E.Var(_nhwc16(x).cuda(), True))
    torch.cuda.synchronize()
    tag = "aconv-rows" if big else "aconv-prefin"
    assert log.group_rows() == ([_rows(B)] * 4 if big else [-1] * 4), log.group_rows()
    _check_routes(tag, log)
    assert len(hidden) == 2 and all(len(h) == 2 for h in hidden)
    for g in range(2):
        b0, b1 = blocks[0][g], blocks[1][g]
        w0, w1 = (b.seq[0].weight.detach().double().cpu() for b in (b0, b1))
        c0 = [F.conv2d(x.double(), w0, padding=b0.padding, dilation=b0.dilation) for x in xs]
        _check_bn(f"{tag} level 0 branch {g}", b0.seq[1], olds[0][g], c0)
        c1 = [F.conv2d(h[g].double(), w1, padding=b1.padding, dilation=b1.dilation) for h in hidden]
        _check_bn(f"{tag} level 1 branch {g}", b1.seq[1], olds[1][g], c1)


def _channel_slice(t, lo, total):
    """``t`` ([B, C, H, W] values) as channels lo .. lo + C of a bf16 NHWC buffer of ``total`` channels: a view whose
    pixel stride is not its channel count, like a channel slice of a tower's concat buffer."""
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, total), float("nan"), dtype=BF, device="cuda:0")
    view = buf.permute(0, 3, 1, 2)[:, lo:lo + C]
    view.copy_(t.to(BF))
    return view


def test_batchnorm_first_on_a_channel_slice(monkeypatch):
    """ConvBlock2d with batchnorm_first on a channel slice of a wider NHWC buffer (a pixel stride that is not the channel
    count, as in a tower's concat buffer): the grouped kernel's own reduction, the route only batchnorm_first takes in
    the whole model. Two forwards against float64 on the bf16 inputs; D = bbn_depth of tests/test_norm_gpu.py."""
    from cultionet_amd import engine as E
    from cultionet_amd.convolution import ConvBlock2d
    from test_norm_gpu import bbn_depth

    B, C, H = 2, 32, 25  # an odd plane, more than one block
    mod = _seed_module(ConvBlock2d(C, 16, 3, padding=1, batchnorm_first=True), 403).to("cuda:0").train()
    bn = mod.seq[0]
    old = (bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone())
    xs = [(0.3 + torch.randn((B, C, H, H), generator=_gen(430 + i))).to(BF).float() for i in range(2)]
    store = E.ParamStore(mod)
    log = _Log(monkeypatch)
    with E.using_store(store), E.recording(True):
        for x in xs:
            mod(E.Var(_channel_slice(x, 8, 48), True))
    torch.cuda.synchronize()
    _check_routes("slice-own", log)
    _check_bn("slice-own", bn, old, [x.double() for x in xs], depth=bbn_depth(B * H * H, C))


@pytest.mark.parametrize("big", [True, False], ids=["rows_only", "finished_in_launch"])
def test_conv_into_a_channel_slice_updates_running_statistics_once(big, monkeypatch):
    """conv2d(want_stats, bn) writing into a channel slice of a wider buffer, then bn_act on that slice. Above 1008 rows
    the BatchNorm call finishes the rows. At batch 2 the convolution launch has already finished them AND made the
    running update: the BatchNorm call gets -1 and must not make it again."""
    from cultionet_amd import engine as E

    B = _first_batch_over_the_limit() if big else 2
    conv = torch.nn.Conv2d(CIN, COUT, 3, padding=1, bias=False)
    bn = torch.nn.BatchNorm2d(COUT)
    mods = _seed_module(torch.nn.ModuleList([conv, bn]), 404).to("cuda:0").train()
    old = (bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone())
    xs = [torch.randn((B, CIN, PLANE, PLANE), generator=_gen(440 + i)).to(BF).float() for i in range(2)]
    store = E.ParamStore(mods)
    log = _Log(monkeypatch)
    with E.using_store(store), E.recording(True):
        for x in xs:
            out = _channel_slice(torch.zeros((B, COUT, PLANE, PLANE)), 64, 256)
            y = E.conv2d(E.Var(_nhwc16(x).cuda(), True), conv, 1, 1, 1, out=out, want_stats=True, bn=bn)
            assert y.t.data_ptr() == out.data_ptr() and y.stats is not None
            E.bn_act(y, bn, E.ACT_SILU, training=True)
    torch.cuda.synchronize()
    tag = "slice-rows" if big else "slice-prefin"
    _check_routes(tag, log)
    w = conv.weight.detach().double().cpu()
    _check_bn(tag, bn, old, [F.conv2d(x.double(), w, padding=1) for x in xs])


def test_bf16_batchnorm_refuses_a_view_that_is_not_one_run_of_rows():
    """Every bf16 BatchNorm kernel walks P = B*H*W pixel rows at ONE stride. A spatial crop of a larger NHWC buffer
    (rows of 26 pixels that lie 28 apart) is not such a run: the engine must refuse it -- as input or as output -- before
    any launch and leave the running statistics alone. (It used to hand such views to cn_bn_act_fwd_bf16, which read
    the first P pixels of the parent buffer instead: wrong batch statistics into the running buffers, silently.) The
    same values as one dense run go through, and are held to float64."""
    from cultionet_amd import engine as E
    from test_norm_gpu import bbn_depth

    B, C, H = 2, 32, 28
    bn = _seed_module(torch.nn.BatchNorm2d(C), 405).to("cuda:0").train()
    old = (bn.running_mean.detach().cpu().clone(), bn.running_var.detach().cpu().clone())
    values = (0.3 + torch.randn((B, C, H, H), generator=_gen(450))).to(BF).float()
    full = _nhwc16(values).cuda()
    crop = full[:, :, 1:-1, 1:-1]
    assert not E._dense16(crop) and crop.data_ptr() % 16 == 0
    store = E.ParamStore(bn)
    with E.using_store(store), E.recording(True):
        with pytest.raises(NotImplementedError):
            E.bn_act(E.Var(crop, True), bn, E.ACT_SILU, training=True)
        with pytest.raises(NotImplementedError):
            E.bn_act(E.Var(_nhwc16(values[:, :, 1:-1, 1:-1]).cuda(), True), bn, E.ACT_SILU, training=True,
                     out=torch.empty_like(full)[:, :, 1:-1, 1:-1])
        torch.cuda.synchronize()
        assert torch.equal(bn.running_mean.cpu(), old[0]) and torch.equal(bn.running_var.cpu(), old[1])
        inner = values[:, :, 1:-1, 1:-1]
        E.bn_act(E.Var(_nhwc16(inner).cuda(), True), bn, E.ACT_SILU, training=True)
    torch.cuda.synchronize()
    _check_bn("dense copy of the crop", bn, old, [inner.double()], depth=bbn_depth(B * (H - 2) ** 2, C))


# ---------------------------------------------------------------------------------------------------------------------
# part 5: train-to-eval handover against a model without caches
# ---------------------------------------------------------------------------------------------------------------------

def _scene():
    g = _gen(9)
    return torch.randint(0, 9000, (3, 12, 70, 95), generator=g, dtype=torch.int32).to(torch.int16).cuda()


def _predictor(lit, precision):
    from cultionet_amd.predict import SlidingWindowPredictor

    # 3 x 3 windows of 32 in batches of 4: two launch plans (full batches and the ragged last one)
    return SlidingWindowPredictor(lit, window_size=32, padding=4, batch_size=4, mean=torch.tensor([0.31, 0.28, 0.35]),
                                  std=torch.tensor([0.21, 0.19, 0.24]), precision=precision, replay=True,
                                  pixels_per_launch=0)


def _evaluate(lit, predictor, batch, scene, precision):
    lit.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF, enabled=precision != "32-true"):
        pred = lit(batch)
    maps = {k: pred[k].detach().clone() for k in KEYS}
    mosaic = predictor.predict_scene(scene).clone()
    assert not lit.training
    return maps, mosaic


def _fresh_copy(lit, precision):
    """A model that has never run: no folded weights, no plans, no packed copies. Loaded from a deep copy of the
    trained model's state_dict."""
    from cultionet_amd.lightning import CultionetLitModel

    fresh = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0)
    fresh.load_state_dict(copy.deepcopy(lit.state_dict()))
    fresh = fresh.to("cuda:0").eval()
    return fresh, _predictor(fresh, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_train_to_eval_handover_is_bitwise_a_fresh_model(precision, monkeypatch):
    """One model through: eval (fills folds and plans) -> two eager training steps -> replayed training steps -> an
    in-place torch write to a running_mean -> load_state_dict -> one more native step -> state_dict round trip. After
    each, lit(batch) and the planned sliding-window predictor must give bitwise what a freshly built model loaded with
    the current state_dict gives (the eval forward is bit-reproducible), and something other than at the stage before."""
    from cultionet_amd import engine as E
    from cultionet_amd import replay as R
    from cultionet_amd import synthetic as Sy
    from cultionet_amd.lightning import HipTrainer

    assert E._EVAL_FUSION
    replays = []
    orig = R.replay_step
    monkeypatch.setattr(R, "replay_step", lambda plan, batch: (replays.append(plan), orig(plan, batch))[1])
    lit = _lit()
    model = lit.cultionet_model.mask_model
    predictor = _predictor(lit, precision)
    batches = _on_gpu(S.batch_sequence(3))
    scene = _scene()
    eager = HipTrainer(lit, precision=precision)
    planned = HipTrainer(lit, precision=precision, replay=True)
    seen = []

    def stage(what):
        got = _evaluate(lit, predictor, batches[0], scene, precision)
        fresh, fresh_predictor = _fresh_copy(lit, precision)
        want = _evaluate(fresh, fresh_predictor, batches[0], scene, precision)
        for k in KEYS:
            assert torch.equal(got[0][k], want[0][k]), f"{what}: lit(batch)[{k}] is not what a fresh model gives"
        assert torch.equal(got[1], want[1]), f"{what}: the planned predictor's mosaic is not what a fresh model gives"
        if seen:
            assert all(not torch.equal(got[0][k], seen[-1][0][k]) for k in KEYS), f"{what}: same maps as before"
            assert not torch.equal(got[1], seen[-1][1]), f"{what}: same mosaic as before"
        seen.append(got)

    stage("1 first eval")
    lit.train()
    for i in range(2):
        eager.training_step(batches[i])
    stage("2 after two eager steps")
    lit.train()
    for i in range(12):  # two eager steps, the recorded one, then from the plan
        if len(replays) == 3:
            break
        planned.training_step(batches[i % 3])
    assert planned._plan is not None and len(replays) == 3
    stage("3 after replayed steps")
    deep = model.encoder.down_c.res_conv.res_modules[0].block[1].seq[1]
    with torch.no_grad():
        deep.running_mean.mul_(1.1)
    stage("4 after an in-place write to running_mean")
    model.load_state_dict(Sy.seeded_state_dict(model.state_dict(), salt=1))
    stage("5 after load_state_dict")
    lit.train()
    eager.training_step(batches[1])
    stage("6 after a native step on the loaded weights")
    # 7: the state_dict carries everything the next training forward needs
    from cultionet_amd.lightning import CultionetLitModel

    third = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0)
    third.load_state_dict(copy.deepcopy(lit.state_dict()))
    third = third.to("cuda:0").train()
    lit.train()
    a = eager.forward_backward(batches[2]).clone()
    b = HipTrainer(third, precision=precision).forward_backward(batches[2]).clone()
    assert torch.equal(a, b), (float(a), float(b))
