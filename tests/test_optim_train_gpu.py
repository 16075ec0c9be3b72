"""HipTrainer with every optimizer, clip mode, scheduler and gradient accumulation against the drop-in route: the same
model driven by ``lit.training_step`` -> ``loss.backward()`` -> torch's clip -> the torch optimizer and scheduler that
``configure_optimizers`` builds. The pattern (and the tolerances) of
tests/test_transfer_train_gpu.py::test_gradual_unfreezing_matches_torch_adamw: both sides share the gradient kernels, so
what separates them is the float-atomic summation order of the parameter gradients, amplified by the optimizer."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0)
TOL = 2e-5          # fp32: every loss, and every parameter relative to max(1, max|p|), after every optimizer step
STEPS = 6
VALUE_CLIP = 1e-4   # gradient_clip_val under the value algorithm: must clamp some elements and spare others (asserted)
# a constant rate through the real schedule paths of both sides: StepLR that never reaches its first decay
CONSTANT = dict(lr_scheduler="StepLR", steplr_step_size=1000)


def _pair(**kw):
    from cultionet_amd import synthetic as S
    from cultionet_amd.lightning import CultionetLitModel

    lits = []
    for _ in range(2):
        lit = CultionetLitModel(**KW, **kw)
        mm = lit.cultionet_model.mask_model
        mm.load_state_dict(S.seeded_state_dict(mm.state_dict()))
        lits.append(lit.to("cuda:0").train())
    return lits


def _batches(n, B=2, H=28, W=28):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data

    out = []
    for k in range(n):
        x, y, bd = S.seeded_batch(B, height=H, width=W, seed=70 + k, with_mask=True)
        out.append(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()))
    return out


def _torch_side(lit, total_steps):
    """(optimizer, scheduler, interval) of configure_optimizers; OneCycleLR reads its length from the trainer."""
    lit.__dict__["trainer"] = types.SimpleNamespace(max_epochs=1, estimated_stepping_batches=total_steps)
    try:
        out = lit.configure_optimizers()
    except (AttributeError, RuntimeError):  # a LightningModule base that guards `.trainer`
        lit._trainer = lit.__dict__.pop("trainer")
        out = lit.configure_optimizers()
    return out["optimizer"], out["lr_scheduler"]["scheduler"], out["lr_scheduler"]["interval"]


class _Reference:
    """The drop-in route with Lightning's loop semantics for clipping, accumulation and scheduler stepping."""

    def __init__(self, lit, clip_val, algorithm, accumulate=1, steps_per_epoch=1, total_steps=STEPS):
        self.lit, self.clip_val, self.algorithm, self.k = lit, clip_val, algorithm, accumulate
        self.opt, self.sched, self.interval = _torch_side(lit, total_steps)
        self.steps_per_epoch, self.steps, self.clamped = steps_per_epoch, 0, []
        self.opt.zero_grad(set_to_none=True)

    def micro(self, batch):
        loss = self.lit.training_step(batch)
        (loss / self.k if self.k > 1 else loss).backward()
        return float(loss.detach())

    def step(self):
        params = [p for p in self.lit.cultionet_model.parameters() if p.grad is not None]
        if self.algorithm == "norm":
            torch.nn.utils.clip_grad_norm_(params, self.clip_val)
        else:
            n = sum(p.numel() for p in params)
            self.clamped.append(sum(int((p.grad.abs() > self.clip_val).sum()) for p in params) / n)
            torch.nn.utils.clip_grad_value_(params, self.clip_val)
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        self.steps += 1
        if self.interval == "step" or self.steps % self.steps_per_epoch == 0:
            self.sched.step()


def _compare_params(ma, mb, what, tol, worst):
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        err = float((pa.detach() - pb.detach()).abs().max())
        bound = tol * max(1.0, float(pb.detach().abs().max()))
        worst[0] = max(worst[0], err / bound)
        assert err <= bound, (what, n, err, bound)


def _run(lit_kw, trainer_kw, algorithm="norm", one_cycle=False, steps_per_epoch=None, freeze=None):
    from cultionet_amd.lightning import HipTrainer

    if not one_cycle and steps_per_epoch is None:
        lit_kw, steps_per_epoch = {**lit_kw, **CONSTANT}, 1
    a, b = _pair(**lit_kw)
    ma, mb = a.cultionet_model.mask_model, b.cultionet_model.mask_model
    clip_val = 1.0 if algorithm == "norm" else VALUE_CLIP
    if freeze is not None:
        for mm in (ma, mb):
            for n, p in mm.named_parameters():
                p.requires_grad_(bool(freeze[0](n)))
    trainer = HipTrainer(a, gradient_clip_val=clip_val, gradient_clip_algorithm=algorithm,
                         total_steps=STEPS if one_cycle else None, steps_per_epoch=steps_per_epoch, **trainer_kw)
    ref = _Reference(b, clip_val, algorithm, steps_per_epoch=steps_per_epoch or 1)
    batches = _batches(3)
    worst, wl = [0.0], 0.0
    for k in range(STEPS):
        if freeze is not None:
            for mm in (ma, mb):
                for n, p in mm.named_parameters():
                    p.requires_grad_(bool(freeze[k](n)))
        bt = batches[k % 3]
        ln = float(trainer.training_step(bt).item())
        lr = ref.micro(bt)
        ref.step()
        wl = max(wl, abs(ln - lr) / TOL)
        assert abs(ln - lr) <= TOL, (k, ln, lr)
        _compare_params(ma, mb, f"step {k + 1}", TOL, worst)
    what = " ".join(f"{k}={v}" for k, v in {**lit_kw, "clip": algorithm}.items())
    print(f"{what}: worst err/tol loss {wl:.3f} params {worst[0]:.3f}"
          + (f", clamped share per step {[round(c, 4) for c in ref.clamped]}" if ref.clamped else ""))
    assert all(0.01 < c < 0.99 for c in ref.clamped), ref.clamped  # value clipping: elements on both sides of the bound
    assert trainer.step_count == STEPS
    return trainer, ref, (ma, mb)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("optimizer", ["Adam", "AdamW", "RAdam", "SGD"])
def test_optimizer_and_clip_mode_match_dropin(optimizer, algorithm):
    _run(dict(optimizer=optimizer), {}, algorithm=algorithm)


@pytest.mark.parametrize("scheduler", ["CosineAnnealingLR", "ExponentialLR", "StepLR"])
def test_per_epoch_schedulers_match_dropin(scheduler):
    trainer, ref, _ = _run(dict(lr_scheduler=scheduler, steplr_step_size=1), {}, steps_per_epoch=2)
    # three "epochs" of two optimizer steps: the rate of the last step is the scheduler's after two epoch steps
    lr = trainer.lr_fn(STEPS)[0]
    assert lr < 0.01 and abs(lr - ref.sched.get_last_lr()[0]) > 0  # (the torch side has stepped once more, after step 6)
    assert abs(trainer.lr_fn(STEPS + 1)[0] - ref.sched.get_last_lr()[0]) <= 1e-12 + 1e-9 * lr


@pytest.mark.parametrize("optimizer", ["SGD", "RAdam"])
def test_one_cycle_drives_lr_and_first_moment(optimizer):
    _run(dict(optimizer=optimizer), {}, one_cycle=True)


def test_radam_unfrozen_tower_starts_unrectified():
    """Heads alone for two steps, a tower joins at step 3: at step 6 the heads are rectified (t = 6) while the tower
    (t = 4) is not, inside one segmented launch."""
    heads = lambda n: n.startswith("final_")  # noqa: E731
    both = lambda n: n.startswith("final_") or n.startswith("tower_fusion.tower_b.")  # noqa: E731
    schedule = [heads, heads, both, both, both, both]
    trainer, ref, (ma, mb) = _run(dict(optimizer="RAdam"), {}, freeze=schedule)
    steps = dict(zip([id(p) for p in trainer.store.params], trainer.param_steps))
    named_b = dict(mb.named_parameters())
    seen = set()
    for n, p in ma.named_parameters():
        want = sum(1 for keep in schedule if keep(n))
        assert steps[id(p)] == want, n
        st = ref.opt.state.get(named_b[n])
        assert (int(st["step"]) if st else 0) == want, n
        seen.add(want)
    assert seen == {0, 4, 6}


def _accumulate(precision, loss_tol, param_tol, relative):
    from cultionet_amd.lightning import HipTrainer

    k, n_micro = 3, 7
    a, b = _pair(optimizer="AdamW", **CONSTANT)
    b.hip_precision = precision
    ma, mb = a.cultionet_model.mask_model, b.cultionet_model.mask_model
    trainer = HipTrainer(a, accumulate_grad_batches=k, precision=precision, steps_per_epoch=1)
    ref = _Reference(b, 1.0, "norm", accumulate=k)
    batches = _batches(n_micro)
    worst, wl = [0.0], 0.0
    for i, bt in enumerate(batches):
        ln = float(trainer.training_step(bt).item())
        lr = ref.micro(bt)
        wl = max(wl, abs(ln - lr) / loss_tol)
        assert abs(ln - lr) <= loss_tol, (i, ln, lr)
        if (i + 1) % k == 0:
            ref.step()
            assert trainer.step_count == ref.steps
            if relative:
                _compare_params(ma, mb, f"micro-batch {i + 1}", param_tol, worst)
    assert trainer.step_count == 2 and trainer.flush_accumulated() and trainer.step_count == 3
    assert not trainer.flush_accumulated()
    ref.step()  # the trailing micro-batch: still divided by k
    if relative:
        _compare_params(ma, mb, "flush", param_tol, worst)
    else:
        err = max(float((pa.detach() - pb.detach()).abs().max()) for pa, pb in zip(ma.parameters(), mb.parameters()))
        worst[0] = err / param_tol
        assert err <= param_tol, err
    assert trainer.param_steps == [3] * len(trainer.store.params)
    print(f"accumulate {precision}: worst err/tol loss {wl:.3f} params {worst[0]:.3f}")


def test_accumulated_micro_batches_match_dropin_fp32():
    _accumulate("32-true", TOL, TOL, relative=True)


def test_accumulated_micro_batches_match_dropin_bf16():
    """The mixed-precision bounds of tests/test_replay_train_gpu.py::test_replayed_steps_follow_the_eager_trajectory."""
    _accumulate("bf16-mixed", 1e-3, 0.05, relative=False)


@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed"])
def test_every_gradient_producer_adds_into_the_flat_gradient(precision):
    """Two micro-batches without a zero-fill in between leave g0 + g1 in store.flat_grad, for every parameter. A producer
    that overwrote its slice would leave g1 alone there: an error of the size of g0. Two passes over the same batch
    differ by the summation order of float atomics only (~1e-6 of the largest summand), so 1e-3 of a parameter's
    largest gradient element separates the two cleanly."""
    from cultionet_amd.lightning import HipTrainer

    (a, _) = _pair()
    single, double = HipTrainer(a, precision=precision), HipTrainer(a, precision=precision, accumulate_grad_batches=2)
    store = single.store
    assert double.store is store
    b0, b1 = _batches(2)
    g = []
    for bt in (b0, b1):
        single.forward_backward(bt)
        g.append(store.flat_grad.clone())
    double.forward_backward(b0)
    double.forward_backward(b1)
    torch.cuda.synchronize()
    want, got = g[0] + g[1], store.flat_grad
    worst = 0.0
    names = {id(p): n for n, p in a.cultionet_model.mask_model.named_parameters()}
    for p, o in zip(store.params, store.offsets):
        sl = slice(o, o + p.numel())
        scale = float(want[sl].abs().max())
        assert float(g[0][sl].abs().max()) > 0, names[id(p)]  # (every parameter has a gradient to lose)
        err = float((got[sl] - want[sl]).abs().max())
        worst = max(worst, err / (1e-3 * scale))
        assert err <= 1e-3 * scale, (names[id(p)], err, scale)
    print(f"accumulated gradients {precision}: worst err/tol {worst:.4f}")


def test_changing_requires_grad_inside_a_group_is_an_error():
    from cultionet_amd.lightning import HipTrainer

    (a, _) = _pair()
    trainer = HipTrainer(a, accumulate_grad_batches=2)
    bt = _batches(1)[0]
    trainer.training_step(bt)
    next(iter(trainer.model.parameters())).requires_grad_(False)
    with pytest.raises(RuntimeError, match="requires_grad"):
        trainer.training_step(bt)


def test_constructor_refusals():
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    def lit(**kw):
        return CultionetLitModel(**KW, **kw).to("cuda:0")

    with pytest.raises(NameError):
        HipTrainer(lit(optimizer="Lion"))
    with pytest.raises(ValueError, match="norm"):
        HipTrainer(lit(), gradient_clip_algorithm="agc")
    with pytest.raises(ValueError, match="steps_per_epoch"):
        HipTrainer(lit(lr_scheduler="StepLR"), total_steps=10)
    with pytest.raises(ValueError):
        HipTrainer(lit(), accumulate_grad_batches=0)
    assert HipTrainer(lit(optimizer="SGD")).exp_avg_sq is None  # one state buffer only
