"""The float64 restatement of the optimizers (tests/optim_ref.py) against torch.optim on the CPU, with the reference's
constructor arguments, and the per-epoch schedules of the native step against torch.optim.lr_scheduler. No GPU."""
import pytest
import torch

import optim_ref as R

LR, WD, EPS = 0.01, 1e-3, 1e-4  # the reference's defaults (scripts/args.yml)
STEPS = 14                       # RAdam (betas[1] = 0.99) rectifies from step 6 on: both branches


def _run(name, steps, sched_cls=None, clip=None):
    """max |p_torch - p_ref| over ``steps`` steps of float64 torch.optim vs optim_ref from the same start."""
    gen = torch.Generator().manual_seed(17)
    p0 = torch.randn(257, generator=gen, dtype=torch.float64) * 0.05
    p = torch.nn.Parameter(p0.clone())
    opt = R.torch_optimizer(name, [p], LR, WD, EPS)
    sch = sched_cls(opt) if sched_cls is not None else None
    q, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    worst = 0.0
    for t in range(1, steps + 1):
        g = torch.randn(257, generator=gen, dtype=torch.float64) * (0.3 if t % 3 else 3.0)
        p.grad = g.clone()
        if clip is not None:
            torch.nn.utils.clip_grad_value_([p], clip)
            g = R.clip_value(g, clip)
            assert torch.equal(p.grad, g)
        grp = opt.param_groups[0]
        beta1 = grp["momentum"] if name == "SGD" else grp["betas"][0]
        q, m, v = R.step(name, q, g, m, v, grp["lr"], beta1, EPS, WD, t)
        opt.step()
        if sch is not None:
            sch.step()
        worst = max(worst, float((p.detach() - q).abs().max()))
    return worst


@pytest.mark.parametrize("name", ["Adam", "AdamW", "RAdam", "SGD"])
@pytest.mark.parametrize("schedule", ["constant", "one_cycle"])
def test_reference_rules_match_torch(name, schedule):
    sched = None
    if schedule == "one_cycle":  # cycles lr AND betas[0] / momentum
        sched = lambda opt: torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=STEPS)  # noqa: E731
    worst = _run(name, STEPS, sched)
    print(f"{name} {schedule}: max |dp| {worst:.3e} (bound 1e-14)")
    assert worst <= 1e-14  # float64 rounding of ~14 steps on |p| ~ 0.1


def test_radam_crosses_the_rectification_switch():
    assert all(R.radam_rect(t, 0.99) is None for t in range(1, 6))
    assert all(R.radam_rect(t, 0.99) is not None for t in range(6, STEPS + 1))


@pytest.mark.parametrize("name", ["AdamW", "SGD"])
def test_value_clip_matches_torch(name):
    assert _run(name, STEPS, clip=0.5) <= 1e-14


def test_one_cycle_cycles_the_first_moment_of_every_optimizer():
    from cultionet_amd.schedules import OneCycleLR

    mine = OneCycleLR(LR, 20)
    for name in ("Adam", "AdamW", "RAdam", "SGD"):
        p = torch.nn.Parameter(torch.zeros(3))
        opt = R.torch_optimizer(name, [p], LR, WD, EPS)
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=LR, total_steps=20)
        for k in range(1, 21):
            grp = opt.param_groups[0]
            b1 = grp["momentum"] if name == "SGD" else grp["betas"][0]
            lr, beta1 = mine(k)
            assert abs(lr - grp["lr"]) <= 1e-12 + 1e-9 * abs(grp["lr"]) and abs(beta1 - b1) <= 1e-12, (name, k)
            p.grad = torch.ones(3)
            opt.step()
            sch.step()


def _epochs(make_torch, mine, epochs=100):
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=LR)
    sch = make_torch(opt)
    worst = 0.0
    for e in range(epochs):
        lr = opt.param_groups[0]["lr"]
        tol = 1e-12 + 1e-9 * abs(lr)  # the tolerance of tests/test_schedules.py
        worst = max(worst, abs(mine(e) - lr) / tol)
        assert abs(mine(e) - lr) <= tol, (e, mine(e), lr)
        p.grad = torch.ones(3)
        opt.step()
        sch.step()
    return worst


def test_cosine_annealing_matches_torch():
    from cultionet_amd.schedules import CosineAnnealingLR

    sched = torch.optim.lr_scheduler
    worst = _epochs(lambda o: sched.CosineAnnealingLR(o, T_max=20, eta_min=1e-5, last_epoch=-1), CosineAnnealingLR(LR))
    print(f"cosine: worst err/tol {worst:.3e}")


def test_exponential_matches_torch():
    from cultionet_amd.schedules import ExponentialLR

    worst = _epochs(lambda o: torch.optim.lr_scheduler.ExponentialLR(o, gamma=0.5), ExponentialLR(LR))
    print(f"exponential: worst err/tol {worst:.3e}")


@pytest.mark.parametrize("step_size", [1, 5, 7])
def test_steplr_matches_torch(step_size):
    from cultionet_amd.schedules import StepLR

    worst = _epochs(lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=step_size, gamma=0.5), StepLR(LR, step_size))
    print(f"steplr {step_size}: worst err/tol {worst:.3e}")


def test_per_epoch_adapter_maps_optimizer_steps_to_epochs():
    from cultionet_amd.schedules import PerEpoch, StepLR

    fn = PerEpoch(StepLR(LR, 1), steps_per_epoch=3)
    assert [fn(k) for k in (1, 3, 4, 7)] == [(LR, 0.9), (LR, 0.9), (LR * 0.5, 0.9), (LR * 0.25, 0.9)]
