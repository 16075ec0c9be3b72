"""HipTrainer(replay=True) with gradient accumulation against the eager trainer on identical weights and micro-batches.
A step has two phases with a recorded plan each: the first micro-batch of a group zeroes the flat gradient and repacks
the weights the optimizer just wrote; the later ones do neither, and a plan of one phase never replays for the other."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pair(precision, k):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    trainers = []
    for replay in (False, True):
        lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0)
        m = lit.cultionet_model.mask_model
        m.load_state_dict(S.seeded_state_dict(m.state_dict()))
        trainers.append(HipTrainer(lit.to("cuda:0").train(), precision=precision, replay=replay,
                                   accumulate_grad_batches=k))
    batches = []
    for i in range(3):
        x, y, bd = S.seeded_batch(2, height=28, width=28, seed=50 + i, with_mask=True)
        batches.append(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()))
    return trainers, batches


# the bounds of tests/test_replay_train_gpu.py::test_replayed_steps_follow_the_eager_trajectory (eight optimizer steps)
@pytest.mark.parametrize("precision,loss_tol,param_tol", [("32-true", 2e-6, 1e-4), ("bf16-mixed", 1e-3, 0.05)])
def test_replayed_accumulation_follows_the_eager_trajectory(precision, loss_tol, param_tol):
    from cultionet_amd import replay as R

    (eager, plan), batches = _pair(precision, 2)
    replayed = {False: 0, True: 0}  # micro-steps that ran from a plan, by the phase the PLAN was recorded for
    orig = R.replay_step

    def counting(p, batch):
        assert p.accumulates == plan._accumulating  # the phase of the plan is the phase of the micro-step
        replayed[p.accumulates] += 1
        return orig(p, batch)

    R.replay_step = counting
    try:
        le, lp = [], []
        for i in range(16):
            b = batches[i % 3]
            le.append(float(eager.training_step(b).item()))
            lp.append(float(plan.training_step(b).item()))
    finally:
        R.replay_step = orig
    assert eager.step_count == plan.step_count == 8
    zeroing, adding = plan._plan, plan._plan_acc
    assert zeroing is not None and adding is not None and zeroing is not adding and zeroing.key != adding.key
    # eight micro-steps per phase: two eager, one recorded, five replayed (fewer if a recording had to be repeated
    # because a scratch buffer moved under it)
    assert 1 <= replayed[False] <= 5 and 1 <= replayed[True] <= 5, replayed
    assert not zeroing.accumulates and zeroing.grad_fills == 1 and zeroing.repacks >= 1
    assert adding.accumulates and adding.grad_fills == 0 and adding.repacks == 0
    assert adding.n_calls > 100 and zeroing.n_calls >= adding.n_calls + zeroing.grad_fills + zeroing.repacks
    err = float(np.abs(np.array(le) - np.array(lp)).max())
    pe = dict(eager.model.named_parameters())
    worst = max(float((p.detach() - pe[n].detach()).abs().max()) for n, p in plan.model.named_parameters())
    print(f"replay + accumulation {precision}: loss err/tol {err / loss_tol:.3f}, parameter err/tol {worst / param_tol:.3f}")
    assert err <= loss_tol, (le, lp)
    assert worst <= param_tol, worst
    assert le[-1] < le[0]
    for k in ("distance", "edge", "crop"):
        assert torch.isfinite(plan.last_outputs[k]).all()
