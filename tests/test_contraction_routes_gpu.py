"""The contraction routes of the real workloads, held against the ledger (tests/contraction_routes.py).

No numerics here: one native training step (HipTrainer forward + loss + backward, the second one, once every workspace
exists), one eval forward, and the sliding-window predict forward are run inside the route recorder at the shapes the
benchmark and the CLI defaults run. The recorded keys must equal PRODUCTION[config] (so a dispatch change shows in
review as a changed ledger line), every one of them must be the route of some exact case in CASES, and none may be an
instantiation the ledger calls unreachable. The launches are recorded from the eager path: a replayed plan repeats
exactly these launches without passing the host dispatchers again.
"""
import pytest
import torch

import contraction_routes as CR
from route_ledger import covers, instantiation, production_facts, recording, route_key

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _keys(launches, phase):
    """Sorted route keys of the recorded launches; -s prints the first launch that took each."""
    first = {}
    for name, desc in launches:
        k = route_key(name, desc)
        first.setdefault(k + production_facts(k, phase), desc)
    for k in sorted(first):
        print(f"  {phase}: {k} <- {first[k]}")
    return sorted(first)


def _hold(config, got):
    print(f"PRODUCTION {config!r}: {got!r},")
    by_inst = {}
    for phase, keys in got.items():
        for k in keys:
            by_inst.setdefault(instantiation(k), set()).add(phase)
    for inst in sorted(by_inst):
        print(f"  {inst}: {sorted(by_inst[inst])}")
    want = CR.PRODUCTION.get(config)
    assert want is not None, f"route ledger: no PRODUCTION entry for {config}; it emitted {got}"
    for phase in sorted(set(want) | set(got)):
        old, new = sorted(want.get(phase, [])), sorted(got.get(phase, []))
        gone, came = [k for k in old if k not in new], [k for k in new if k not in old]
        assert old == new, f"route changed: {config} {phase}: no longer taken {gone}, newly taken {came}"
    case_keys = [k for parts in CR.CASES.values() for keys in parts.values() for k in keys]
    for phase, keys in got.items():
        for k in keys:
            assert instantiation(k) not in CR.UNREACHABLE, f"{config} {phase}: {k} runs an 'unreachable' instantiation"
            assert any(covers(c, k) for c in case_keys), f"{config} {phase}: no exact case takes the route {k}"


TRAIN = {
    # config id: precision, hidden, batch, dropout
    "train fp32 hidden 32 batch 8": ("32-true", 32, 8, 0.0),
    "train bf16-mixed hidden 32 batch 32": ("bf16-mixed", 32, 32, 0.0),
    "train bf16-mixed hidden 64 batch 4 dropout 0.1": ("bf16-mixed", 64, 4, 0.1),
}


@pytest.mark.parametrize("config", list(TRAIN))
def test_training_step_and_eval_forward_routes(config, tmp_path):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    dev = _dev()
    precision, hidden, B, dropout = TRAIN[config]
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=hidden, dropout=dropout)
    model = lit.cultionet_model.mask_model
    model.load_state_dict(S.seeded_state_dict(model.state_dict()))
    lit = lit.to(dev).train()
    x, y, bdist = S.seeded_batch(B, seed=7)
    batch = Data(x=x.to(dev), y=y.to(dev), bdist=bdist.to(dev), lon=torch.zeros(B, device=dev),
                 lat=torch.zeros(B, device=dev))
    trainer = HipTrainer(lit, gradient_clip_val=1.0, precision=precision, replay=False)
    trainer.forward_backward(batch)  # the first step sizes every workspace
    torch.cuda.synchronize()
    got = {}
    with recording(tmp_path) as launches:
        trainer.forward_backward(batch)
    got["step"] = _keys(launches, "step")
    lit.eval()
    with recording(tmp_path) as launches, torch.no_grad(), \
            torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision != "32-true"):
        model(batch.x)
    got["eval"] = _keys(launches, "eval")
    _hold(config, got)


PREDICT = {
    # config id: precision, scene side (windows of 100 + 2 x 5), windows per forward
    "predict fp32 4 windows": ("32-true", 200, 4),
    "predict bf16-mixed 4 windows": ("bf16-mixed", 200, 4),
    "predict fp32 36 windows": ("32-true", 600, 36),
    "predict bf16-mixed 36 windows": ("bf16-mixed", 600, 36),
}


@pytest.mark.parametrize("config", list(PREDICT))
def test_predict_forward_routes(config, tmp_path):
    from cultionet_amd import synthetic as S
    from cultionet_amd.lightning import CultionetLitModel
    from cultionet_amd.predict import SlidingWindowPredictor

    dev = _dev()
    precision, side, n = PREDICT[config]
    lit = CultionetLitModel(in_channels=4, in_time=25, hidden_channels=32, dropout=0.0)
    model = lit.cultionet_model.mask_model
    model.load_state_dict(S.seeded_state_dict(model.state_dict()))
    lit = lit.to(dev).eval()
    g = torch.Generator().manual_seed(11)
    scene = (torch.rand(4, 25, side, side, generator=g) * 10000.0).to(torch.int16).to(dev)
    sp = SlidingWindowPredictor(lit, window_size=100, padding=5, batch_size=n, precision=precision, replay=False,
                                pixels_per_launch=0)
    assert sp.launch_bs == n == (side // 100) ** 2  # one forward of [n, 4, 25, 110, 110]
    sp.predict_scene(scene)
    torch.cuda.synchronize()
    with recording(tmp_path) as launches:
        sp.predict_scene(scene)
    _hold(config, {"forward": _keys(launches, "eval")})
