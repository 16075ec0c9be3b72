"""NativeOptimizer as a torch.optim.Optimizer, without a device: defaults, param group, state_dict structure and the
reference's schedulers, against the torch classes of tests/test_configure_optimizers.py. CPU only (no kernels)."""
import types

import pytest
import torch

import optim_ref as R
from test_configure_optimizers import EXPECT_OPT, EXPECT_SCHED

LR, WD, EPS = 0.02, 3e-3, 1e-4


def _lit(**kw):
    from cultionet_amd.lightning import CultionetLitModel

    return CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, **kw)


def _pair(name, params):
    """(NativeOptimizer without a store, the torch optimizer the reference builds) over the same parameter list."""
    from cultionet_amd.lightning import LightningModuleMixin
    from cultionet_amd.optim import NativeOptimizer

    cls_name, takes, fixed = LightningModuleMixin._OPTIMIZERS[name]
    hyper = {"lr": LR, "weight_decay": WD, "eps": EPS}
    native = NativeOptimizer(params, None, cls_name, **{k: hyper[k] for k in takes}, **fixed)
    return native, R.torch_optimizer(name, params, LR, WD, EPS)


@pytest.mark.parametrize("name", list(EXPECT_OPT))
def test_defaults_are_those_of_the_torch_class(name):
    params = list(_lit().cultionet_model.parameters())
    native, stock = _pair(name, params)
    cls, fixed = EXPECT_OPT[name]
    assert type(stock) is cls and isinstance(native, torch.optim.Optimizer)
    assert native.defaults == stock.defaults
    for k, v in fixed.items():
        assert native.defaults[k] == v
    assert native.defaults["lr"] == LR
    assert native.defaults["weight_decay"] == (0 if name == "Adam" else WD)
    if name != "SGD":
        assert native.defaults["eps"] == EPS
    assert len(native.param_groups) == 1 and native.param_groups[0]["params"] == params
    assert native._step_supports_amp_scaling is True


@pytest.mark.parametrize("name", list(EXPECT_OPT))
def test_state_dict_structure_is_torchs(name):
    params = list(_lit().cultionet_model.parameters())
    native, stock = _pair(name, params)
    a, b = native.state_dict(), stock.state_dict()
    assert a.keys() == b.keys() and a["state"] == b["state"] == {}
    assert a["param_groups"] == b["param_groups"]
    assert a["param_groups"][0]["params"] == list(range(len(params)))
    stock.load_state_dict(a)   # either accepts the other's
    native.load_state_dict(b)


@pytest.mark.parametrize("name", list(EXPECT_OPT))
@pytest.mark.parametrize("sched", list(EXPECT_SCHED))
def test_every_reference_scheduler_constructs(name, sched):
    lit = _lit(optimizer=name, lr_scheduler=sched, learning_rate=LR, weight_decay=WD, eps=EPS, steplr_step_size=7)
    lit.__dict__["trainer"] = types.SimpleNamespace(max_epochs=3, estimated_stepping_batches=11)
    native, stock = _pair(name, list(lit.cultionet_model.parameters()))
    try:
        s, interval = lit._make_scheduler(native)
    except (AttributeError, RuntimeError):  # a LightningModule base that guards `.trainer`
        lit._trainer = lit.__dict__.pop("trainer")
        s, interval = lit._make_scheduler(native)
    t, _ = lit._make_scheduler(stock)
    scls, sfixed, want = EXPECT_SCHED[sched]
    assert type(s) is scls and interval == want
    for k, v in sfixed.items():
        assert getattr(s, k) == pytest.approx(v), k
    # the scheduler wrote the same initial values into both groups (OneCycleLR: lr and betas[0] / momentum)
    ga, gb = native.param_groups[0], stock.param_groups[0]
    assert ga["lr"] == gb["lr"]
    assert ga.get("betas") == gb.get("betas") and ga.get("momentum") == gb.get("momentum")


def test_second_param_group_is_refused():
    from cultionet_amd.optim import NativeOptimizer

    a, b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))
    opt = NativeOptimizer([a], None, "AdamW", lr=LR)
    with pytest.raises(ValueError, match="second param group"):
        opt.add_param_group({"params": [b]})
    with pytest.raises(ValueError, match="second param group"):
        NativeOptimizer([{"params": [a]}, {"params": [b], "lr": 0.1}], None, "SGD", lr=LR, momentum=0.9)
    with pytest.raises(NameError):
        NativeOptimizer([a], None, "Lion", lr=LR)
    with pytest.raises(RuntimeError, match="cannot step"):
        opt.step()


def test_flag_off_still_returns_the_torch_class_and_on_needs_a_device():
    lit = _lit(optimizer="AdamW", lr_scheduler="StepLR")
    assert lit.native_optimizer is False
    assert type(lit.configure_optimizers()["optimizer"]) is torch.optim.AdamW
    lit.native_optimizer = True
    assert "native_optimizer" not in lit.hparams  # a plain attribute, not a constructor keyword
    with pytest.raises(RuntimeError, match="ROCm"):
        lit.configure_optimizers()  # the model is on the CPU


def test_clipping_hook_hands_the_values_to_the_native_optimizer():
    from cultionet_amd.optim import NativeOptimizer

    lit = _lit()
    params = list(lit.cultionet_model.parameters())
    native, stock = _pair("AdamW", params)
    for p in params:
        p.grad = torch.full_like(p, 3.0)
    lit.configure_gradient_clipping(native, 1.0, "norm")
    assert (native.clip, native.clip_algorithm) == (1.0, "norm")
    assert all(bool((p.grad == 3.0).all()) for p in params)  # no gradient was touched
    lit.configure_gradient_clipping(native, 0.5, "value")
    assert (native.clip, native.clip_algorithm) == (0.5, "value")
    lit.configure_gradient_clipping(native, None, None)
    assert native.clip is None
    lit.configure_gradient_clipping(stock, 0.5, "value")  # any other optimizer: the base class clips the gradients
    assert all(bool((p.grad == 0.5).all()) for p in params)
    assert isinstance(native, NativeOptimizer)
