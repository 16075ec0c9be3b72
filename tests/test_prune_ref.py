"""Global magnitude pruning, host side: the prunable set, the count of a round, the refusals, and the restated rule
(tests/prune_ref.py) against torch.nn.utils.prune.global_unstructured. Runs without a GPU."""
import types

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils import prune

import prune_ref as R


class _Gate(nn.Module):
    def __init__(self):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(1))
        self.sca_gamma1 = nn.Parameter(torch.ones(1))


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3)
        self.bn = nn.BatchNorm2d(5)
        self.ln = nn.LayerNorm(5)
        self.seq = nn.Sequential(nn.Linear(5, 7), nn.ReLU(), nn.Linear(7, 2, bias=False))
        self.gate = _Gate()
        self.blocks = nn.ModuleList([nn.Conv2d(5, 5, 1, bias=False)])
        self.named = nn.ModuleDict({"head": nn.Linear(2, 3)})


EXPECTED = {("conv", "weight"), ("conv", "bias"), ("bn", "weight"), ("bn", "bias"), ("ln", "weight"), ("ln", "bias"),
            ("seq.0", "weight"), ("seq.0", "bias"), ("seq.2", "weight"), ("blocks.0", "weight"),
            ("named.head", "weight"), ("named.head", "bias")}


def test_prunable_set_is_weight_and_bias_of_non_containers():
    from cultionet_amd.pruning import prunable_parameters

    net = _Net()
    net.conv.weight.requires_grad_(False)  # (does not matter)
    got = prunable_parameters(net)
    assert {(m, n) for m, n, _ in got} == EXPECTED and len(got) == len(EXPECTED)
    named = dict(net.named_parameters())
    assert all(p is named[f"{m}.{n}"] for m, n, p in got)
    # what Lightning's ModelPruning collects by default
    containers = (nn.Sequential, nn.ModuleList, nn.ModuleDict)
    theirs = {id(getattr(m, n)) for n in ("weight", "bias") for m in net.modules()
              if not isinstance(m, containers) and getattr(m, n, None) is not None}
    assert theirs == {id(p) for _, _, p in got}


def test_the_lightning_module_itself_is_a_container():
    from cultionet_amd.lightning import _Base
    from cultionet_amd.pruning import prunable_parameters

    class Lit(_Base):
        def __init__(self):
            super().__init__()
            self.weight = nn.Parameter(torch.ones(3))  # directly on the LightningModule: not pruned
            self.inner = nn.Linear(2, 2)

    assert {(m, n) for m, n, _ in prunable_parameters(Lit())} == {("inner", "weight"), ("inner", "bias")}


def test_shared_parameter_is_listed_once():
    from cultionet_amd.pruning import prunable_parameters

    net = nn.Sequential(nn.Linear(4, 4), nn.Linear(4, 4))
    net[1].weight = net[0].weight
    assert [(m, n) for m, n, _ in prunable_parameters(net)] == [("0", "weight"), ("0", "bias"), ("1", "bias")]


def test_flags_cover_prunable_parameters_and_nothing_else():
    from cultionet_amd.pruning import build_flags, prunable_parameters

    net = _Net()
    params = list(net.parameters())
    offs, n = R.layout([p.numel() for p in params])
    store = types.SimpleNamespace(params=params, offsets=offs, numel=n)
    flags = build_flags([p for _, _, p in prunable_parameters(net)], store).numpy()
    want = np.zeros(n, dtype=np.uint8)
    prunable = {id(p) for _, _, p in prunable_parameters(net)}
    for p, o in zip(params, offs):
        if id(p) in prunable:
            want[o:o + p.numel()] = 3
    assert (flags == want).all()
    assert int((flags == 3).sum()) == sum(p.numel() for p in params) - 2  # all but gamma and sca_gamma1
    assert int((flags == 0).sum()) > 2  # (padding exists: odd-sized tensors)
    with pytest.raises(ValueError, match="ParamStore"):
        build_flags([nn.Parameter(torch.ones(2))], store)


def test_round_count_follows_python_round_and_refuses():
    from cultionet_amd.pruning import prune_count

    # round-half-even: 0.5 * 5 = 2.5 -> 2, 0.5 * 7 = 3.5 -> 4, 0.3 * 15 = 4.5 -> 4
    for amount, alive in [(0.5, 5), (0.5, 7), (0.3, 15), (0.3, 1000), (0.0, 9), (1.0, 9), (0.1, 4), (0.3, 10643211)]:
        assert prune_count(amount, alive) == round(amount * alive) == prune._compute_nparams_toprune(amount, alive)
    assert prune_count(0.5, 5) == 2 and prune_count(0.5, 7) == 4
    assert prune_count(3, 10) == 3 and prune_count(0, 10) == 0 and prune_count(10, 10) == 10
    assert prune_count(np.int64(4), 10) == 4 and prune_count(np.float32(0.5), 8) == 4
    with pytest.raises(ValueError):
        prune_count(11, 10)
    with pytest.raises(ValueError):
        prune_count(-1, 10)
    with pytest.raises(ValueError):
        prune_count(1.5, 10)
    with pytest.raises(ValueError):
        prune_count(-0.1, 10)
    with pytest.raises(TypeError):
        prune_count("0.3", 10)
    with pytest.raises(TypeError):
        prune_count(True, 10)


def test_restated_rule_equals_torch_global_unstructured_over_three_rounds():
    from cultionet_amd.pruning import prunable_parameters

    torch.manual_seed(5)
    net = _Net()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p))
    pairs = prunable_parameters(net)
    params = list(net.parameters())
    offs, n = R.layout([p.numel() for p in params])
    offset = {id(p): o for p, o in zip(params, offs)}
    flat = np.zeros(n, dtype=np.float32)
    flags = np.zeros(n, dtype=np.uint8)
    for p, o in zip(params, offs):
        flat[o:o + p.numel()] = p.detach().numpy().ravel()
    spans = []
    for mod, name, p in pairs:
        flags[offset[id(p)]:offset[id(p)] + p.numel()] = 3
        spans.append((net.get_submodule(mod), name, offset[id(p)], p.numel()))
    prunable = np.abs(flat[flags == 3])
    assert np.unique(prunable).size == prunable.size  # |w| distinct: the condition under which torch is unambiguous
    alive = int((flags == 3).sum())
    for _ in range(3):
        k = R.round_count(0.3, alive)
        prune.global_unstructured([(m, name) for m, name, _, _ in spans], pruning_method=prune.L1Unstructured, amount=0.3)
        flags = R.prune_round(flat, flags, k)
        alive -= k
        assert int((flags == 3).sum()) == alive
        for m, name, o, size in spans:
            theirs = getattr(m, name + "_mask").numpy().ravel() != 0
            assert (theirs == ((flags[o:o + size] & 1) != 0)).all(), name


def test_ties_go_to_the_lowest_index_and_zero_signs_are_one_key():
    from cultionet_amd import pruning

    assert (pruning.ALIVE, pruning.PRUNABLE) == (R.ALIVE, R.PRUNABLE)  # the restatement speaks the package's flag bits
    flat = np.array([0.5, -0.0, 0.25, 0.0, -0.25, 0.25, 9.0, 0.25], dtype=np.float32)
    flags = np.array([3, 3, 3, 3, 3, 3, 2, 3], dtype=np.uint8)  # element 6: pruned earlier
    out = R.prune_round(flat, flags, 4)
    assert out.tolist() == [3, 2, 2, 2, 2, 3, 2, 3]  # both zeros, then the first two of the four |0.25|
    assert R.masked(flat, out).tolist() == [0.5, 0.0, 0.0, 0.0, 0.0, 0.25, 0.0, 0.25]
    assert not np.signbit(R.masked(flat, out)[1])
