"""The yardstick of the mixed-precision predict tests, on the CPU oracle alone (no GPU, no kernel): the distance between
oracle/predict_ref.predict_scene under CPU bf16 autocast and in fp32 (tests/predict_bound_ref.py).

* It is steady: on two scenes each of its nine statistics moves by less than the 1.5 margin the GPU tests allow.
* The bound has teeth: structural errors planted into the fp32 oracle -- a 3x3 tap dropped or the input channels rolled
  by one in a mid-network convolution, a tap dropped in a final 3x3 -- land several times above 1.5 x the yardstick.
* Its blind spots, asserted so that nobody reads more into the whole-model bound than it holds: BatchNorm eps 1e-3 for
  1e-5 everywhere and one running_var times 1.1 stay below the reference's own bf16 noise. (A running_var of the first
  encoder stage times 1.1 does reach 1.9 x: how far such an error shows depends on the depth below it.)

The mutated layers are named, not indexed. Run with -s to read the ratios.
"""
import copy

import numpy as np
import pytest
import torch

import predict_bound_ref as P
from oracle import predict_ref
from oracle import towerunet_oracle as O
from oracle.make_golden import calibrate_bn

H, W, WS, PAD = 70, 95, 40, 4
MEAN = np.array([0.31, 0.28, 0.35], dtype=np.float32)
STD = np.array([0.21, 0.19, 0.24], dtype=np.float32)
SEEDS = (5, H * 131 + W)  # the scenes of the two GPU tests in tests/test_predict_edges_gpu.py

MID_CONV = "tower_fusion.tower_b.res_conv.res_modules.0.block.1.seq.0"  # 32 -> 32, 3x3, at half resolution
MID_BN = "tower_fusion.tower_b.res_conv.res_modules.0.block.1.seq.1"    # the BatchNorm behind it
FINAL_CONV = "final_a.fuse_conv.seq.0"                                   # 3 -> 3, 3x3, the full-resolution head's last


def _scene(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16).numpy().astype(np.float64)


def _run(model, scene, **kw):
    return predict_ref.predict_scene(model, scene, WS, PAD, MEAN, STD, **kw)


@pytest.fixture(scope="module")
def oracle():
    """The model of the GPU predict tests, built without build_pair (which needs a GPU), its fp32 mosaics and the
    yardstick on both scenes: computed once and left unchanged."""
    m = O.TowerUNet(3, 12, hidden_channels=8)
    m.load_state_dict(O.seeded_state_dict(m.state_dict()))
    xc, _, _ = O.seeded_batch(2, channels=3, time=12, height=28, width=28, seed=77)
    calibrate_bn(m, lambda: m(xc))
    layers = dict(m.named_modules())
    assert tuple(layers[MID_CONV].weight.shape) == (32, 32, 3, 3) and tuple(layers[FINAL_CONV].weight.shape) == (3, 3, 3, 3)
    assert isinstance(layers[MID_BN], torch.nn.BatchNorm2d)
    scenes = {s: _scene(s) for s in SEEDS}
    f32 = {s: _run(m, scenes[s]) for s in SEEDS}
    b16 = {s: _run(m, scenes[s], autocast=True) for s in SEEDS}
    return {"model": m, "scenes": scenes, "f32": f32, "b16": b16,
            "yardstick": {s: P.band_stats(b16[s], f32[s]) for s in SEEDS}}


def test_autocast_option_widens_and_leaves_fp32_alone(oracle):
    """autocast=True returns a uint16 mosaic that differs from the fp32 one (the bf16 forward really ran, and its
    BFloat16 maps reached numpy widened); the default is the fp32 path, the same mosaic every time."""
    s = SEEDS[0]
    assert oracle["b16"][s].dtype == np.uint16 and oracle["b16"][s].shape == (3, H, W)
    assert (oracle["b16"][s] != oracle["f32"][s]).any()
    assert np.array_equal(_run(oracle["model"], oracle["scenes"][s], autocast=False), oracle["f32"][s])


def test_yardstick_is_steady_between_scenes(oracle):
    a, b = (oracle["yardstick"][s] for s in SEEDS)
    r = P.ratios(a, b)
    print("yardstick, scene", SEEDS[0], a.round(1).tolist(), "scene", SEEDS[1], b.round(1).tolist())
    print("ratio scene to scene", r.round(2).tolist())
    assert (r < P.MARGIN).all() and (1.0 / r < P.MARGIN).all(), r


def _mutant_ratios(oracle, what, mutate):
    """The nine ratios of |mutated fp32 oracle - fp32 oracle| to the yardstick on the first scene."""
    s = SEEDS[0]
    m = copy.deepcopy(oracle["model"])
    with torch.no_grad():
        mutate(dict(m.named_modules()), m)
    r = P.ratios(P.band_stats(_run(m, oracle["scenes"][s]), oracle["f32"][s]), oracle["yardstick"][s])
    print(f"{what}: ratios to the yardstick {r.round(2).tolist()}")
    return r


def _drop_last_tap(name):
    def mutate(layers, m):
        layers[name].weight[:, :, 2, 2] = 0.0
    return mutate


def _roll_input_channels(name):
    def mutate(layers, m):
        w = layers[name].weight
        w.copy_(w.roll(1, dims=1))
    return mutate


@pytest.mark.parametrize("what,mutate", [("last tap dropped", _drop_last_tap(MID_CONV)),
                                         ("input channels rolled by one", _roll_input_channels(MID_CONV))])
def test_mid_network_conv_errors_exceed_the_bound_in_every_band(oracle, what, mutate):
    r = _mutant_ratios(oracle, f"{MID_CONV} {what}", mutate)
    assert (r.max(axis=1) > P.MARGIN).all(), r
    with pytest.raises(AssertionError):  # and the helper the GPU tests call refuses it
        P.assert_within_spread(what, r * oracle["yardstick"][SEEDS[0]], oracle["yardstick"][SEEDS[0]])


def test_final_conv_dropped_tap_exceeds_the_bound_on_edge_and_crop(oracle):
    r = _mutant_ratios(oracle, f"{FINAL_CONV} last tap dropped", _drop_last_tap(FINAL_CONV))
    assert (r[1:].max(axis=1) > P.MARGIN).all(), r


def test_blind_spots_of_the_whole_model_bound(oracle):
    """Documented, not wished for: these two errors are smaller than the reference's own bf16 rounding noise, so no
    whole-model mixed-precision test can see them. The exact per-kernel suites (BatchNorm against float64) do."""
    def eps(layers, m):
        for mod in m.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                assert mod.eps == 1e-5
                mod.eps = 1e-3

    def var(layers, m):
        layers[MID_BN].running_var.mul_(1.1)

    for what, mutate in (("BatchNorm eps 1e-3 everywhere", eps), (f"{MID_BN} running_var x 1.1", var)):
        r = _mutant_ratios(oracle, what, mutate)
        assert (r > 0).all() and (r <= P.MARGIN).all(), (what, r)
