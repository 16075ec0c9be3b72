"""SURVEY 8(f)-2/3 and BASELINE configs[4]: collate + device prologue, and sliding-window scene prediction against the
CPU restatement oracle/predict_ref.py (the reference's predict path needs the GIS stack: restatement-checked)."""
import numpy as np
import pytest
import torch

import predict_bound_ref as P

pytestmark = pytest.mark.gpu


def _pair(hidden=8, C=3, Tn=12):
    from oracle.make_golden import calibrate_bn
    from oracle.selfcheck import build_pair
    from oracle import towerunet_oracle as O

    lit, ref = build_pair(hidden=hidden, in_channels=C, in_time=Tn)
    xc, _, _ = O.seeded_batch(2, channels=C, time=Tn, height=28, width=28, seed=77)
    calibrate_bn(ref, lambda: ref(xc))
    lit.cultionet_model.mask_model.load_state_dict(ref.state_dict())
    return lit, ref


@pytest.mark.parametrize("H,W,ws,pad", [(70, 95, 40, 4), (64, 64, 32, 6), (50, 41, 64, 5)])
def test_sliding_window_predict_matches_restatement(H, W, ws, pad):
    from cultionet_amd.predict import SlidingWindowPredictor
    from oracle import predict_ref

    lit, ref = _pair()
    g = torch.Generator().manual_seed(H * 131 + W)
    scene = torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16)
    mean = torch.tensor([0.31, 0.28, 0.35])
    std = torch.tensor([0.21, 0.19, 0.24])
    want = predict_ref.predict_scene(ref, scene.numpy().astype(np.float64), ws, pad, mean.numpy(), std.numpy())
    pred = SlidingWindowPredictor(lit, window_size=ws, padding=pad, batch_size=3, mean=mean, std=std)
    got = pred.predict_scene(scene.cuda()).cpu().numpy().astype(np.int64)
    d = np.abs(got - want.astype(np.int64))
    # probabilities agree to ~1e-5 (x10000 = 0.1 count): a count flips only when a value straddles an integer
    assert d.max() <= 2, d.max()
    assert (d > 0).mean() <= 0.05, (d > 0).mean()
    assert got.shape == (3, H, W) and got.max() <= 10000


def _yardstick(ref, scene, ws, pad, mean, std):
    """(the oracle's fp32 mosaic, the reference's own bf16 spread on this scene): the nine statistics of
    |oracle under CPU bf16 autocast - oracle fp32| (tests/predict_bound_ref.py), computed on the CPU."""
    from oracle import predict_ref

    s = scene.cpu().numpy().astype(np.float64)
    want = predict_ref.predict_scene(ref, s, ws, pad, mean.numpy(), std.numpy())
    cast = predict_ref.predict_scene(ref, s, ws, pad, mean.numpy(), std.numpy(), autocast=True)
    return want, P.band_stats(cast, want)


def test_sliding_window_predict_bf16_mixed():
    """precision="bf16-mixed" (the reference's default predict precision is 16-mixed): the same mosaic as the fp32 path
    within 1.5 x the reference's own bf16 spread on this scene, for the mean, the 99.9th percentile and the max of every
    band (the margin test_bf16_train_step_matches_reference gives), and a mean of at most 60 counts (6e-3).

    A cap of 400 counts on the max stood here and failed at 431: the reference's own bf16 run of this scene moves the
    fp32 mosaic by up to 484 counts, so that cap asked more of the kernels than the reference delivers."""
    from cultionet_amd.predict import SlidingWindowPredictor

    lit, ref = _pair()
    H, W, ws, pad = 70, 95, 40, 4
    g = torch.Generator().manual_seed(5)
    scene = torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16).cuda()
    mean = torch.tensor([0.31, 0.28, 0.35])
    std = torch.tensor([0.21, 0.19, 0.24])
    _, yard = _yardstick(ref, scene, ws, pad, mean, std)
    kw = dict(window_size=ws, padding=pad, batch_size=3, mean=mean, std=std)
    f32 = SlidingWindowPredictor(lit, **kw).predict_scene(scene).cpu().numpy().astype(np.int64)
    b16 = SlidingWindowPredictor(lit, precision="bf16-mixed", **kw).predict_scene(scene).cpu().numpy().astype(np.int64)
    d = np.abs(f32 - b16)
    assert b16.shape == (3, H, W) and b16.max() <= 10000
    print(f"bf16-mixed against the fp32 path: max {d.max()}, mean {d.mean():.2f}")
    P.assert_within_spread("predict bf16-mixed vs the fp32 path", P.band_stats(b16, f32), yard)
    assert d.mean() <= 60, d.mean()
    assert (b16 != f32).any()  # the bf16 path really ran
    with pytest.raises(ValueError):
        SlidingWindowPredictor(lit, precision="fp8")


@pytest.mark.parametrize("pack", [0, 400_000])
def test_sliding_window_predict_bf16_mixed_vs_restatement(pack):
    """The `predict` headline path -- precision="bf16-mixed", fused inference ConvBlock2d, launch-plan replay, packed
    batches -- against the CPU restatement of the reference's predict path (oracle/predict_ref.py, fp32), not against
    the repo's own fp32 mosaic: <= 400 counts max (4e-2 in probability), mean <= 60 counts (6e-3), and every one of
    the nine band statistics within 1.5 x the reference's own bf16 spread on this scene."""
    from cultionet_amd.predict import SlidingWindowPredictor

    lit, ref = _pair()
    H, W, ws, pad = 70, 95, 40, 4
    g = torch.Generator().manual_seed(H * 131 + W)
    scene = torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16)
    mean = torch.tensor([0.31, 0.28, 0.35])
    std = torch.tensor([0.21, 0.19, 0.24])
    want, yard = _yardstick(ref, scene, ws, pad, mean, std)
    sp = SlidingWindowPredictor(lit, window_size=ws, padding=pad, batch_size=3, mean=mean, std=std,
                                precision="bf16-mixed", pixels_per_launch=pack)
    for call in range(2):  # second call: the recorded launch plan is replayed
        got = sp.predict_scene(scene.cuda()).cpu().numpy().astype(np.int64)
        d = np.abs(got - want.astype(np.int64))
        assert got.shape == (3, H, W) and got.max() <= 10000
        print(f"bf16-mixed pack {pack} call {call} against the fp32 restatement: max {d.max()}, mean {d.mean():.2f}")
        assert d.max() <= 400, d.max()
        assert d.mean() <= 60, d.mean()
        P.assert_within_spread(f"predict bf16-mixed pack {pack} call {call} vs the fp32 restatement",
                               P.band_stats(got, want), yard)


def _prologue_ref(raw, mean, std):
    """tests/pointwise_ref.prepare_chips_ref at the prologue's constants, as a CPU tensor."""
    import pointwise_ref as R

    as_np = lambda t: None if t is None else t.cpu().numpy()
    return torch.from_numpy(R.prepare_chips_ref(as_np(raw), as_np(mean), as_np(std), 1.0 / 10_000.0, 1e-9, 1.0))


def test_collate_and_device_prologue():
    from cultionet_amd.data import Data, collate_fn
    from cultionet_amd.lightning import CultionetLitModel

    g = torch.Generator().manual_seed(3)
    samples = []
    for i in range(3):
        samples.append(Data(x=torch.randint(0, 9000, (1, 3, 12, 20, 20), generator=g, dtype=torch.int32),
                            y=torch.randint(-1, 3, (1, 20, 20), generator=g),
                            bdist=torch.randint(0, 10000, (1, 20, 20), generator=g, dtype=torch.int32),
                            train_id=[f"s{i}"], lon=torch.zeros(1), extra=None, arr=np.array([i])))
    batch = collate_fn(samples)
    assert batch.x.shape == (3, 3, 12, 20, 20) and batch.train_id == ["s0", "s1", "s2"] and batch.extra is None
    assert np.array_equal(batch.arr, np.array([0, 1, 2])) and batch.num_samples == 3
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0).to("cuda:0")
    mean, std = torch.tensor([0.3, 0.25, 0.4]), torch.tensor([0.2, 0.15, 0.3])
    lit.set_norm_values(mean, std)
    dev = batch.to("cuda:0")
    out = lit.on_after_batch_transfer(dev)
    want = ((batch.x.float() / 10000.0).clip(1e-9, 1) - mean.view(1, 3, 1, 1, 1)) / std.view(1, 3, 1, 1, 1)
    assert (out.x.cpu() - want).abs().max() <= 1e-6
    wb = (batch.bdist.float() / 10000.0).clip(1e-9, 1)
    assert (out.bdist.cpu() - wb).abs().max() <= 1e-7
    # and bit for bit the kernel's own arithmetic (tests/pointwise_ref.py), which every augmenter test builds on
    assert torch.equal(out.x.cpu(), _prologue_ref(batch.x, mean, std))
    assert torch.equal(out.bdist.cpu(), _prologue_ref(batch.bdist.unsqueeze(1), None, None).squeeze(1))
    pred = lit.eval()(out)  # the prepared batch feeds the forward
    assert pred["distance"].shape == (3, 1, 20, 20)


def test_device_feeder_double_buffers_raw_batches():
    """cultionet_amd.feeder.DeviceFeeder: raw int16 batches in pinned host memory -> copy stream -> cn_prepare_chips_f32
    -> the consumer's stream. Every yielded batch equals the reference arithmetic (datasets.py:443-446 +
    normalize.py:63-82: x / 10000 -> clip(1e-9, 1) -> z-score) of ITS host batch, also when the consumer is slow or
    fast relative to the copies (ordering is by stream events, not by luck)."""
    from cultionet_amd.data import Data
    from cultionet_amd.feeder import DeviceFeeder, pin_batch

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    mean = torch.rand(3, generator=g) * 0.3
    std = torch.rand(3, generator=g) * 0.2 + 0.05
    hosts = []
    for k in range(5):
        xr = torch.randint(-20, 11000, (4, 3, 6, 20, 24), generator=g).to(torch.int16)
        y = torch.randint(-1, 3, (4, 20, 24), generator=g)
        bd = torch.randint(0, 10001, (4, 20, 24), generator=g).to(torch.int16)
        hosts.append(pin_batch(Data(x=xr, y=y, bdist=bd)))
    feeder = DeviceFeeder(dev, mean=mean, std=std)
    burn = torch.empty(4096, 4096, device=dev)
    seen = 0
    for i, b in enumerate(feeder.iterate(hosts)):
        if i % 2 == 0:
            for _ in range(20):  # a slow consumer: the next batch's copy + prologue overlap this
                burn.normal_()
        h = hosts[i]
        ref = (h.x.float() / 10_000.0).clip(1e-9, 1)
        ref = (ref - mean.view(1, 3, 1, 1, 1)) / std.view(1, 3, 1, 1, 1)
        assert b.x.dtype == torch.float32 and b.x.is_cuda
        assert (b.x.cpu() - ref).abs().max() <= 1e-5
        assert torch.equal(b.y.cpu(), h.y)
        assert (b.bdist.cpu() - (h.bdist.float() / 10_000.0).clip(1e-9, 1)).abs().max() <= 1e-6
        assert torch.equal(b.x.cpu(), _prologue_ref(h.x, mean, std))
        assert torch.equal(b.bdist.cpu(), _prologue_ref(h.bdist.unsqueeze(1), None, None).squeeze(1))
        seen += 1
    assert seen == len(hosts)
    assert list(feeder.iterate([])) == []


@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed"])
def test_launch_plan_replay_is_bitwise_the_eager_forward(precision):
    """cultionet_amd/replay.py: the recorded launch plan of the eval forward replays the SAME kernels on the same
    buffers -- mosaics are bit-identical to the eager path, for new scene data, for the ragged last batch (its own
    plan), and plans are dropped when the parameters or the BatchNorm running statistics change."""
    from cultionet_amd.predict import SlidingWindowPredictor

    lit, _ = _pair()
    model = lit.cultionet_model.mask_model
    H, W, ws, pad = 70, 95, 32, 4   # 3 x 3 = 9 windows, batches of 4 -> 4, 4, 1
    g = torch.Generator().manual_seed(9)
    mean = torch.tensor([0.31, 0.28, 0.35])
    std = torch.tensor([0.21, 0.19, 0.24])
    kw = dict(window_size=ws, padding=pad, batch_size=4, mean=mean, std=std, precision=precision,
              pixels_per_launch=0)  # batches as given: this test wants the ragged last batch
    eager = SlidingWindowPredictor(lit, replay=False, **kw)
    plan = SlidingWindowPredictor(lit, replay=True, **kw)
    for rep in range(3):
        scene = torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16).cuda()
        a = eager.predict_scene(scene)
        b = plan.predict_scene(scene)
        assert torch.equal(a, b), rep
    plans = model.__dict__["_cn_plans"]
    assert len(plans) == 2 and all(len(p.calls) > 50 for p in plans.values())  # full batches and the ragged last one
    assert model.replay is False  # the predictor restores the switch
    # parameters change -> the old plan must not be replayed
    with torch.no_grad():
        for p in model.final_a.parameters():
            p.mul_(1.5)
    a = eager.predict_scene(scene)
    b = plan.predict_scene(scene)
    assert torch.equal(a, b)
    # running statistics change (train-mode forward through the HIP kernels) -> same
    lit.train()
    with torch.no_grad():
        model(torch.rand(2, 3, 12, 28, 28, device="cuda"))
    lit.eval()
    a2 = eager.predict_scene(scene)
    b2 = plan.predict_scene(scene)
    assert torch.equal(a2, b2) and not torch.equal(a2, a)


@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed"])
def test_packed_window_batches_give_the_same_mosaic(precision):
    """pixels_per_launch (default 400k): consecutive batches of ``batch_size`` windows are packed into one forward. The
    eval forward is independent per window, so the mosaic is the one the reference's loop granularity gives (fp32: the
    launch-cost model may pick another K split for another batch size -> last-bit differences, at most one count)."""
    from cultionet_amd.predict import SlidingWindowPredictor

    lit, _ = _pair()
    H, W, ws, pad = 70, 95, 32, 4   # 9 windows: 4 + 4 + 1 as given, one launch of 9 when packed
    g = torch.Generator().manual_seed(21)
    scene = torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16).cuda()
    kw = dict(window_size=ws, padding=pad, batch_size=4, precision=precision)
    given = SlidingWindowPredictor(lit, pixels_per_launch=0, **kw)
    packed = SlidingWindowPredictor(lit, **kw)
    assert given.launch_bs == 4 and packed.launch_bs == 250  # 400k / 40^2
    a = given.predict_scene(scene).cpu().numpy().astype(np.int64)
    b = packed.predict_scene(scene).cpu().numpy().astype(np.int64)
    d = np.abs(a - b)
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (d.max(), (d > 0).mean())
    # a large window keeps the caller's batch size: 266^2 padded pixels -> 6 windows per launch, never fewer than asked
    assert SlidingWindowPredictor(lit, window_size=256, padding=5, batch_size=8).launch_bs == 8
    assert SlidingWindowPredictor(lit, window_size=256, padding=5, batch_size=2).launch_bs == 6
