"""Mixed precision for the two constructor variants with their own bf16 kernels: attention_weights="spatial_channel"
and pool_by_max=True -- the reference's default precision ("16-mixed", model.py:86,168-186) with its CLI options
--attention-weights spatial_channel / --pool-by-max.

Fixtures tests/golden/train_bf16_{h8_b2_28_sca, h8_b2_28_poolmax, h32_b4_100_sca}.npz (tools/make_bf16_variant_golden.py)
hold the reference's training step under torch.autocast(bfloat16) and its fp32 step on the same seeded weights / inputs.
Criteria, stated against the fp32 reference (the ground truth both mixed-precision runs approximate):
    probability maps   mean |d| <= 6e-3, max |d| <= 8e-2, and mean no worse than 1.5x the reference's own bf16 deviation
    > 0.5 masks        identical wherever the fp32 probability is farther than 8e-2 from 0.5; overall agreement no worse
                       than the reference's own bf16 run minus 1 %
    loss               |d| <= 5e-4
    gradient norms     median relative deviation <= 1e-2, 90th percentile <= 6e-2, median <= 1.5x the reference's
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("distance", "edge", "crop")
VARIANTS = {"sca": {"attention_weights": "spatial_channel"}, "poolmax": {"pool_by_max": True}}


def _variant(name):
    return VARIANTS[name.rsplit("_", 1)[1]]


def _setup(g, kw):
    from cultionet_amd.data import Data
    from oracle import towerunet_oracle as O
    from oracle.selfcheck import build_pair

    hidden, B, H, W, with_mask, seed = (int(v) for v in g["meta"])
    lit, _ = build_pair(hidden=hidden, device="cuda:0", **kw)
    x, y, bdist = O.seeded_batch(B, height=H, width=W, seed=seed, with_mask=bool(with_mask))
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bdist.cuda(), lon=torch.zeros(B).cuda(), lat=torch.zeros(B).cuda())
    return lit, batch


def _check_maps(p, g, k):
    f32 = g["fp32_" + k]
    d32 = np.abs(p - f32)
    dref = np.abs(g[k] - f32)
    assert d32.mean() <= 6e-3 and d32.max() <= 8e-2, (k, d32.mean(), d32.max())
    assert d32.mean() <= 1.5 * dref.mean() + 1e-4, (k, d32.mean(), dref.mean())
    clear = np.abs(f32 - 0.5) > 8e-2
    assert np.array_equal((p > 0.5)[clear], (f32 > 0.5)[clear]), k
    agree = float(((p > 0.5) == (f32 > 0.5)).mean())
    agree_ref = float(((g[k] > 0.5) == (f32 > 0.5)).mean())
    assert agree >= agree_ref - 0.01, (k, agree, agree_ref)


@pytest.mark.parametrize("name", ["train_bf16_h8_b2_28_sca", "train_bf16_h8_b2_28_poolmax",
                                  "train_bf16_h32_b4_100_sca"])
def test_bf16_variant_train_step_matches_reference(golden_dir, name):
    from cultionet_amd import engine as E
    from cultionet_amd.lightning import HipTrainer

    g = np.load(os.path.join(golden_dir, name + ".npz"))
    lit, batch = _setup(g, _variant(name))
    lit.train()
    trainer = HipTrainer(lit, precision="16-mixed")
    assert trainer.bf16
    model = lit.cultionet_model.mask_model
    store = model.param_store()
    with E.using_store(store), E.recording(False), E.mixed_precision(True):
        outs = model.forward_vars(model.input_var(batch.x))
    for k in KEYS:
        assert outs[k].t.dtype == torch.float32
        _check_maps(outs[k].t.float().cpu().numpy(), g, k)
    loss = trainer.forward_backward(batch)
    torch.cuda.synchronize()
    assert abs(float(loss.item()) - float(g["fp32_loss"])) <= 5e-4, (float(loss.item()), float(g["fp32_loss"]))
    norms = {n: float(trainer.store.grad_of(p).double().norm()) for n, p in model.named_parameters()}
    rel = np.array([abs(norms[str(n)] - r) / max(abs(r), 1e-4) for n, r in zip(g["grad_names"], g["fp32_grad_norms"])])
    relref = np.abs(g["grad_norms"] - g["fp32_grad_norms"]) / np.maximum(np.abs(g["fp32_grad_norms"]), 1e-4)
    assert np.median(rel) <= 1e-2 and np.percentile(rel, 90) <= 6e-2, (np.median(rel), np.percentile(rel, 90))
    assert np.median(rel) <= 1.5 * np.median(relref) + 1e-3, (np.median(rel), np.median(relref))
    if "sca" in name:  # the attention path carries gradient (gamma, the channel MLPs, the spatial 3x3 conv)
        for n in g["grad_names"]:
            if "attention_conv" in str(n) and not str(n).endswith("bias"):
                assert norms[str(n)] > 0.0, n
    trainer.optimizer_step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in model.parameters())


@pytest.mark.parametrize("variant", ["sca", "poolmax"])
def test_16_mixed_trainer_tracks_fp32_and_trains(variant):
    """HipTrainer(precision="16-mixed") on each variant: six steps track the model's own fp32 path to 2e-2 and the
    loss goes down."""
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import HipTrainer
    from oracle import towerunet_oracle as O
    from oracle.selfcheck import build_pair

    x, y, bdist = O.seeded_batch(4, height=50, width=50, seed=3, with_mask=True)
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bdist.cuda())
    losses = {}
    for prec in ("32-true", "16-mixed"):
        lit, _ = build_pair(hidden=16, device="cuda:0", **VARIANTS[variant])
        lit.train()
        tr = HipTrainer(lit, precision=prec)
        losses[prec] = [float(tr.training_step(batch).item()) for _ in range(6)]
    a, b = np.array(losses["32-true"]), np.array(losses["16-mixed"])
    assert np.isfinite(b).all(), b
    assert np.abs(a - b).max() <= 2e-2, (a, b)
    assert b[-1] < b[0] - 1e-3, b


@pytest.mark.parametrize("variant", ["sca", "poolmax"])
def test_16_mixed_replay_with_dropout(variant):
    """replay=True with dropout 0.1 records a launch plan whose steps follow the eager steps (same seed, so the same
    masks; the two trainers run in separate phases as they share the process-wide seed state). Hidden 24: decoder
    widths of 96, a multiple of 8 but not 8 * 2^n."""
    from cultionet_amd import engine as E
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    batches = []
    for k in range(3):
        x, y, bd = S.seeded_batch(2, height=28, width=28, seed=50 + k, with_mask=True)
        batches.append(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()))
    runs = {}
    for replay in (False, True):
        lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=24, dropout=0.1, **VARIANTS[variant])
        m = lit.cultionet_model.mask_model
        m.load_state_dict(S.seeded_state_dict(m.state_dict()))
        lit = lit.to("cuda:0").train()
        tr = HipTrainer(lit, precision="16-mixed", replay=replay)
        assert tr.bf16
        E.manual_seed(1234)
        runs[replay] = [float(tr.training_step(batches[i % 3]).item()) for i in range(6)]
        if replay:
            assert tr._plan is not None and tr._plan.n_calls > 100  # the later steps ran from the recorded plan
    le, lp = np.array(runs[False]), np.array(runs[True])
    assert np.isfinite(le).all() and np.isfinite(lp).all(), (le, lp)
    assert np.abs(le - lp).max() <= 2e-3, (le, lp)


@pytest.mark.parametrize("name", ["train_bf16_h8_b2_28_sca", "train_bf16_h8_b2_28_poolmax"])
def test_dropin_autocast_matches_native_bf16_step(golden_dir, name):
    """The drop-in surface: forward(Data) under torch.autocast(bfloat16), calc_loss, loss.backward() -- the loss matches
    the native bf16 step's to 5e-4 and every parameter gets a finite gradient."""
    from cultionet_amd.lightning import HipTrainer

    g = np.load(os.path.join(golden_dir, name + ".npz"))
    kw = _variant(name)
    lit, batch = _setup(g, kw)
    lit.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred = lit(batch)
        loss, _ = lit.calc_loss(batch, pred)
    loss.backward()
    model = lit.cultionet_model.mask_model
    grads = [p.grad for p in model.parameters()]
    assert all(gr is not None and torch.isfinite(gr).all() for gr in grads)
    assert sum(float(gr.abs().sum()) for gr in grads) > 0.0
    lit2, batch2 = _setup(g, kw)
    lit2.train()
    native = float(HipTrainer(lit2, precision="bf16-mixed").forward_backward(batch2).item())
    assert abs(float(loss) - native) <= 5e-4, (float(loss), native)
    assert abs(float(loss) - float(g["fp32_loss"])) <= 5e-4


def test_predictor_16_mixed_for_both_variants():
    """SlidingWindowPredictor(precision="16-mixed") on a small raw scene: within the bf16 map tolerance of the fp32
    predictor for an SCA model and a max-pool model, and within 1.5 x the spread of the reference's own bf16 run
    (the oracle built with the variant's arguments, tests/predict_bound_ref.py) in every band and statistic."""
    import predict_bound_ref as P
    from cultionet_amd.predict import SlidingWindowPredictor
    from oracle import predict_ref
    from oracle import towerunet_oracle as O
    from oracle.make_golden import calibrate_bn
    from oracle.selfcheck import build_pair

    H, W, ws, pad = 70, 95, 40, 4
    g = torch.Generator().manual_seed(5)
    scene = torch.randint(0, 9000, (3, 12, H, W), generator=g, dtype=torch.int32).to(torch.int16).cuda()
    mean = torch.tensor([0.31, 0.28, 0.35])
    std = torch.tensor([0.21, 0.19, 0.24])
    kw = dict(window_size=ws, padding=pad, batch_size=3, mean=mean, std=std)
    for variant in ("sca", "poolmax"):
        lit, ref = build_pair(hidden=8, **VARIANTS[variant])
        xc, _, _ = O.seeded_batch(2, height=28, width=28, seed=77)
        calibrate_bn(ref, lambda: ref(xc))
        lit.cultionet_model.mask_model.load_state_dict(ref.state_dict())
        f32 = SlidingWindowPredictor(lit, **kw).predict_scene(scene).cpu().numpy().astype(np.int64)
        b16 = SlidingWindowPredictor(lit, precision="16-mixed", **kw).predict_scene(scene).cpu().numpy().astype(np.int64)
        d = np.abs(f32 - b16)
        assert b16.shape == (3, H, W) and b16.max() <= 10000, variant
        print(f"16-mixed {variant} against the fp32 path: max {d.max()}, mean {d.mean():.2f}")
        assert d.max() <= 800 and d.mean() <= 60, (variant, d.max(), d.mean())  # 8e-2 max, 6e-3 mean in probability
        assert (b16 != f32).any(), variant  # the bf16 path really ran
        # and no further from it than 1.5 x what the reference's own bf16 run of THIS variant moves its fp32 mosaic
        s = scene.cpu().numpy().astype(np.float64)
        want = predict_ref.predict_scene(ref, s, ws, pad, mean.numpy(), std.numpy())
        cast = predict_ref.predict_scene(ref, s, ws, pad, mean.numpy(), std.numpy(), autocast=True)
        P.assert_within_spread(f"predict 16-mixed {variant} vs the fp32 path", P.band_stats(b16, f32),
                               P.band_stats(cast, want))
