"""The device augmentation stage (cn_augment_chips_f32, cultionet_amd.augment) against the float64 restatement
tests/augment_ref.py (itself pinned to torch and to the reference's Perlin generator by tests/test_augment_ref.py),
under hand-built plans.

Conditions:
* labels, and the flips / rotations of x and bdist, match EXACTLY (torch.equal; for x and bdist against the same
  permutation of what cn_prepare_chips_f32 gives); `none` samples and a whole batch at augment_prob = 0 equal
  cn_prepare_chips_f32 bit for bit;
* interpolated, blurred and noisy outputs: |d| <= 2e-6 / std[c]. Before the z-score every value lies in [0, 1], where one
  fp32 rounding is at most 6e-8; each op is under about a dozen roundings, and the noise term is bounded by
  0.01 * 5.8 through logf / sqrtf / cosf accurate to a few ulp;
* at most two launches per apply().

Shapes: 20 x 20 (one sample per op), 13 x 13 (odd, a 3-pixel crop at div 4; u16, i32 and f32), 10 x 28 (non-square) and
40 x 40 (two row bands per plane, two rotation tiles per band, a blur halo that crosses the band edge)."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-6
PERMUTATIONS = ("rot90", "rot180", "rot270", "fliplr", "flipud")
EDGE = 3  # the edge class of the labels below: y in {-1, 0, 1, 2, EDGE}
MEAN = {1: [0.27], 2: [0.31, 0.22], 3: [0.3, 0.25, 0.4]}
STD = {1: [0.21], 2: [0.17, 0.09], 3: [0.2, 0.15, 0.3]}


def _raw(B, C, T, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lo = 0 if dtype == torch.uint16 else -20
    x = torch.randint(lo, 11000, (B, C, T, H, W), generator=g)  # below 0 and above 10000: both clips are exercised
    bd = torch.randint(0, 10001, (B, H, W), generator=g)
    y = torch.randint(-1, EDGE + 1, (B, H, W), generator=g)
    y[:, 0, 0], y[:, 0, 1], y[:, 1, 0], y[:, -1, -1] = -1, 0, 1, EDGE
    if dtype == torch.float32:
        x = x.float() + torch.rand(x.shape, generator=g)
        bd = bd.float() + torch.rand(bd.shape, generator=g)
    return x.to(dtype), bd.to(dtype), y


def _angles(r, seed):
    a = (2 * np.pi * np.random.default_rng(seed).random((2, 2, r + 1, r + 1))).astype(np.float32)
    return a[0], a[1]


def _plan(entries):
    from cultionet_amd.augment import AugmentPlan

    plan = AugmentPlan(len(entries))
    for b, e in enumerate(entries):
        plan.set(b, e["op"], **{k: v for k, v in e.items() if k != "op"})
    return plan


def _entries(ops, H, W, seed=0):
    """One entry per name; 'cropresize4' / 'cropresize2' and 'perlin2' / 'perlin5' / 'perlin10' carry their parameter."""
    g = np.random.default_rng(1000 + seed)
    out = []
    for k, name in enumerate(ops):
        if name.startswith("cropresize"):
            div = int(name[len("cropresize"):])
            h, w = H // div, W // div
            # the last crop of a list sits in the bottom-right corner: the largest offsets that are still inside
            top, left = (H - h, W - w) if k == len(ops) - 1 else (int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1)))
            out.append({"op": "cropresize", "div": div, "top": top, "left": left})
        elif name.startswith("perlin"):
            r = int(name[len("perlin"):])
            th, ph = _angles(r, seed + r)
            out.append({"op": "perlin", "r": r, "theta": th, "phi": ph})
        elif name == "gaussian":
            out.append({"op": name, "sigma": float(np.float32(g.uniform(0.2, 0.5)))})
        elif name == "saltpepper":
            out.append({"op": name, "seed": int(g.integers(0, 2 ** 63)) | (1 << 63)})  # a full 64-bit seed
        else:
            out.append({"op": name})
    return out


def _launches():
    from cultionet_amd import _lib

    return _lib.query("cn_launch_count", 0)


def _check(C, T, H, W, dtype, ops, seed):
    """Runs apply() under the plan of `ops` and checks every output against the restatement and the exact conditions."""
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import prepare_chips

    B = len(ops)
    x, bd, y = _raw(B, C, T, H, W, dtype, seed)
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])
    entries = _entries(ops, H, W, seed)
    plan = _plan(entries)
    assert [e["op"] for e in R.entries_of(plan)] == [e["op"] for e in entries]
    aug = DeviceAugmenter()
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda(), lon=torch.zeros(B))
    torch.cuda.synchronize()
    n0 = _launches()
    out = aug.apply(batch, mean, std, plan=plan)
    assert _launches() - n0 <= 2
    plain_x = prepare_chips(batch.x, mean, std).cpu()
    plain_bd = prepare_chips(batch.bdist.reshape(B, 1, 1, H, W)).reshape(B, H, W).cpu()
    gx, gb, gy = out.x.cpu(), out.bdist.cpu(), out.y.cpu()
    assert gx.dtype == torch.float32 and gb.dtype == torch.float32 and gy.dtype == torch.int64
    assert gx.shape == x.shape and torch.equal(out.lon, batch.lon)

    wx, wb, wy = R.pipeline(x.double().numpy(), bd.double().numpy(), y.numpy(), R.entries_of(plan), MEAN[C], STD[C])
    assert torch.equal(gy, torch.from_numpy(wy))
    bound = TOL / np.asarray(STD[C]).reshape(1, C, 1, 1, 1)
    ex = np.abs(gx.double().numpy() - wx)
    eb = np.abs(gb.double().numpy() - wb)
    for b, e in enumerate(entries):
        print(f"{H}x{W} {dtype} {e['op']:>10}: x err/bound {(ex[b] / bound[0]).max():.3f}  bdist err {eb[b].max():.2e}")
    assert (ex <= bound).all(), [(e["op"], float((ex[b] / bound[0]).max())) for b, e in enumerate(entries)]
    assert eb.max() <= TOL
    for b, e in enumerate(entries):
        op = e["op"]
        if op == "none":
            assert torch.equal(gx[b], plain_x[b]) and torch.equal(gb[b], plain_bd[b]) and torch.equal(gy[b], y[b])
        elif op in PERMUTATIONS:
            fn = {"rot90": lambda a: torch.rot90(a, 1, (-2, -1)), "rot180": lambda a: torch.rot90(a, 2, (-2, -1)),
                  "rot270": lambda a: torch.rot90(a, 3, (-2, -1)), "fliplr": lambda a: torch.flip(a, (-1,)),
                  "flipud": lambda a: torch.flip(a, (-2,))}[op]
            assert torch.equal(gx[b], fn(plain_x[b])), op
            assert torch.equal(gb[b], fn(plain_bd[b])), op
            assert torch.equal(gy[b], fn(y[b])), op
        elif op in R.X_ONLY:
            assert torch.equal(gb[b], plain_bd[b]) and torch.equal(gy[b], y[b]), op
            assert not torch.equal(gx[b], plain_x[b]), op
        else:
            assert set(gy[b].unique().tolist()) <= set(y[b].unique().tolist())
    return out


def test_all_ops_batch():
    """B = 10, C = 2, T = 3, H = W = 20, int16: one sample per op, and `none`."""
    ops = ("rot90", "gaussian", "none", "perlin5", "fliplr", "saltpepper", "rot270", "cropresize4", "flipud", "rot180")
    _check(2, 3, 20, 20, torch.int16, ops, seed=1)
    _check(1, 2, 20, 20, torch.int16, ("perlin2", "perlin10", "cropresize2"), seed=2)


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int32, torch.float32], ids=["u16", "i32", "f32"])
def test_square_odd_plane(dtype):
    """H = W = 13: a 3-pixel crop at div 4, reflect halos and rotation tiles that end inside a tile."""
    ops = ("fliplr", "flipud", "rot90", "rot180", "rot270", "gaussian", "saltpepper", "cropresize2", "none", "cropresize4")
    _check(3, 2, 13, 13, dtype, ops, seed=3)


def test_non_square_plane():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data

    ops = ("fliplr", "flipud", "rot180", "cropresize2", "gaussian", "perlin2", "none", "cropresize4")
    _check(2, 3, 10, 28, torch.int16, ops, seed=4)
    x, bd, y = _raw(2, 2, 3, 10, 28, torch.int16, 5)
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    n0 = _launches()
    with pytest.raises(ValueError):
        DeviceAugmenter().apply(batch)  # rot90 / rot270 are enabled by default
    with pytest.raises(ValueError):
        DeviceAugmenter().apply(batch, plan=_plan([{"op": "none"}, {"op": "rot90"}]))
    assert _launches() == n0
    names = ("fliplr", "flipud", "rot180", "gaussian", "saltpepper", "cropresize", "perlin")
    out = DeviceAugmenter(augment_prob=1.0, augmentations=names).apply(batch)
    assert torch.isfinite(out.x).all()


def test_two_row_bands():
    """H = W = 40: two bands of output rows per plane (the second one short), two rotation tiles per band, a blur halo
    that crosses the band edge, crops and Perlin cells that straddle it."""
    ops = ("rot90", "rot270", "gaussian", "cropresize4", "perlin2", "perlin5", "perlin10", "saltpepper", "rot180",
           "fliplr", "flipud", "none", "cropresize2")
    _check(1, 2, 40, 40, torch.int16, ops, seed=6)


def test_label_dtypes_and_missing_bdist():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data

    ops = ("rot90", "cropresize2", "flipud", "none")
    x, bd, y = _raw(4, 1, 2, 20, 20, torch.int16, 7)
    plan = _plan(_entries(ops, 20, 20, 7))
    want = DeviceAugmenter().apply(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()), plan=plan)
    for dt in (torch.int16, torch.int32):
        got = DeviceAugmenter().apply(Data(x=x.cuda(), y=y.to(dt).cuda(), bdist=bd.cuda()), plan=plan)
        assert got.y.dtype == torch.int64 and torch.equal(got.y, want.y) and torch.equal(got.x, want.x)
    got = DeviceAugmenter().apply(Data(x=x.cuda(), y=y.cuda()), plan=plan)
    assert torch.equal(got.y, want.y) and torch.equal(got.x, want.x) and not hasattr(got, "bdist")


def test_augment_prob_zero_and_unlabelled_batches_are_the_plain_prologue():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import prepare_chips

    x, bd, y = _raw(3, 3, 4, 20, 24, torch.int16, 8)
    mean, std = torch.tensor(MEAN[3]), torch.tensor(STD[3])
    px = prepare_chips(x.cuda(), mean, std)
    pb = prepare_chips(bd.cuda().reshape(3, 1, 1, 20, 24)).reshape(3, 20, 24)
    names = ("fliplr", "gaussian", "cropresize")
    out = DeviceAugmenter(augment_prob=0.0, augmentations=names).apply(Data(x=x.cuda(), y=y.to(torch.int16).cuda(), bdist=bd.cuda()), mean, std)
    assert torch.equal(out.x, px) and torch.equal(out.bdist, pb) and torch.equal(out.y.cpu(), y)
    out = DeviceAugmenter(augment_prob=1.0, augmentations=names).apply(Data(x=x.cuda(), bdist=bd.cuda()), mean, std)
    assert out.y is None and torch.equal(out.x, px) and torch.equal(out.bdist, pb)


def test_plans_that_do_not_fit_are_refused_before_any_launch():
    from cultionet_amd import _lib
    from cultionet_amd.augment import AugmentPlan, DeviceAugmenter
    from cultionet_amd.data import Data

    x, bd, y = _raw(2, 1, 2, 20, 20, torch.int16, 9)
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    th, ph = _angles(3, 1)
    bad = [_plan([{"op": "none"}, {"op": "cropresize", "div": 4, "top": 16, "left": 0}]),   # 5-pixel crop at row 16 of 20
           _plan([{"op": "cropresize", "div": 0, "top": 0, "left": 0}, {"op": "none"}]),
           _plan([{"op": "none"}, {"op": "perlin", "r": 3, "theta": th, "phi": ph}]),      # 3 does not divide 20
           _plan([{"op": "gaussian", "sigma": 0.0}, {"op": "none"}])]
    unknown = AugmentPlan(2)
    unknown.table[1, 0] = 10
    bad.append(unknown)
    n0 = _launches()
    for plan in bad:
        with pytest.raises(_lib.HipKernelError, match="CN_ERR_ARG"):
            DeviceAugmenter().apply(batch, plan=plan)
    assert _launches() == n0
    with pytest.raises(ValueError):
        DeviceAugmenter().apply(batch, plan=AugmentPlan(3))


def test_feeder_augments_on_the_copy_stream():
    """DeviceFeeder(augmenter=...) over three pinned batches yields what apply() gives for the same seeded plans."""
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.feeder import DeviceFeeder, pin_batch

    mean, std = torch.tensor(MEAN[2]), torch.tensor(STD[2])
    hosts = []
    for k in range(3):
        x, bd, y = _raw(4, 2, 3, 20, 20, torch.int16, 20 + k)
        hosts.append(pin_batch(Data(x=x, y=y, bdist=bd)))
    feeder = DeviceFeeder("cuda:0", mean=mean, std=std, augmenter=DeviceAugmenter(augment_prob=0.8, seed=5))
    twin = DeviceAugmenter(augment_prob=0.8, seed=5)
    got = [(b.x.clone(), b.bdist.clone(), b.y.clone()) for b in feeder.iterate(hosts)]
    assert len(got) == 3
    augmented = 0
    for h, (gx, gb, gy) in zip(hosts, got):
        plan = twin.draw(4, 3, 20, 20)
        augmented += int((plan.table[:, 0] != 0).sum())
        want = twin.apply(h.to("cuda:0"), mean, std, plan=plan)
        assert torch.equal(gx, want.x) and torch.equal(gb, want.bdist) and torch.equal(gy, want.y)
    assert augmented >= 6
    plain = list(DeviceFeeder("cuda:0", mean=mean, std=std).iterate(hosts[:1]))[0]  # no augmenter: unchanged behaviour
    assert torch.equal(plain.y.cpu(), hosts[0].y) and not torch.equal(plain.x, got[0][0])


def test_lightning_hook_augments_only_in_training_mode():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import prepare_chips
    from cultionet_amd.lightning import CultionetLitModel

    x, bd, y = _raw(4, 3, 12, 20, 20, torch.int16, 30)
    mean, std = torch.tensor(MEAN[3]), torch.tensor(STD[3])
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0).to("cuda:0")
    lit.set_norm_values(mean, std)
    plain = prepare_chips(x.cuda(), mean, std)

    def batch():
        return Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())

    assert torch.equal(lit.train().on_after_batch_transfer(batch()).x, plain)  # no augmenter: as before
    lit.set_augmenter(DeviceAugmenter(augment_prob=1.0, augmentations=("fliplr",)))
    out = lit.train().on_after_batch_transfer(batch())
    assert torch.equal(out.x, torch.flip(plain, (-1,))) and torch.equal(out.y.cpu(), torch.flip(y, (-1,)))
    out = lit.eval().on_after_batch_transfer(batch())
    assert torch.equal(out.x, plain) and torch.equal(out.y.cpu(), y)
    lit.set_augmenter(None)
    assert torch.equal(lit.train().on_after_batch_transfer(batch()).x, plain)


def test_training_step_on_an_augmented_batch():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    x, bd, y = _raw(2, 3, 12, 20, 20, torch.int16, 40)
    y = y.clamp(max=2)  # background 0, crop 1, edge 2 (the model's default edge class), -1 unlabelled
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0).to("cuda:0").train()
    aug = DeviceAugmenter(augment_prob=1.0, seed=3)
    batch = aug.apply(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda()), torch.tensor(MEAN[3]), torch.tensor(STD[3]))
    loss = HipTrainer(lit).training_step(batch)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.item()))
