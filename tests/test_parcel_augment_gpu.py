"""Parcel labelling (cn_label_parcels_i32, cultionet_amd.augment.label_parcels) and the `roll` op of the augmentation
prologue (cn_augment_parcels_f32) against tests/parcel_ref.py, itself pinned to scipy.ndimage.label and to the
reference's own roll_time by tests/test_parcel_ref.py.

Conditions -- all exact, nothing here is arithmetic beyond the prologue's own:
* labels and counts are torch.equal to label4, and to themselves on a second run;
* x of a `roll` sample is torch.equal to roll_parcels of what cn_prepare_chips_f32 gives (roll is a gather along T);
  its y and bdist, and every sample that is not `roll`, equal what apply() gives without `roll`;
* the recorded outputs of the reference (tests/golden/augment_roll.npz) are met within 6e-8, one fp32 rounding of a value
  in [0, 1]: the device forms raw * 1e-4f where the reference divides by 10000;
* at most three launches with a `roll` row, at most two without."""
import os

import numpy as np
import pytest
import torch

import parcel_ref as P

pytestmark = pytest.mark.gpu

MEAN = {1: [0.27], 2: [0.31, 0.22], 3: [0.3, 0.25, 0.4]}
STD = {1: [0.21], 2: [0.17, 0.09], 3: [0.2, 0.15, 0.3]}
FIELDS = P.fields()


def _launches():
    from cultionet_amd import _lib

    return _lib.query("cn_launch_count", 0)


def _label_twice(y, crop_value=1):
    """y: host tensor [B, H, W]. Labels it twice on the device, checks both runs against label4, returns the labels."""
    from cultionet_amd.augment import label_parcels

    yd = y.cuda()
    torch.cuda.synchronize()
    n0 = _launches()
    labels, counts = label_parcels(yd, crop_value)
    assert _launches() - n0 == 1
    again, counts_again = label_parcels(yd, crop_value)
    want, n = P.label4(y.numpy().astype(np.int64), crop_value)
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32
    assert labels.shape == y.shape and counts.shape == (y.shape[0],)
    assert torch.equal(counts.cpu(), torch.from_numpy(n))
    assert torch.equal(labels.cpu(), torch.from_numpy(want))
    assert torch.equal(again, labels) and torch.equal(counts_again, counts)
    return labels


@pytest.mark.parametrize("name", list(FIELDS))
def test_labels_equal_label4(name):
    _label_twice(torch.from_numpy(FIELDS[name])[None])


def test_batch_of_different_fields():
    names = [f"random_64_{d}_{s}" for d, s in ((0.45, 1), (0.59, 2), (0.75, 3), (0.59, 1), (0.45, 3))]
    _label_twice(torch.from_numpy(np.stack([FIELDS[n] for n in names])))
    large = np.stack([FIELDS[f"random_128_{d}"] for d in (0.45, 0.59, 0.75)] + [FIELDS["all_fg_128"]])
    _label_twice(torch.from_numpy(large))
    small = np.stack([FIELDS["all_fg_13"], FIELDS["checkerboard_13"], FIELDS["all_bg_13"]])
    _label_twice(torch.from_numpy(small))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int16, torch.uint16, torch.int64], ids=["i32", "i16", "u16", "i64"])
def test_label_dtypes(dtype):
    y = torch.from_numpy(FIELDS["random_40"])[None].to(dtype)
    want = _label_twice(torch.from_numpy(FIELDS["random_40"])[None])
    assert torch.equal(_label_twice(y), want)


@pytest.mark.parametrize("crop_value", [1, 2])
def test_only_the_crop_class_is_foreground(crop_value):
    y = torch.from_numpy(np.stack([P.classes_field(20, 20, 7), P.classes_field(20, 20, 8)]))
    assert set(y.unique().tolist()) == {-1, 0, 1, 2, 3}
    labels = _label_twice(y, crop_value)
    assert torch.equal(labels.cpu() > 0, y == crop_value)


def test_label_arguments():
    from cultionet_amd import _lib
    from cultionet_amd.augment import label_parcels

    with pytest.raises(RuntimeError):
        label_parcels(torch.zeros(1, 4, 4, dtype=torch.int64))
    with pytest.raises(TypeError):
        label_parcels(torch.zeros(1, 4, 4).cuda())
    y = torch.ones(1, 4, 4, dtype=torch.int32).cuda()
    out = torch.empty(16, dtype=torch.int32).cuda()
    n0 = _launches()
    for args in ((None, 1, 1, out.data_ptr(), out.data_ptr(), 1, 4, 4), (y.data_ptr(), 0, 1, out.data_ptr(), out.data_ptr(), 1, 4, 4),
                 (y.data_ptr(), 5, 1, out.data_ptr(), out.data_ptr(), 1, 4, 4), (y.data_ptr(), 1, 1, None, out.data_ptr(), 1, 4, 4),
                 (y.data_ptr(), 1, 1, out.data_ptr(), None, 1, 4, 4), (y.data_ptr(), 1, 1, out.data_ptr(), out.data_ptr(), 0, 4, 4),
                 (y.data_ptr(), 1, 1, out.data_ptr(), out.data_ptr(), 1, 4, -1),
                 (y.data_ptr(), 1, 1, out.data_ptr(), out.data_ptr(), 1, 1 << 16, 1 << 15)):
        with pytest.raises(_lib.HipKernelError, match="CN_ERR_ARG"):
            _lib.call("cn_label_parcels_i32", *args, None)
    assert _launches() == n0


# ---- roll -------------------------------------------------------------------------------------------------------------

def _raw(B, C, T, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lo = 0 if dtype == torch.uint16 else -20
    x = torch.randint(lo, 11000, (B, C, T, H, W), generator=g)  # below 0 and above 10000: both clips are exercised
    bd = torch.randint(0, 10001, (B, H, W), generator=g)
    if dtype == torch.float32:
        x = x.float() + torch.rand(x.shape, generator=g)
        bd = bd.float() + torch.rand(bd.shape, generator=g)
    return x.to(dtype), bd.to(dtype)


def _shift_tables(T, seed):
    """Four tables: every parcel by -3, by 3, by 0, and mixed signs over the whole range |s| < T."""
    g = np.random.default_rng(seed)
    out = []
    for fill in (-3, 3, 0, None):
        s = np.zeros(256, dtype=np.int32)
        s[1:] = g.integers(-(T - 1), T, 255) if fill is None else fill
        out.append(s)
    assert out[3].min() < 0 < out[3].max()
    return out


def _plan(entries):
    from cultionet_amd.augment import AugmentPlan

    plan = AugmentPlan(len(entries))
    for b, e in enumerate(entries):
        plan.set(b, e["op"], **{k: v for k, v in e.items() if k != "op"})
    return plan


def _apply_roll(x, bd, y, tables, C):
    """apply() under a plan whose sample b rolls by tables[b]; checks x, y, bdist and the launch count."""
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import prepare_chips

    B, _, T, H, W = x.shape
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])
    plan = _plan([{"op": "roll", "shifts": s} for s in tables])
    assert sorted(P.roll_entries(plan)) == list(range(B))
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    torch.cuda.synchronize()
    n0 = _launches()
    out = DeviceAugmenter().apply(batch, mean, std, plan=plan)
    assert _launches() - n0 <= 3
    plain_x = prepare_chips(batch.x, mean, std).cpu()
    plain_bd = prepare_chips(batch.bdist.reshape(B, 1, 1, H, W)).reshape(B, H, W).cpu()
    labels, _ = P.label4(y.numpy())
    gx = out.x.cpu()
    assert gx.dtype == torch.float32 and out.y.dtype == torch.int64
    for b in range(B):
        want = P.roll_parcels(plain_x[b].numpy(), labels[b], tables[b])
        assert torch.equal(gx[b], torch.from_numpy(want)), b
        if np.any(tables[b][labels[b] & 255]):
            assert not torch.equal(gx[b], plain_x[b]), b
    assert torch.equal(out.y.cpu(), y.long()) and torch.equal(out.bdist.cpu(), plain_bd)
    return gx, plain_x, labels


@pytest.mark.parametrize("C,T,H,W,dtype", [(3, 12, 20, 20, torch.int16), (1, 5, 13, 13, torch.uint16), (2, 12, 10, 28, torch.float32)],
                         ids=["20x20_i16", "13x13_u16", "10x28_f32"])
def test_roll_equals_the_gather(C, T, H, W, dtype):
    tables = _shift_tables(T, seed=H)
    x, bd = _raw(4, C, T, H, W, dtype, seed=W)
    planes = [P.classes_field(H, W, 50 + k) for k in range(3)] + [P.random_field(H, W, 0.55, 60)]
    y = torch.from_numpy(np.stack(planes))
    assert min(P.label4(p)[1] for p in planes) >= 3
    _apply_roll(x, bd, y, tables, C)


def test_roll_wraps_parcels_as_uint8():
    """34 x 34 lattice, 289 parcels: 256 stays put, 257 moves with the shift of parcel 1."""
    tables = _shift_tables(12, seed=34)
    for s in tables:
        s[1] = 2 if s[1] == 0 else s[1]
    x, bd = _raw(4, 1, 12, 34, 34, torch.int16, seed=34)
    y = torch.from_numpy(np.stack([FIELDS["lattice_34"]] * 4))
    gx, plain_x, labels = _apply_roll(x, bd, y, tables, 1)
    (h, w), (h1, w1) = np.argwhere(labels[0] == 256)[0], np.argwhere(labels[0] == 257)[0]
    for b in range(4):
        assert torch.equal(gx[b, :, :, h, w], plain_x[b, :, :, h, w])
        assert torch.equal(gx[b, :, :, h1, w1], torch.roll(plain_x[b, :, :, h1, w1], int(tables[b][1]), dims=1))
        assert not torch.equal(gx[b, :, :, h1, w1], plain_x[b, :, :, h1, w1])


def test_mixed_batch_leaves_the_other_samples_alone():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data

    C, T, H, W = 2, 12, 20, 20
    tables = _shift_tables(T, seed=5)
    x, bd = _raw(5, C, T, H, W, torch.int16, seed=9)
    y = torch.from_numpy(np.stack([P.classes_field(H, W, 70 + k) for k in range(5)]))
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])
    entries = [{"op": "roll", "shifts": tables[3]}, {"op": "none"}, {"op": "fliplr"}, {"op": "gaussian", "sigma": 0.3},
               {"op": "roll", "shifts": tables[0]}]
    without = [e if e["op"] != "roll" else {"op": "none"} for e in entries]
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    aug = DeviceAugmenter()
    torch.cuda.synchronize()
    n0 = _launches()
    want = aug.apply(batch, mean, std, plan=_plan(without))
    n1 = _launches()
    got = aug.apply(batch, mean, std, plan=_plan(entries))
    assert n1 - n0 <= 2 and _launches() - n1 <= 3
    for b in (1, 2, 3):
        assert torch.equal(got.x[b], want.x[b]), b
    assert torch.equal(got.y, want.y) and torch.equal(got.bdist, want.bdist)  # roll leaves the targets as `none` does
    labels, _ = P.label4(y.numpy())
    for b, s in ((0, tables[3]), (4, tables[0])):
        rolled = P.roll_parcels(want.x[b].cpu().numpy(), labels[b], s)
        assert torch.equal(got.x[b].cpu(), torch.from_numpy(rolled)) and not torch.equal(got.x[b], want.x[b]), b


@pytest.mark.parametrize("case", ["small", "lattice"])
def test_roll_equals_the_reference(golden_dir, case):
    from cultionet_amd.augment import DeviceAugmenter, label_parcels
    from cultionet_amd.data import Data

    g = np.load(os.path.join(golden_dir, "augment_roll.npz"))
    x_raw, y = torch.from_numpy(g[f"{case}_x_raw"]), torch.from_numpy(g[f"{case}_y"])[None]
    labels, counts = label_parcels(y.cuda())
    assert torch.equal(labels.cpu()[0], torch.from_numpy(g[f"{case}_labels"]))  # scipy's own numbering, recorded
    assert int(counts[0]) == int(g[f"{case}_labels"].max())
    shifts = P.shifts_of_props(g[f"{case}_prop_labels"], g[f"{case}_prop_shifts"])
    out = DeviceAugmenter().apply(Data(x=x_raw.cuda(), y=y.cuda()), plan=_plan([{"op": "roll", "shifts": shifts}]))
    err = (out.x.cpu().double() - torch.from_numpy(g[f"{case}_out"]).double()).abs().max().item()
    print(f"{case}: max |x - reference| = {err:.3e}")
    assert err <= 6e-8
    assert not torch.equal(out.x.cpu(), torch.from_numpy(g[f"{case}_x"]))


def test_drawn_roll_plans_apply():
    """DeviceAugmenter(parcel_augmentations=("roll",)) end to end: what apply() draws is what it applies."""
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import prepare_chips

    x, bd = _raw(3, 2, 12, 20, 20, torch.int16, seed=11)
    y = torch.from_numpy(np.stack([P.classes_field(20, 20, 90 + k) for k in range(3)]))

    def make():
        return DeviceAugmenter(augment_prob=1.0, augmentations=(), parcel_augmentations=("roll",), seed=4)

    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    out = make().apply(batch)
    plan = make().draw(3, 12, 20, 20)
    plain = prepare_chips(batch.x).cpu()
    labels, _ = P.label4(y.numpy())
    for b, s in P.roll_entries(plan).items():
        assert torch.equal(out.x[b].cpu(), torch.from_numpy(P.roll_parcels(plain[b].numpy(), labels[b], s)))
    assert len(P.roll_entries(plan)) == 3


def test_bad_shift_tables_are_refused():
    from cultionet_amd import _lib
    from cultionet_amd.augment import AugmentPlan, DeviceAugmenter
    from cultionet_amd.data import Data

    x, bd = _raw(2, 1, 12, 20, 20, torch.int16, seed=12)
    y = torch.from_numpy(np.stack([P.classes_field(20, 20, 1), P.classes_field(20, 20, 2)]))
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    good = np.zeros(256, dtype=np.int32)
    good[1:] = 11
    DeviceAugmenter().apply(batch, plan=_plan([{"op": "none"}, {"op": "roll", "shifts": good}]))  # |s| = T - 1 fits
    for k, v in ((200, 12), (7, -12), (0, 1)):
        bad = good.copy()
        bad[k] = v
        with pytest.raises(_lib.HipKernelError, match="CN_ERR_ARG"):
            DeviceAugmenter().apply(batch, plan=_plan([{"op": "none"}, {"op": "roll", "shifts": bad}]))
    by_hand = AugmentPlan(2)  # the op code alone, no shifts: not a parcel plan, and refused before any launch
    by_hand.table[1, 0] = P.ROLL
    n0 = _launches()
    with pytest.raises(_lib.HipKernelError, match="CN_ERR_ARG"):
        DeviceAugmenter().apply(batch, plan=by_hand)
    assert _launches() == n0
