"""CPU tests of tests/parcel_ref.py, the numpy restatement the GPU tests of the parcel labelling and of the `roll` op are
held to (tests/test_parcel_augment_gpu.py), and of the host side of `roll` in cultionet_amd.augment:

* label4 equals scipy.ndimage.label (labels and count) on every plane the GPU test uses;
* roll_parcels reproduces, exactly, what the reference's own roll_time made of the two samples recorded in
  tests/golden/augment_roll.npz (tools/make_parcel_golden.py), from the shifts it drew -- the uint8 wrap included;
* DeviceAugmenter.draw: the shifts' value set, the pinned entry 0, reproducibility, an untouched draw stream when no parcel
  augmenter is enabled, and the frequency of `roll` among the candidates;
* the constructor refuses what it does not cover."""
import os

import numpy as np
import pytest

import parcel_ref as P


def test_label4_equals_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    planes = dict(P.fields())
    planes["classes_crop1"] = P.classes_field(20, 20, 7)
    for name, y in planes.items():
        want, n = nd.label(y == 1)
        got, m = P.label4(y)
        assert m == n and got.dtype == np.int32 and np.array_equal(got, want), name
    y = planes["classes_crop1"]
    want, n = nd.label(y == 2)
    got, m = P.label4(y, 2)
    assert m == n and np.array_equal(got, want) and n > 1
    stack = np.stack([planes[f"random_64_0.59_{k}"] for k in (1, 2, 3)])
    labels, counts = P.label4(stack)
    assert labels.shape == stack.shape and [int(c) for c in counts] == [nd.label(p == 1)[1] for p in stack]
    # the planes are what their names say
    assert P.label4(planes["checkerboard_13"])[1] == 85 and P.label4(planes["lattice_34"])[1] == 289
    assert P.label4(planes["comb_20"])[1] == 1 and P.label4(planes["spiral_21"])[1] == 1
    assert planes["spiral_21"].sum() == 241


@pytest.mark.parametrize("case,parcels", [("small", 5), ("lattice", 289)])
def test_roll_parcels_equals_the_reference(golden_dir, case, parcels):
    g = np.load(os.path.join(golden_dir, "augment_roll.npz"))
    x, y, want = g[f"{case}_x"][0], g[f"{case}_y"], g[f"{case}_out"][0]
    labels, n = P.label4(y)
    assert n == parcels and np.array_equal(labels, g[f"{case}_labels"])
    assert np.array_equal(np.uint8(labels), g[f"{case}_segments"])
    shifts = P.shifts_of_props(g[f"{case}_prop_labels"], g[f"{case}_prop_shifts"])
    assert len(g[f"{case}_prop_labels"]) == min(parcels, 255) and np.abs(shifts).max() == 3
    got = np.clip(P.roll_parcels(x, labels, shifts), np.float32(1e-9), np.float32(1.0))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert not np.array_equal(want, x)
    if case == "lattice":  # parcel 256 is background to the reference; 257 is one prop with parcel 1
        assert shifts[1] != 0
        (h, w), (h1, w1) = np.argwhere(labels == 256)[0], np.argwhere(labels == 257)[0]
        assert np.array_equal(want[:, :, h, w], x[:, :, h, w])
        assert np.array_equal(want[:, :, h1, w1], np.roll(x[:, :, h1, w1], shifts[1], axis=1))
    else:  # the L's bbox covers the block: the block still moves by its own shift only
        assert np.array_equal(want[:, :, 2, 3], np.roll(x[:, :, 2, 3], shifts[labels[2, 3]], axis=1))
        assert shifts[labels[2, 3]] != shifts[labels[1, 1]]


def test_roll_parcels_is_a_true_modulus():
    x = np.arange(5, dtype=np.float64).reshape(1, 5, 1, 1) * np.ones((1, 5, 1, 3))
    labels = np.array([[1, 2, 0]])
    shifts = np.zeros(256, dtype=np.int32)
    shifts[1], shifts[2] = -3, 4
    got = P.roll_parcels(x, labels, shifts)
    assert got[0, :, 0, 0].tolist() == [3, 4, 0, 1, 2]   # torch.roll(x, -3): out[t] = x[(t + 3) mod 5]
    assert got[0, :, 0, 1].tolist() == [1, 2, 3, 4, 0]   # torch.roll(x, 4):  out[t] = x[(t - 4) mod 5]
    assert got[0, :, 0, 2].tolist() == [0, 1, 2, 3, 4]


# ---- host side of cultionet_amd.augment ----------------------------------------------------------------------------

def test_plan_rows_of_roll():
    from cultionet_amd.augment import OP_CODES, OPS, PARCEL_AUGMENTATIONS, PARCEL_OP_CODES, AugmentPlan

    assert PARCEL_AUGMENTATIONS == ("roll",) and PARCEL_OP_CODES == {"roll": len(OPS)} and "roll" not in OP_CODES
    plan = AugmentPlan(3)
    assert plan.parcel.shape == (3, 256) and plan.parcel.dtype == np.int32 and not plan.has_parcel
    shifts = np.zeros(256, dtype=np.int64)
    shifts[1:4] = (-3, 3, 1)
    plan.set(1, "roll", shifts=shifts)
    assert plan.has_parcel and [plan.op(b) for b in range(3)] == ["none", "roll", "none"]
    assert list(P.roll_entries(plan)) == [1] and np.array_equal(P.roll_entries(plan)[1], shifts)
    assert int(plan.table[1, 0]) == P.ROLL
    plan.set(1, "fliplr")
    assert not plan.has_parcel and not plan.parcel.any()
    for bad in (None, np.zeros(255, dtype=np.int32), np.zeros(256, dtype=np.float32)):
        with pytest.raises(ValueError):
            plan.set(0, "roll", shifts=bad)
    assert not plan.has_parcel


def test_draw_of_roll_shifts():
    from cultionet_amd.augment import DeviceAugmenter

    def make(seed=3):
        return DeviceAugmenter(augment_prob=1.0, augmentations=(), parcel_augmentations=("roll",), seed=seed)

    plan = make().draw(80, 12, 20, 20)  # 80 * 255 = 20 400 draws
    assert plan.has_parcel and all(plan.op(b) == "roll" for b in range(80))
    assert (plan.parcel[:, 0] == 0).all()
    drawn = plan.parcel[:, 1:]
    assert drawn.size >= 20_000 and drawn.min() == -3 and drawn.max() == 3 and set(np.unique(drawn)) == set(range(-3, 4))
    assert not make().draw(16, 3, 20, 20).parcel.any()  # int(3 * 0.25) = 0
    assert np.abs(make().draw(16, 5, 20, 20).parcel).max() == 1
    a, b = make(7), make(7)
    for _ in range(3):
        pa, pb = a.draw(16, 12, 20, 20), b.draw(16, 12, 20, 20)
        assert np.array_equal(pa.table, pb.table) and np.array_equal(pa.parcel, pb.parcel)
    assert not np.array_equal(pa.parcel, make(8).draw(16, 12, 20, 20).parcel)


def test_draw_without_parcel_augmenters_is_unchanged():
    from cultionet_amd.augment import DeviceAugmenter

    a, b = DeviceAugmenter(seed=11), DeviceAugmenter(seed=11, parcel_augmentations=())
    for _ in range(3):
        pa, pb = a.draw(64, 12, 20, 20), b.draw(64, 12, 20, 20)
        assert np.array_equal(pa.table, pb.table) and np.array_equal(pa.perlin, pb.perlin)
        assert not pb.has_parcel and not pb.parcel.any()
        assert "roll" not in {pb.op(k) for k in range(64)}


def test_roll_is_one_candidate_among_the_others():
    from cultionet_amd.augment import DeviceAugmenter

    others = ("fliplr", "flipud", "rot180")
    N = 20_000
    plan = DeviceAugmenter(augment_prob=1.0, augmentations=others, parcel_augmentations=("roll",), seed=5).draw(N, 12, 10, 28)
    ops = [plan.op(b) for b in range(N)]
    assert set(ops) == set(others) | {"roll"}
    p = 1.0 / (len(others) + 1)
    frac = ops.count("roll") / N
    assert abs(frac - p) <= 4 * np.sqrt(p * (1 - p) / N), frac  # 4 standard errors = 0.0122
    rolled = np.array([o == "roll" for o in ops])
    assert not plan.parcel[~rolled].any() and plan.parcel[rolled].any(axis=1).all()


def test_constructor_errors():
    from cultionet_amd.augment import PARCEL_AUGMENTATIONS, DeviceAugmenter

    for name in ("tswarp", "tsnoise", "tsdrift", "tspeaks"):
        with pytest.raises(NotImplementedError, match="tsaug"):
            DeviceAugmenter(parcel_augmentations=(name,))
    for name in ("shear", "fliplr", "none"):
        with pytest.raises(KeyError):
            DeviceAugmenter(parcel_augmentations=(name,))
    with pytest.raises(NotImplementedError, match="host"):
        DeviceAugmenter(augmentations=("fliplr", "roll"))  # `augmentations=` keeps its meaning
    aug = DeviceAugmenter(parcel_augmentations=PARCEL_AUGMENTATIONS)
    assert aug.parcel_augmentations == ("roll",)
