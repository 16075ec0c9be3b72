"""CPU tests of tests/ts_ref.py, the float64 restatement the GPU test of the series ops is held to
(tests/test_series_augment_gpu.py), and of the host side of tswarp / tsnoise / tsdrift / tspeaks in cultionet_amd.augment:

* halves equals F.interpolate(mode="linear") on float64 tensors within 1e-12;
* apply_series reproduces what the reference's own augment_time made of the two samples recorded in
  tests/golden/augment_series.npz (tools/make_series_golden.py) within 6e-8, one fp32 rounding of the recorded float32
  output -- the uint8 wrap and the parcel inside another parcel's box included;
* the drawn tables have the properties tsaug's TimeWarp / Drift / AddNoise give them, slot 0 is the identity, and every
  value of the two integer parameters is reached;
* the draw is reproducible, leaves the stream of an augmenter without series ops untouched, gives every series op its
  share of the candidates, and drops them when T does not fit the device op;
* the constructor and AugmentPlan.set refuse what they do not cover."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ts_ref as R


@pytest.mark.parametrize("T", [2, 3, 5, 12, 13, 25])
def test_halves_equal_interpolate(T):
    v = torch.from_numpy(np.random.default_rng(T).random((7, 3, T)))
    want = torch.cat((F.interpolate(v, size=T // 2, mode="linear"), F.interpolate(v, size=T - T // 2, mode="linear")), dim=-1)
    got = R.halves(v.numpy())
    assert got.shape == (7, 3, T) and np.abs(got - want.numpy()).max() <= 1e-12


@pytest.mark.parametrize("case,parcels", [("small", 5), ("lattice", 289)])
@pytest.mark.parametrize("op", R.SERIES)
def test_apply_series_equals_the_reference(golden_dir, case, parcels, op):
    import parcel_ref as P

    g = np.load(os.path.join(golden_dir, "augment_series.npz"))
    x, y, want = g[f"{case}_x"][0], g[f"{case}_y"], g[f"{case}_{op}_out"][0]
    labels, n = P.label4(y)
    assert n == parcels and np.array_equal(labels, g[f"{case}_labels"])
    pos, drift, nscale = g[f"{case}_pos"], g[f"{case}_drift"], g[f"{case}_{op}_nscale"]
    assert pos.dtype == drift.dtype == nscale.dtype == np.float32 and want.dtype == np.float32
    used = np.unique(labels & 255)
    assert (nscale[used[used != 0]] > 0).all() and nscale[0] == 0 and np.array_equal(pos[0], np.arange(x.shape[1]))
    got = np.clip(R.apply_series(x, labels, op, pos, drift, nscale, int(g[f"{case}_{op}_seed"])), 1e-9, 1.0)
    err = np.abs(got - want.astype(np.float64)).max()
    print(f"{case} {op}: max |restatement - reference| = {err:.3e}")
    assert err <= 6e-8
    background = (labels & 255) == 0
    assert np.array_equal(want[:, :, background], x[:, :, background])       # slot 0 and parcel 256: untouched
    assert (want[:, :, ~background] != x[:, :, ~background]).mean() > 0.9
    if case == "lattice":  # parcel 257 is one prop with parcel 1: it takes slot 1's tables, which the match above covers
        (h, w), (h1, w1) = np.argwhere(labels == 256)[0], np.argwhere(labels == 257)[0]
        assert np.array_equal(want[:, :, h, w], x[:, :, h, w]) and not np.array_equal(want[:, :, h1, w1], x[:, :, h1, w1])


def test_identity_tables_change_nothing():
    import parcel_ref as P

    g = np.random.default_rng(0)
    x = g.random((2, 12, 10, 28))
    labels, _ = P.label4(P.random_field(10, 28, 0.55, 28))
    for op in ("tswarp", "tsnoise", "tsdrift"):
        assert np.array_equal(R.apply_series(x, labels, op, *R.identity_tables(2, 12), seed=5), x)
    peaks = R.apply_series(x, labels, "tspeaks", *R.identity_tables(2, 12), seed=5)
    assert np.array_equal(peaks[:, :, labels == 0], x[:, :, labels == 0]) and not np.array_equal(peaks, x)


# ---- host side of cultionet_amd.augment ----------------------------------------------------------------------------

def _augmenter(names=None, seed=3, **kw):
    from cultionet_amd.augment import SERIES_AUGMENTATIONS, DeviceAugmenter

    return DeviceAugmenter(augment_prob=1.0, augmentations=(), seed=seed,
                           series_augmentations=SERIES_AUGMENTATIONS if names is None else names, **kw)


def test_constants():
    from cultionet_amd import augment as A

    assert A.SERIES_AUGMENTATIONS == R.SERIES and A.SERIES_OP_CODES == R.CODES
    assert A.SERIES_SLOTS == 256 and A.SERIES_TMAX == 64
    assert A.PARCEL_AUGMENTATIONS == ("roll",) and set(A.HOST_AUGMENTATIONS) == set(R.SERIES) | {"roll"}


@pytest.mark.parametrize("C,T", [(3, 12), (1, 2), (2, 25), (1, 64)])
def test_drawn_tables(C, T):
    plan = _augmenter().draw(200, T, 20, 20, C)
    assert plan.has_series and not plan.has_parcel and plan.series_rows() == list(range(200))
    seeds = set()
    for b in range(200):
        op = plan.op(b)
        pos, drift, nscale = plan.series[b]
        seeds.add(plan.seed(b))
        assert op in R.SERIES and 0 <= plan.seed(b) < 2 ** 63 and not plan.table[b, 1:6].any()
        assert nscale.dtype == np.float32 and nscale.shape == (256,) and nscale[0] == 0
        assert nscale[1:].min() >= np.float32(0.01) and nscale[1:].max() <= np.float32(0.05)
        assert (np.unique(nscale[1:]).size == 1) == (op == "tsnoise")
        assert (pos is not None) == (op in ("tswarp", "tspeaks")) and (drift is not None) == (op == "tsdrift")
        if pos is not None:
            assert pos.dtype == np.float32 and pos.shape == (256, T) and np.array_equal(pos[0], np.arange(T))
            assert (pos[:, 0] == 0).all() and (pos[:, T - 1] == T - 1).all()
            assert (np.diff(pos, axis=1) >= 0).all() and pos.min() >= 0 and pos.max() <= T - 1
            # one curve per slot (with one speed change there are two: the fast half first or last, their ratio is fixed)
            assert T == 2 or len({c.tobytes() for c in pos[1:]}) >= 2
        if drift is not None:
            assert drift.dtype == np.float32 and drift.shape == (256, C, T) and not drift[0].any()
            assert (drift[..., 0] == 0).all()
            top = np.abs(drift[1:]).max(axis=-1)                    # one max_drift per sample, met by every curve
            assert 0.05 <= top.min() and top.max() <= np.float32(0.1) and top.max() - top.min() <= 2 * np.finfo(np.float32).eps * 0.1
    assert len(seeds) == 200
    packed = plan.pack_series(C, T)
    assert packed.shape == (200, 256 * (T + C * T + 1)) and packed.dtype == np.float32
    assert np.array_equal(packed[:, :T], np.tile(np.arange(T, dtype=np.float32), (200, 1)))   # slot 0 of every row


class _Spy:
    """A generator that records the scalar integers(low, high) draws it passes on."""

    def __init__(self, rng):
        self.rng, self.drawn = rng, []

    def integers(self, low, high=None, size=None):
        v = self.rng.integers(low, high, size)
        if size is None and high is not None:
            self.drawn.append(((low, high), int(v)))
        return v

    def __getattr__(self, name):
        return getattr(self.rng, name)


def test_every_n_and_m_is_reached():
    """n speed changes in {1, 2} (integers(1, 3)) and m drift points in 1..5 (integers(1, 6)), one draw per sample, all
    values reached over 2 000 samples; the spied draw is the draw: its plan equals that of an untouched twin."""
    aug, twin = _augmenter(("tswarp", "tsdrift", "tspeaks"), seed=9), _augmenter(("tswarp", "tsdrift", "tspeaks"), seed=9)
    aug.rng = _Spy(aug.rng)
    plan = aug.draw(2000, 12, 20, 20, 2)
    assert np.array_equal(plan.table, twin.draw(2000, 12, 20, 20, 2).table)
    n = [v for key, v in aug.rng.drawn if key == (1, 3)]
    m = [v for key, v in aug.rng.drawn if key == (1, 6)]
    ops = [plan.op(b) for b in range(2000)]
    assert set(n) == {1, 2} and set(m) == {1, 2, 3, 4, 5}
    assert len(n) == ops.count("tswarp") + ops.count("tspeaks") and len(m) == ops.count("tsdrift")


def test_draw_is_reproducible_and_leaves_other_augmenters_alone():
    from cultionet_amd.augment import DeviceAugmenter

    a, b = _augmenter(seed=7), _augmenter(seed=7)
    for _ in range(3):
        pa, pb = a.draw(16, 12, 20, 20, 3), b.draw(16, 12, 20, 20, 3)
        assert np.array_equal(pa.table, pb.table) and np.array_equal(pa.pack_series(3, 12), pb.pack_series(3, 12))
    assert not np.array_equal(pa.pack_series(3, 12), _augmenter(seed=8).draw(16, 12, 20, 20, 3).pack_series(3, 12))
    for kw in ({}, {"parcel_augmentations": ("roll",)}):
        a, b = DeviceAugmenter(seed=11, **kw), DeviceAugmenter(seed=11, series_augmentations=(), **kw)
        for _ in range(3):
            pa, pb = a.draw(64, 12, 20, 20), b.draw(64, 12, 20, 20, 3)
            assert np.array_equal(pa.table, pb.table) and np.array_equal(pa.perlin, pb.perlin)
            assert np.array_equal(pa.parcel, pb.parcel) and not pb.has_series and not pb.series
            assert not set(R.SERIES) & {pb.op(k) for k in range(64)}


def test_series_ops_are_candidates_among_the_others():
    from cultionet_amd.augment import SERIES_AUGMENTATIONS, DeviceAugmenter

    others = ("fliplr", "flipud")
    N = 20_000
    aug = DeviceAugmenter(augment_prob=1.0, augmentations=others, parcel_augmentations=("roll",),
                          series_augmentations=SERIES_AUGMENTATIONS, seed=5)
    assert aug._candidates(10, 28, 5)[0] == list(others) + ["roll"] + list(SERIES_AUGMENTATIONS)
    plan = aug.draw(N, 5, 10, 28, 1)
    ops = [plan.op(b) for b in range(N)]
    p = 1.0 / 7
    for name in SERIES_AUGMENTATIONS + others + ("roll",):
        frac = ops.count(name) / N
        assert abs(frac - p) <= 4 * np.sqrt(p * (1 - p) / N), (name, frac)  # 4 standard errors = 0.0099
    assert plan.series_rows() == [b for b, o in enumerate(ops) if o in SERIES_AUGMENTATIONS]


@pytest.mark.parametrize("T", [1, 65])
def test_a_series_the_device_cannot_hold_drops_the_ops(T):
    from cultionet_amd.augment import SERIES_AUGMENTATIONS, DeviceAugmenter

    plan = _augmenter().draw(64, T, 20, 20, 1)
    assert not plan.has_series and not plan.table.any()                     # no candidate left: nothing is drawn
    aug = DeviceAugmenter(augment_prob=1.0, augmentations=("fliplr",), series_augmentations=SERIES_AUGMENTATIONS, seed=2)
    plan = aug.draw(64, T, 20, 20, 1)
    assert {plan.op(b) for b in range(64)} == {"fliplr"}
    for T_ok in (2, 64):
        assert _augmenter().draw(8, T_ok, 20, 20, 1).has_series


def test_constructor_errors():
    from cultionet_amd.augment import SERIES_AUGMENTATIONS, DeviceAugmenter

    for name in ("roll", "fliplr", "none", "shear"):
        with pytest.raises(KeyError):
            DeviceAugmenter(series_augmentations=(name,))
    for name in SERIES_AUGMENTATIONS:  # the two older keywords keep refusing the names
        with pytest.raises(NotImplementedError, match="tsaug"):
            DeviceAugmenter(parcel_augmentations=(name,))
        with pytest.raises(NotImplementedError, match="series_augmentations"):
            DeviceAugmenter(parcel_augmentations=(name,))
        with pytest.raises(NotImplementedError, match="host"):
            DeviceAugmenter(augmentations=(name,))
    aug = DeviceAugmenter(series_augmentations=SERIES_AUGMENTATIONS)
    assert aug.series_augmentations == SERIES_AUGMENTATIONS and aug.parcel_augmentations == ()
    with pytest.raises(ValueError, match="channels"):   # tsdrift draws one curve per channel: draw() must be told C
        aug.draw(4, 12, 20, 20)
    assert len(aug.draw(4, 12, 20, 20, 3)) == 4
    assert len(DeviceAugmenter(series_augmentations=("tswarp", "tsnoise", "tspeaks")).draw(4, 12, 20, 20)) == 4
    assert len(aug.draw(4, 1, 20, 20)) == 4             # no series candidate at T = 1: nothing to ask for


def test_plan_rows_of_the_series_ops():
    from cultionet_amd.augment import AugmentPlan

    C, T = 2, 5
    pos, drift, nscale = R.hand_tables(C, T, 1)
    plan = AugmentPlan(4)
    assert not plan.has_series and plan.series_rows() == []
    plan.set(1, "tswarp", pos=pos, nscale=nscale, seed=(1 << 62) + 5)
    plan.set(3, "tsdrift", drift=drift)
    plan.set(2, "tsnoise")
    assert plan.has_series and not plan.has_parcel and plan.series_rows() == [1, 2, 3]
    assert [plan.op(b) for b in range(4)] == ["none", "tswarp", "tsnoise", "tsdrift"]
    assert [int(plan.table[b, 0]) for b in (1, 2, 3)] == [11, 12, 13] and plan.seed(1) == (1 << 62) + 5
    ident = R.identity_tables(C, T)
    packed = plan.pack_series(C, T).reshape(3, -1)
    for row, want in zip(packed, ((pos, ident[1], nscale), ident, (ident[0], drift, ident[2]))):
        assert np.array_equal(row, np.concatenate([a.reshape(-1) for a in want]))   # what is left out is the identity
    saved = pos.copy()   # the plan keeps copies: changing the caller's array afterwards changes nothing
    pos[1:, 1:] += np.float32(0.125)
    assert not np.array_equal(pos, saved) and np.array_equal(plan.series[1][0], saved)
    assert np.array_equal(plan.pack_series(C, T)[0, :256 * T].reshape(256, T), saved)
    pos[:] = saved
    # setting a row again leaves nothing stale
    plan.set(1, "fliplr")
    assert plan.series_rows() == [2, 3] and 1 not in plan.series and not plan.table[1, 1:].any()
    plan.set(3, "tspeaks", pos=R.hand_tables(C, T, 2)[0])
    assert plan.series[3][1] is None and plan.op(3) == "tspeaks" and int(plan.table[3, 0]) == 14
    plan.set(2, "roll", shifts=np.zeros(256, dtype=np.int32))
    assert plan.series_rows() == [3] and plan.has_parcel
    plan.set(2, "tsnoise", nscale=nscale)
    assert not plan.has_parcel and not plan.parcel.any()
    by_hand = AugmentPlan(2)   # the op code alone, no tables: not a series plan
    by_hand.table[1, 0] = 11
    assert not by_hand.has_series and by_hand.op(1) == "tswarp"
    # shapes and dtypes
    before = plan.table.copy()
    for kw in (dict(pos=pos.astype(np.float64)), dict(pos=pos[:255]), dict(pos=pos[0]), dict(drift=drift[:, 0]),
               dict(drift=drift.astype(np.float64)), dict(nscale=nscale[:, None]), dict(nscale=nscale.astype(np.float64)),
               dict(nscale=np.zeros(255, dtype=np.float32)), dict(pos=pos, drift=np.zeros((256, C, T + 1), dtype=np.float32))):
        with pytest.raises(ValueError):
            plan.set(0, "tswarp", **kw)
    with pytest.raises(ValueError):
        plan.set(0, "fliplr", pos=pos)
    assert np.array_equal(plan.table, before) and 0 not in plan.series
    for C_, T_ in ((C, T + 1), (C + 1, T)):   # tables that do not fit the batch
        wrong = AugmentPlan(1).set(0, "tsdrift", pos=pos, drift=drift)
        with pytest.raises(ValueError):
            wrong.pack_series(C_, T_)
