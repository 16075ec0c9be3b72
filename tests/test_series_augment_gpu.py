"""The series ops of the augmentation prologue (tswarp, tsnoise, tsdrift, tspeaks: cn_augment_series_f32,
cultionet_amd.augment) against tests/ts_ref.py, itself pinned to F.interpolate and to the reference's own augment_time by
tests/test_ts_ref.py.

Exact conditions (torch.equal): a tswarp / tsdrift / tsnoise sample with identity tables, and the slot-0 pixels of every
series sample, equal cn_prepare_chips_f32; y and bdist of a series sample equal those of `none`; the other samples of a
mixed batch equal what the batch gives without the series rows; two runs of a plan are equal.

Numerical condition: each op against ts_ref.apply_series, computed in float64 from the float32 values of the prologue and
z-scored, |d| <= 4e-6 / std[c]. The ops are continuous in every input (lerps, max / min, clips), so there is no tie to
exclude; intermediates stay below about 1.4, where one fp32 rounding is 1.2e-7; the longest chain (halves, warp, noise) is
under thirty roundings = 3.6e-6; the noise term is bounded by 0.05 * 5.8 * range through logf / sqrtf / cosf accurate to a
few ulp, as in tests/test_augment_gpu.py. The test prints the observed maximum per op.

Shapes: the smallest at which the kernel can go wrong -- planes of more than one pixel tile that are no multiple of it
(20 x 20, 34 x 34 against 256; 13 x 13 against 128), T on both sides of the switch from 256 to 128 pixels per block
(32, 33), T = 2 and T = 64, one and several channels, every raw dtype."""
import os

import numpy as np
import pytest
import torch

import parcel_ref as P
import ts_ref as R

pytestmark = pytest.mark.gpu

MEAN = {1: [0.27], 2: [0.31, 0.22], 3: [0.3, 0.25, 0.4]}
STD = {1: [0.21], 2: [0.17, 0.09], 3: [0.2, 0.15, 0.3]}
BOUND = 4e-6
FIELDS = P.fields()
SHAPES = [(3, 12, 20, 20, torch.int16), (1, 5, 13, 13, torch.uint16), (2, 25, 10, 28, torch.float32),
          (1, 2, 9, 9, torch.int16), (1, 12, 34, 34, torch.int16), (1, 32, 17, 17, torch.int16),
          (2, 33, 13, 13, torch.int16), (1, 64, 12, 12, torch.uint16)]
IDS = ["20x20_i16", "13x13_u16", "10x28_f32", "T2_9x9", "lattice_34", "T32_17x17", "T33_13x13", "T64_12x12"]


def _launches():
    from cultionet_amd import _lib

    return _lib.query("cn_launch_count", 0)


def _raw(B, C, T, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    lo = 0 if dtype == torch.uint16 else -20
    x = torch.randint(lo, 11000, (B, C, T, H, W), generator=g)  # below 0 and above 10000: both clips are exercised
    bd = torch.randint(0, 10001, (B, H, W), generator=g)
    if dtype == torch.float32:
        x = x.float() + torch.rand(x.shape, generator=g)
        bd = bd.float() + torch.rand(bd.shape, generator=g)
    return x.to(dtype), bd.to(dtype)


def _planes(B, H, W):
    """B label planes [H, W] with several parcels each, background and other classes between them."""
    if (H, W) == (34, 34):
        return np.stack([FIELDS["lattice_34"]] * B)
    out = [P.classes_field(H, W, 50 + k) for k in range(B - 1)] + [P.random_field(H, W, 0.55, 60)]
    assert min(P.label4(p)[1] for p in out) >= 2
    return np.stack(out)


def _plan(entries):
    from cultionet_amd.augment import AugmentPlan

    plan = AugmentPlan(len(entries))
    for b, e in enumerate(entries):
        plan.set(b, e["op"], **{k: v for k, v in e.items() if k != "op"})
    return plan


def _entry(op, tables, seed):
    return {"op": op, "pos": tables[0], "drift": tables[1], "nscale": tables[2], "seed": seed}


def _without_series(entries):
    return [e if e["op"] not in R.SERIES else {"op": "none"} for e in entries]


def _batch(x, bd, y):
    from cultionet_amd.data import Data

    return Data(x=x.cuda(), y=torch.as_tensor(y).cuda(), bdist=bd.cuda())


def _want(plain, labels, e, mean, std, lo=1e-9, hi=1.0):
    """float64 reference of one sample from the float32 prologue values `plain` [C, T, H, W] (not z-scored)."""
    out = R.apply_series(plain.double().numpy(), labels, e["op"], e["pos"], e["drift"], e["nscale"], e["seed"])
    out = np.clip(out, lo, hi)
    C = out.shape[0]
    return (out - np.asarray(mean, dtype=np.float64).reshape(C, 1, 1, 1)) / np.asarray(std, dtype=np.float64).reshape(C, 1, 1, 1)


@pytest.mark.parametrize("C,T,H,W,dtype", SHAPES, ids=IDS)
def test_ops_match_the_restatement(C, T, H, W, dtype):
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.edges import prepare_chips

    B = 5
    x, bd = _raw(B, C, T, H, W, dtype, seed=W + T)
    y = _planes(B, H, W)
    labels, _ = P.label4(y)
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])
    entries = [_entry(op, R.hand_tables(C, T, 10 * T + k), (1 << 40) + 977 * k + T) for k, op in enumerate(R.SERIES)]
    entries.insert(2, {"op": "fliplr"})
    batch = _batch(x, bd, y)
    aug = DeviceAugmenter()
    torch.cuda.synchronize()
    n0 = _launches()
    base = aug.apply(batch, mean, std, plan=_plan(_without_series(entries)))
    n1 = _launches()
    got = aug.apply(batch, mean, std, plan=_plan(entries))
    assert n1 - n0 <= 2 and _launches() - n1 <= 4
    again = aug.apply(batch, mean, std, plan=_plan(entries))
    assert torch.equal(again.x, got.x)
    assert torch.equal(got.y, base.y) and torch.equal(got.bdist, base.bdist) and torch.equal(got.x[2], base.x[2])
    assert got.x.dtype == torch.float32 and got.y.dtype == torch.int64
    plain = prepare_chips(batch.x).cpu()              # the prologue's float32 values, before the z-score
    plain_z = prepare_chips(batch.x, mean, std).cpu()
    gx = got.x.cpu()
    tol = (BOUND / np.asarray(STD[C])).reshape(C, 1, 1, 1)
    for b, e in enumerate(entries):
        if e["op"] not in R.SERIES:
            continue
        slot0 = torch.from_numpy((labels[b] & 255) == 0)
        assert slot0.any() and not slot0.all()
        assert torch.equal(gx[b][:, :, slot0], plain_z[b][:, :, slot0]), (b, e["op"])
        assert not torch.equal(gx[b], plain_z[b]), (b, e["op"])
        d = np.abs(gx[b].double().numpy() - _want(plain[b], labels[b], e, MEAN[C], STD[C]))
        print(f"{e['op']}: max |d| * std = {(d * np.asarray(STD[C]).reshape(C, 1, 1, 1)).max():.3e}")
        assert (d <= tol).all(), (b, e["op"], float((d / tol).max()))


@pytest.mark.parametrize("H,W", [(20, 20), (36, 36)], ids=["20x20", "36x36"])
def test_mixed_batch_leaves_the_other_samples_alone(H, W):
    """`none`, `gaussian`, `roll` and `fliplr` rows beside the four series rows: x of those rows, and y and bdist of the
    whole batch, are torch.equal to the batch applied with `none` in place of the series rows. The roll tables travel
    through cn_augment_series_f32 here; at 36 x 36 the blur's band outgrows the rotation tile, so the LDS of the plane
    launch is sized by the blur inside a series call, and a plane has two bands."""
    from cultionet_amd.augment import DeviceAugmenter

    C, T, B = 2, 12, 8
    x, bd = _raw(B, C, T, H, W, torch.int16, seed=H)
    y = _planes(B, H, W)
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])
    shifts = np.zeros(256, dtype=np.int32)
    shifts[1:] = np.random.default_rng(H).integers(-(T - 1), T, 255)
    series = [_entry(op, R.hand_tables(C, T, 40 + k), 500 + k) for k, op in enumerate(R.SERIES)]
    entries = [series[0], {"op": "none"}, {"op": "gaussian", "sigma": 0.3}, {"op": "roll", "shifts": shifts}, series[1],
               {"op": "fliplr"}, series[2], series[3]]
    batch = _batch(x, bd, y)
    aug = DeviceAugmenter()
    torch.cuda.synchronize()
    n0 = _launches()
    base = aug.apply(batch, mean, std, plan=_plan(_without_series(entries)))
    n1 = _launches()
    got = aug.apply(batch, mean, std, plan=_plan(entries))
    assert n1 - n0 <= 3 and _launches() - n1 <= 4
    assert torch.equal(got.y, base.y) and torch.equal(got.bdist, base.bdist)
    plain = aug.apply(batch, mean, std, plan=_plan([{"op": "none"}] * B))
    for b, e in enumerate(entries):
        if e["op"] in R.SERIES:
            assert not torch.equal(got.x[b], base.x[b]), (b, e["op"])
        else:
            assert torch.equal(got.x[b], base.x[b]), (b, e["op"])
            assert e["op"] == "none" or not torch.equal(got.x[b], plain.x[b]), (b, e["op"])  # the op itself acted
    assert not torch.equal(got.y[5], plain.y[5]) and torch.equal(got.y[3], plain.y[3])      # fliplr turns y, roll does not


@pytest.mark.parametrize("C,T,H,W,dtype", SHAPES, ids=IDS)
def test_identity_tables_are_exact(C, T, H, W, dtype):
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.edges import prepare_chips

    x, bd = _raw(4, C, T, H, W, dtype, seed=H + T)
    y = _planes(4, H, W)
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])
    ident = R.identity_tables(C, T)
    entries = [_entry("tswarp", ident, 3), _entry("tsdrift", ident, 4), {"op": "tsnoise", "seed": 5}, _entry("tspeaks", ident, 6)]
    batch = _batch(x, bd, y)
    got = DeviceAugmenter().apply(batch, mean, std, plan=_plan(entries))
    plain_z = prepare_chips(batch.x, mean, std)
    assert torch.equal(got.x[:3], plain_z[:3])       # every step returns its input bit for bit
    slot0 = torch.from_numpy((P.label4(y)[0][3] & 255) == 0).cuda()
    assert torch.equal(got.x[3][:, :, slot0], plain_z[3][:, :, slot0])
    assert not torch.equal(got.x[3], plain_z[3])     # the halves alone change a parcel
    assert torch.equal(got.y.cpu(), torch.from_numpy(y)) and got.bdist.dtype == torch.float32


def test_wrap_of_the_parcel_slots():
    """34 x 34 lattice, 289 parcels: with tables in slot 1 only, parcels 1 and 257 change and nothing else does; 256 is
    slot 0. (tspeaks halves every parcel but 256 whatever the tables: it is compared with itself under identity tables.)"""
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.edges import prepare_chips

    C, T = 1, 12
    x, bd = _raw(5, C, T, 34, 34, torch.int16, seed=34)
    x[4] = x[3]
    y = _planes(5, 34, 34)
    labels, _ = P.label4(y)
    hand = R.hand_tables(C, T, 7)
    hand[2][1] = 0.05
    tables = R.identity_tables(C, T)
    for a, h in zip(tables, hand):
        a[1] = h[1]
    entries = [_entry(op, tables, 99 + k) for k, op in enumerate(R.SERIES)]
    batch = _batch(x, bd, y)
    gx = DeviceAugmenter().apply(batch, plan=_plan(entries + [_entry("tspeaks", R.identity_tables(C, T), 0)])).x.cpu()
    plain = prepare_chips(batch.x).cpu()
    for b, e in enumerate(entries):
        lab = labels[b]
        (h, w), (h0, w0), (h1, w1) = (np.argwhere(lab == k)[0] for k in (256, 1, 257))
        assert torch.equal(gx[b, :, :, h, w], plain[b, :, :, h, w])
        changed = (gx[b] != (gx[4] if e["op"] == "tspeaks" else plain[b])).any(dim=0).any(dim=0).numpy()
        assert changed[h0, w0] and changed[h1, w1] and not changed[h, w], e["op"]
        assert changed.sum() == 2 and set(lab[changed]) == {1, 257}, e["op"]
        d = np.abs(gx[b].double().numpy() - _want(plain[b], lab, e, [0.0], [1.0]))
        assert d.max() <= BOUND


@pytest.mark.parametrize("case", ["small", "lattice"])
def test_ops_equal_the_reference(golden_dir, case):
    from cultionet_amd.augment import DeviceAugmenter, label_parcels

    g = np.load(os.path.join(golden_dir, "augment_series.npz"))
    x_raw, y = torch.from_numpy(g[f"{case}_x_raw"]), torch.from_numpy(g[f"{case}_y"])[None]
    labels, _ = label_parcels(y.cuda())
    assert torch.equal(labels.cpu()[0], torch.from_numpy(g[f"{case}_labels"]))  # scipy's own numbering, recorded
    entries = [{"op": op, "pos": g[f"{case}_pos"], "drift": g[f"{case}_drift"], "nscale": g[f"{case}_{op}_nscale"],
                "seed": int(g[f"{case}_{op}_seed"])} for op in R.SERIES]
    B = len(entries)
    out = DeviceAugmenter().apply(_batch(x_raw.expand(B, *x_raw.shape[1:]).contiguous(), torch.zeros(B, *y.shape[1:], dtype=torch.int16),
                                         y.expand(B, *y.shape[1:]).contiguous()), plan=_plan(entries))
    for b, op in enumerate(R.SERIES):
        err = (out.x[b].cpu().double() - torch.from_numpy(g[f"{case}_{op}_out"][0]).double()).abs().max().item()
        print(f"{case} {op}: max |x - reference| = {err:.3e}")
        assert err <= 6e-8 + BOUND
        assert not torch.equal(out.x[b].cpu(), torch.from_numpy(g[f"{case}_x"][0]))


def test_noise_statistics():
    """One 64 x 64 all-crop sample under tsnoise, raw values in 3000-7000: the range of a series is at most 0.4, so
    |noise| <= 0.05 * 0.4 * 5.8 = 0.116 < 0.3 and neither clip acts (5.8 bounds a Box-Muller normal from a 24-bit
    uniform: sqrt(2 * 24 * ln 2) = 5.77). (out - in) / (nscale * range) is then the normal field itself."""
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.edges import prepare_chips

    C, T, H, W = 2, 12, 64, 64
    g = torch.Generator().manual_seed(64)
    x = torch.randint(3000, 7001, (1, C, T, H, W), generator=g).to(torch.int16)
    y = torch.ones(1, H, W, dtype=torch.int64)
    nscale = np.zeros(256, dtype=np.float32)
    nscale[1] = 0.05
    batch = _batch(x, torch.zeros(1, H, W, dtype=torch.int16), y)
    plain = prepare_chips(batch.x).cpu().double()
    rng = plain.amax(dim=2, keepdim=True) - plain.amin(dim=2, keepdim=True)
    assert rng.max() <= 0.4 and rng.min() > 0
    fields = []
    for seed in (12345, 12346):
        out = DeviceAugmenter().apply(batch, plan=_plan([{"op": "tsnoise", "nscale": nscale, "seed": seed}])).x.cpu().double()
        noise = out - plain
        assert noise.abs().max() <= 0.05 * 0.4 * 5.8 and out.min() > 0.18 and out.max() < 0.82   # no clip acted
        n = (noise / (float(np.float32(0.05)) * rng)).reshape(-1)
        N = n.numel()
        print(f"seed {seed}: mean {n.mean():.4f} var {n.var():.4f} over {N}")
        assert abs(n.mean()) <= 4 / np.sqrt(N)                       # 4 standard errors of the mean of N(0, 1)
        assert abs(n.var() - 1.0) <= 4 * np.sqrt(2.0 / N)            # and of its variance
        fields.append(n)
    assert not torch.equal(fields[0], fields[1]) and abs(float((fields[0] * fields[1]).mean())) <= 4 / np.sqrt(N)


def test_drawn_series_plans_apply():
    """DeviceAugmenter(series_augmentations=...) end to end: what apply() draws is what it applies, twice the same."""
    from cultionet_amd.augment import SERIES_AUGMENTATIONS, DeviceAugmenter
    from cultionet_amd.edges import prepare_chips

    C, T, H, W = 2, 12, 20, 20
    x, bd = _raw(6, C, T, H, W, torch.int16, seed=11)
    y = _planes(6, H, W)
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])

    def make():
        return DeviceAugmenter(augment_prob=1.0, augmentations=(), series_augmentations=SERIES_AUGMENTATIONS, seed=4)

    batch = _batch(x, bd, y)
    out = make().apply(batch, mean, std)
    plan = make().draw(6, T, H, W, C)
    assert plan.has_series and len({plan.op(b) for b in range(6)}) >= 2
    want = make().apply(batch, mean, std, plan=plan)
    assert torch.equal(out.x, want.x) and torch.equal(make().apply(batch, mean, std).x, out.x)
    assert torch.equal(make().apply(batch, mean, std, plan=plan).x, want.x)      # a plan applies twice alike
    plain = prepare_chips(batch.x).cpu()
    labels, _ = P.label4(y)
    ident = R.identity_tables(C, T)
    tol = (BOUND / np.asarray(STD[C])).reshape(C, 1, 1, 1)
    for b in range(6):
        e = {"op": plan.op(b), "seed": plan.seed(b)}
        e.update({k: v if v is not None else i for k, v, i in zip(("pos", "drift", "nscale"), plan.series[b], ident)})
        d = np.abs(out.x[b].cpu().double().numpy() - _want(plain[b], labels[b], e, MEAN[C], STD[C]))
        assert (d <= tol).all(), (b, e["op"])


def test_feeder_yields_series_batches_and_a_step_trains_on_one():
    from cultionet_amd.augment import SERIES_AUGMENTATIONS, DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.feeder import DeviceFeeder, pin_batch
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    C, T, H, W = 3, 12, 20, 20
    mean, std = torch.tensor(MEAN[C]), torch.tensor(STD[C])

    def make():
        return DeviceAugmenter(augment_prob=1.0, augmentations=("fliplr",), series_augmentations=SERIES_AUGMENTATIONS, seed=5)

    hosts = []
    for k in range(2):
        x, bd = _raw(2, C, T, H, W, torch.int16, 20 + k)
        y = torch.from_numpy(_planes(2, H, W)).clamp(max=2)  # background 0, crop 1, edge 2, -1 unlabelled
        hosts.append(pin_batch(Data(x=x, y=y, bdist=bd)))
    got = [Data(x=b.x.clone(), bdist=b.bdist.clone(), y=b.y.clone()) for b in DeviceFeeder("cuda:0", mean=mean, std=std, augmenter=make()).iterate(hosts)]
    twin, series = make(), 0
    for h, g in zip(hosts, got):
        plan = twin.draw(2, T, H, W, C)
        series += len(plan.series_rows())
        want = twin.apply(h.to("cuda:0"), mean, std, plan=plan)
        assert torch.equal(g.x, want.x) and torch.equal(g.bdist, want.bdist) and torch.equal(g.y, want.y)
    assert series >= 2
    lit = CultionetLitModel(in_channels=C, in_time=T, hidden_channels=8, dropout=0.0).to("cuda:0").train()
    loss = HipTrainer(lit).training_step(got[0])
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.item()))


def test_launch_counts():
    from cultionet_amd.augment import DeviceAugmenter

    C, T, H, W = 1, 5, 13, 13
    x, bd = _raw(3, C, T, H, W, torch.int16, seed=3)
    batch = _batch(x, bd, _planes(3, H, W))
    shifts = np.zeros(256, dtype=np.int32)
    shifts[1:] = 1
    series = _entry("tsdrift", R.hand_tables(C, T, 1), 8)
    aug = DeviceAugmenter()
    torch.cuda.synchronize()
    for entries, most in (([{"op": "none"}, {"op": "fliplr"}, {"op": "gaussian", "sigma": 0.3}], 2),
                          ([{"op": "none"}, {"op": "roll", "shifts": shifts}, {"op": "fliplr"}], 3),
                          ([series, {"op": "roll", "shifts": shifts}, {"op": "fliplr"}], 4),
                          ([series, {"op": "none"}, {"op": "tsnoise"}], 4)):
        n0 = _launches()
        aug.apply(batch, plan=_plan(entries))
        assert 2 <= _launches() - n0 <= most, entries


# ---- refusals -------------------------------------------------------------------------------------------------------

def _series_call(x, bd, y, labels, table, packed, rows):
    """cn_augment_series_f32 itself, with the labels made beforehand: the launch counter then counts this call alone."""
    from cultionet_amd import _lib

    B, C, T, H, W = x.shape
    keep = [torch.from_numpy(np.ascontiguousarray(table)),
            torch.from_numpy(np.ascontiguousarray(packed if packed is not None else np.zeros(1), dtype=np.float32)),
            torch.from_numpy(np.asarray(rows if rows is not None else [0], dtype=np.int32))]
    dev = [k.cuda() for k in keep]
    outs = [torch.empty(x.shape, dtype=torch.float32, device="cuda"), torch.empty(bd.shape, dtype=torch.float32, device="cuda"),
            torch.empty(y.shape, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    n0 = _launches()
    try:
        _lib.call("cn_augment_series_f32", x.data_ptr(), 2, bd.data_ptr(), 2, y.data_ptr(), 4, outs[0].data_ptr(), outs[1].data_ptr(),
                  outs[2].data_ptr(), keep[0].data_ptr(), dev[0].data_ptr(), None, labels.data_ptr() if labels is not None else None,
                  None, None, keep[1].data_ptr() if packed is not None else None, dev[1].data_ptr() if packed is not None else None,
                  keep[2].data_ptr() if rows is not None else None, dev[2].data_ptr() if rows is not None else None,
                  len(rows) if rows is not None else 0, None, None, B, C, T, H, W, 1e-4, 1e-9, 1.0, None)
    finally:
        torch.cuda.synchronize()
    return _launches() - n0, outs[0]


@pytest.mark.parametrize("T", [1, 5, 65])
def test_bad_series_tables_are_refused(T):
    from cultionet_amd import _lib
    from cultionet_amd.augment import AugmentPlan, DeviceAugmenter, label_parcels
    from cultionet_amd.edges import prepare_chips

    C, H, W = 1, 9, 9
    x, bd = _raw(2, C, T, H, W, torch.int16, seed=12)
    x, bd = x.cuda(), bd.cuda()
    y = torch.from_numpy(_planes(2, H, W)).cuda()
    labels, _ = label_parcels(y)
    good = R.hand_tables(C, T, 2) if T > 1 else R.identity_tables(C, T)
    plan = _plan([{"op": "none"}, _entry("tswarp", good, 1)])
    packed = plan.pack_series(C, T)
    refuse = pytest.raises(_lib.HipKernelError, match="CN_ERR_ARG")
    if T != 5:  # a series the kernel does not hold: refused whatever the tables say, also through apply()
        with refuse:
            _series_call(x, bd, y, labels, plan.table, packed, [1])
        n0 = _launches()
        with refuse:
            _series_call(x, bd, y, labels, plan.table, packed, [1])
        assert _launches() == n0
        with refuse:
            DeviceAugmenter().apply(_batch(x, bd, y), plan=plan)
        return
    launched, out = _series_call(x, bd, y, labels, plan.table, packed, [1])   # the good call: planes, series, targets
    assert launched == 3 and torch.equal(out[0], prepare_chips(x)[0]) and not torch.equal(out[1], prepare_chips(x)[1])
    nT = 256 * T
    bad = []
    for at, value in ((nT - 1, T - 0.5), (T + 2, -0.25), (3 * T, np.nan), (nT * 2 + 7, -0.01), (nT * 2 + 9, np.nan),
                      (nT + 5 * T, np.inf), (nT + 6 * T, np.nan), (1, 1.5), (nT + 1, 0.01), (nT * 2, 0.01)):
        p = packed.copy()            # pos above T-1, below 0, NaN; nscale < 0, NaN; drift not finite; slot 0 of each table
        p[0, at] = value
        bad.append((plan.table, p, [1]))
    by_hand = AugmentPlan(2)         # the op code alone: no tables, and as a second series row none either
    by_hand.table[1, 0] = 11
    both = plan.table.copy()
    both[0, 0] = 12
    bad += [(by_hand.table, None, None), (both, packed, [1]), (plan.table, packed, [0]), (plan.table, packed, [2]),
            (plan.table, np.concatenate([packed, packed]), [1, 1])]
    n0 = _launches()
    for table, p, rows in bad:
        with refuse:
            _series_call(x, bd, y, labels, table, p, rows)
    with refuse:
        _series_call(x, bd, y, None, plan.table, packed, [1])                 # no labels
    with refuse:
        DeviceAugmenter().apply(_batch(x, bd, y), plan=by_hand)               # cn_augment_chips_f32: an unknown op, as before
    assert _launches() == n0
