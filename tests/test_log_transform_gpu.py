"""The log transform of the device prologues (the five `_log_f32` entry points, `log_transform=` of prepare_chips,
DeviceAugmenter.apply, DeviceFeeder, set_norm_values, SlidingWindowPredictor and NormValues.from_batches) against
tests/log_transform_ref.py, which tests/test_log_transform_ref.py pins to torch on the CPU.

Expected values come from the restatement, never from the kernels under test. With mean = std = None the output is w:
within 1 fp32 ulp of the float64 value and exactly fp32 1e-9 wherever u == 1. With mean / std the bound on |out - z64|,
z64 = (w64 - m) * inv, is |inv| (ulp(w) + 0.5 ulp(w - m)) + 0.5 ulp(z) (log_transform_ref.log_zscore): derived, not
measured. The augment twins are compared with the restatement applied to what the PLAIN twin (unchanged code, with its
own exact tests) writes with mean = std = None on the same plan. Every plain entry is also held bit-equal to its numpy
restatement on the same inputs: the plain instantiations did not move. Run with -s to read the err / tol ratios.

The predictor's model needs in_time >= 5 (its PreTimeReduction has a 5-tap time convolution), so that test runs a
[3, 12, 23, 17] scene through windows of 8 + 2 * 6 = 20 pixels, the shape the model's other tests run; the window kernel
itself is tested on int16 [2 * 3][23][17] with ws 6, pad 3.
"""
import numpy as np
import pytest
import torch

import log_transform_ref as LR
import parcel_ref as PR
import pointwise_ref as P
import stats_ref as SR
import ts_ref as TS
from conv_exact_worker import Flat, lib, stream
from conv_exact_worker import dev as _dev

pytestmark = pytest.mark.gpu

F = np.float32
SCALE, LO, HI = 1.0 / 10000.0, 1e-9, 1.0
GAIN, FLOOR = 50.0, 1e-9
MEAN3 = np.array([0.9, 2.1, 0.004], dtype=np.float32)   # log-domain magnitudes: values lie in [1e-9, 3.93]
STD3 = np.array([0.43, 0.88, 0.05], dtype=np.float32)
COMBOS = (("mean and std", True, True), ("mean only", True, False), ("std only", False, True), ("no z-score", False, False))
TORCH_DT = {0: torch.float32, 1: torch.int32, 2: torch.int16, 3: torch.uint16}


def _to_dev(x):
    return torch.from_numpy(x.view(np.int16) if x.dtype == np.uint16 else x).to(_dev())


def _typed(x):
    """numpy raw array -> device tensor of the dtype the Python wrappers key on."""
    t = _to_dev(x)
    return t.view(torch.uint16) if x.dtype == np.uint16 else t


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# 1. cn_prepare_chips_log_f32
# ---------------------------------------------------------------------------------------------------------------------
def _prepare_log(code, x3, mean, std, what):
    """x3: numpy [B][C][L]. One call of each entry on NaN-filled outputs: the log entry within the tolerance, the plain
    entry bit-equal to prepare_chips_ref."""
    dev, L = _dev(), lib()
    B, C, Ln = x3.shape
    xd = _to_dev(x3)
    md = None if mean is None else torch.from_numpy(mean).to(dev)
    sd = None if std is None else torch.from_numpy(std).to(dev)
    out, plain = Flat(x3.shape, dev), Flat(x3.shape, dev)
    L.call("cn_prepare_chips_log_f32", xd.data_ptr(), code, out.ptr, _ptr(md), _ptr(sd), B, C, Ln, SCALE, LO, HI, GAIN,
           FLOOR, stream())
    L.call("cn_prepare_chips_f32", xd.data_ptr(), code, plain.ptr, _ptr(md), _ptr(sd), B, C, Ln, SCALE, LO, HI, stream())
    torch.cuda.synchronize()
    LR.check(out.t.cpu().numpy(), LR.log_prepare_chips(x3, mean, std), what)
    assert torch.equal(plain.t.cpu(), torch.from_numpy(P.prepare_chips_ref(x3, mean, std, SCALE, LO, HI))), what
    out.assert_slack(what)
    plain.assert_slack(what)


@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_prepare_chips_log_all_types(code):
    """[2,3,3,21,13]: L = 819, so planes start at odd element offsets; every channel holds the clip's corners and eight of
    the bins where a contracted fma would show; mean and std given or null in every combination. The Python wrapper
    gives the same."""
    from cultionet_amd.edges import prepare_chips

    x = LR.corner_raw((2, 3, 3, 21, 13), code, 20 + code)
    for name, hm, hs in COMBOS:
        _prepare_log(code, x.reshape(2, 3, -1), MEAN3 if hm else None, STD3 if hs else None,
                     f"prepare_chips_log code {code} {name}")
    got = prepare_chips(_typed(x), torch.from_numpy(MEAN3), torch.from_numpy(STD3), log_transform=True)
    assert got.shape == x.shape and got.dtype == torch.float32
    LR.check(got.cpu().numpy(), LR.log_prepare_chips(x, MEAN3, STD3), f"prepare_chips(log_transform=True) code {code}")
    plain = prepare_chips(_typed(x), torch.from_numpy(MEAN3), torch.from_numpy(STD3))
    assert torch.equal(plain.cpu(), torch.from_numpy(P.prepare_chips_ref(x, MEAN3, STD3, SCALE, LO, HI)))


def test_prepare_chips_log_crosses_a_block_stride():
    """L = 1030: two blocks per plane, the second with six elements."""
    x = LR.corner_raw((2, 3, 1030), 2, 31)
    for name, hm, hs in COMBOS:
        _prepare_log(2, x, MEAN3 if hm else None, STD3 if hs else None, f"prepare_chips_log L 1030 {name}")


def test_prepare_chips_log_empty_and_bad_gain():
    """B = 0 is CN_OK and writes nothing; log_gain = 0, a negative one and NaN are CN_ERR_ARG and write nothing."""
    dev, L, st = _dev(), lib(), stream()
    x = torch.zeros(64, dtype=torch.int16, device=dev)
    m = torch.ones(4, device=dev)
    out = Flat((64,), dev)
    L.call("cn_prepare_chips_log_f32", x.data_ptr(), 2, out.ptr, m.data_ptr(), m.data_ptr(), 0, 4, 16, SCALE, LO, HI, GAIN,
           FLOOR, st)
    for gain in (0.0, -50.0, float("nan")):
        with pytest.raises(L.HipKernelError):
            L.call("cn_prepare_chips_log_f32", x.data_ptr(), 2, out.ptr, m.data_ptr(), m.data_ptr(), 1, 4, 16, SCALE, LO, HI,
                   gain, FLOOR, st)
    with pytest.raises(L.HipKernelError):
        L.call("cn_prepare_chips_log_f32", x.data_ptr(), 4, out.ptr, None, None, 1, 4, 16, SCALE, LO, HI, GAIN, FLOOR, st)
    torch.cuda.synchronize()
    assert bool(out.buf.isnan().all()), "an empty or refused call wrote to the output"


# ---------------------------------------------------------------------------------------------------------------------
# 2. cn_window_chips_log_f32, SlidingWindowPredictor(log_transform=True)
# ---------------------------------------------------------------------------------------------------------------------
def _windows_log(scene, wins, C, T, S, pad, mean, std):
    """The restatement's windows: window_chips_ref without a z-score gives v, log_zscore the rest. [nwin][C][T][S][S]."""
    v = P.window_chips_ref(scene, wins, T, S, pad, None, None, SCALE, LO, HI)
    return LR.log_zscore(v.reshape(len(wins), C, T, S, S), mean, std)


@pytest.mark.parametrize("name,hm,hs", COMBOS)
def test_window_chips_log_every_window(name, hm, hs):
    from cultionet_amd.predict import window_origins

    dev, L = _dev(), lib()
    C, T, H, W, ws, pad = 2, 3, 23, 17, 6, 3
    S = ws + 2 * pad
    scene = LR.corner_raw((1, C, T * H * W), 2, 41).reshape(C * T, H, W)
    wins = window_origins(H, W, ws)
    assert len(wins) == 12 and wins[-1] == (18, 12)  # ragged last row and column
    mean, std = (MEAN3[:C] if hm else None), (STD3[:C] if hs else None)
    exp = _windows_log(scene, wins, C, T, S, pad, mean, std)
    sd, wd = _to_dev(scene), torch.tensor(wins, dtype=torch.int32, device=dev)
    md = None if mean is None else torch.from_numpy(mean).to(dev)
    td = None if std is None else torch.from_numpy(std).to(dev)
    shape = (len(wins), C, T, S, S)
    out, plain = Flat(shape, dev), Flat(shape, dev)
    L.call("cn_window_chips_log_f32", sd.data_ptr(), 2, out.ptr, wd.data_ptr(), len(wins), C, T, H, W, S, pad, _ptr(md),
           _ptr(td), SCALE, LO, HI, GAIN, FLOOR, stream())
    L.call("cn_window_chips_f32", sd.data_ptr(), 2, plain.ptr, wd.data_ptr(), len(wins), C, T, H, W, S, pad, _ptr(md),
           _ptr(td), SCALE, LO, HI, stream())
    torch.cuda.synchronize()
    got = out.t.cpu().numpy()
    LR.check(got, exp, f"window_chips_log {name}")
    # zero-filled pixels: outside the scene on every side, for border, corner and ragged windows alike
    fill = np.zeros((len(wins), 1, 1, S, S), dtype=bool)
    for n, (r0, c0) in enumerate(wins):
        yy, xx = np.meshgrid(np.arange(r0 - pad, r0 - pad + S), np.arange(c0 - pad, c0 - pad + S), indexing="ij")
        fill[n, 0, 0] = (yy < 0) | (yy >= H) | (xx < 0) | (xx >= W)
    fill = np.broadcast_to(fill, shape)
    assert fill.any() and not fill.all() and exp["floor_at"][fill].all()
    m = np.zeros(C, F) if mean is None else mean
    inv = np.ones(C, F) if std is None else (F(1) / std).astype(F)
    want_fill = np.broadcast_to((((F(FLOOR) - m).astype(F)) * inv).astype(F).reshape(1, C, 1, 1, 1), shape)
    assert np.array_equal(got[fill].view(np.uint32), want_fill[fill].view(np.uint32))
    want_plain = P.window_chips_ref(scene, wins, T, S, pad, mean, std, SCALE, LO, HI).reshape(shape)
    assert torch.equal(plain.t.cpu(), torch.from_numpy(want_plain)), "the plain window entry moved"
    out.assert_slack(name)
    with pytest.raises(L.HipKernelError):
        L.call("cn_window_chips_log_f32", sd.data_ptr(), 2, out.ptr, wd.data_ptr(), len(wins), C, T, H, W, S, pad, None,
               None, SCALE, LO, HI, 0.0, FLOOR, stream())


def test_predictor_log_transform_equals_the_restatement_windows():
    """SlidingWindowPredictor(log_transform=True) against the same forward and stitch run, eagerly and in the batches as
    given, on windows the restatement prepared; and it is not the plain mosaic."""
    from cultionet_amd.lightning import CultionetLitModel
    from cultionet_amd.predict import SlidingWindowPredictor, window_origins

    dev, L = _dev(), lib()
    C, T, H, W, ws, pad, bs = 3, 12, 23, 17, 8, 6, 3
    S = ws + 2 * pad
    torch.manual_seed(3)
    lit = CultionetLitModel(in_channels=C, in_time=T, hidden_channels=8, dropout=0.0).to(dev).eval()
    scene = LR.corner_raw((1, C, T * H * W), 2, 43).reshape(C, T, H, W)
    wins = window_origins(H, W, ws)
    assert len(wins) == 9
    exp = _windows_log(scene.reshape(C * T, H, W), wins, C, T, S, pad, MEAN3, STD3)
    mean, std = torch.from_numpy(MEAN3), torch.from_numpy(STD3)
    kw = dict(window_size=ws, padding=pad, batch_size=bs, mean=mean, std=std, pixels_per_launch=0)

    # the predictor's loop with replay = False on the restatement's windows
    model = lit.cultionet_model.mask_model
    want = torch.zeros((3, H, W), dtype=torch.uint16, device=dev)
    rc = torch.tensor(wins, dtype=torch.int32, device=dev)
    xs = torch.from_numpy(exp["out"]).to(dev)
    prev = model.replay
    model.replay = False
    try:
        with torch.no_grad():
            for i in range(0, len(wins), bs):
                pred = model(xs[i:i + bs].contiguous())
                d, e, c = (pred[k].float().contiguous() for k in ("distance", "edge", "crop"))
                L.call("cn_stitch_predictions_u16", d.data_ptr(), e.data_ptr(), c.data_ptr(), want.data_ptr(),
                       rc[i:i + bs].data_ptr(), min(bs, len(wins) - i), S, pad, ws, H, W, 10000.0, stream())
    finally:
        model.replay = prev
    sd = _to_dev(scene)
    eager = SlidingWindowPredictor(lit, replay=False, log_transform=True, **kw).predict_scene(sd)
    replayed = SlidingWindowPredictor(lit, log_transform=True, **kw).predict_scene(sd)
    plain = SlidingWindowPredictor(lit, **kw).predict_scene(sd)
    torch.cuda.synchronize()
    as_i = lambda t: t.cpu().numpy().astype(np.int64)
    print("predict log: counts differing from the restatement's mosaic:", int((as_i(eager) != as_i(want)).sum()),
          "; from the plain mosaic:", int((as_i(eager) != as_i(plain)).sum()), "of", 3 * H * W)
    assert np.array_equal(as_i(eager), as_i(want))
    assert np.array_equal(as_i(replayed), as_i(want))
    assert not np.array_equal(as_i(plain), as_i(want))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the augment twins
# ---------------------------------------------------------------------------------------------------------------------
def _raw_batch(B, C, T, H, W, seed, y=None):
    from cultionet_amd.data import Data

    g = np.random.default_rng(seed)
    x = LR.corner_raw((B, C, T * H * W), 2, seed).reshape(B, C, T, H, W)
    bd = g.integers(0, 10001, (B, H, W)).astype(np.int16)
    if y is None:
        y = g.integers(-1, 4, (B, H, W))
    return Data(x=_to_dev(x), y=torch.as_tensor(np.asarray(y)).to(_dev()), bdist=_to_dev(bd))


def _plan(entries):
    from cultionet_amd.augment import AugmentPlan

    plan = AugmentPlan(len(entries))
    for b, e in enumerate(entries):
        plan.set(b, e["op"], **{k: v for k, v in e.items() if k != "op"})
    return plan


def _twins(batch, entries, C, what, null_stats_too=False):
    """The plain twin with mean = std = None gives v (the augmented, clipped values); the log twin on the same plan must
    be the restatement's log-and-z-score of that array, with bdist and y untouched."""
    from cultionet_amd.augment import DeviceAugmenter

    aug = DeviceAugmenter()
    mean, std = torch.from_numpy(MEAN3[:C]), torch.from_numpy(STD3[:C])
    n0 = lib().query("cn_launch_count", 0)
    plain = aug.apply(batch, None, None, plan=_plan(entries))
    n1 = lib().query("cn_launch_count", 0)
    got = aug.apply(batch, mean, std, plan=_plan(entries), log_transform=True)
    assert lib().query("cn_launch_count", 0) - n1 == n1 - n0  # fused into the pass that writes x: no launch more
    base = aug.apply(batch, None, None, plan=_plan([{"op": "none"}] * len(entries)))
    torch.cuda.synchronize()
    v = plain.x.cpu().numpy()
    assert v.min() >= F(LO) and v.max() <= F(HI)
    for b, e in enumerate(entries):
        assert e["op"] == "none" or not torch.equal(plain.x[b], base.x[b]), (what, e["op"])  # the op itself acted
        LR.check(got.x[b:b + 1].cpu().numpy(), LR.log_zscore(v[b:b + 1], MEAN3[:C], STD3[:C]), f"{what} {e['op']}")
    assert torch.equal(got.bdist, plain.bdist) and torch.equal(got.y, plain.y), what
    assert got.x.dtype == torch.float32 and got.y.dtype == torch.int64
    if null_stats_too:
        raw = aug.apply(batch, None, None, plan=_plan(entries), log_transform=True)
        LR.check(raw.x.cpu().numpy(), LR.log_zscore(v, None, None), f"{what} no z-score")


def test_augment_chips_log_square_chips():
    """[5,2,3,16,16], one sample per plan row: none, rot90, flipud, gaussian, saltpepper."""
    entries = [{"op": "none"}, {"op": "rot90"}, {"op": "flipud"}, {"op": "gaussian", "sigma": 0.37},
               {"op": "saltpepper", "seed": (1 << 63) | 12345}]
    _twins(_raw_batch(5, 2, 3, 16, 16, 51), entries, 2, "augment_chips_log 16x16", null_stats_too=True)


def test_augment_chips_log_two_bands():
    """36 x 36: two row bands per plane, and the blur band outgrows the rotation tile. A thread runs its loop four or five
    times here, so the unrolled body of the loops that compute in front of the store runs as well as their remainder:
    the compiler contracts the blur differently in the two, and the log twin has to follow the plain one in both (it took
    2.4 times the tolerance when its loop was not the plain kernel's). saltpepper and perlin are such loops too."""
    ang = (2 * np.pi * np.random.default_rng(8).random((2, 2, 3, 3))).astype(np.float32)
    entries = [{"op": "gaussian", "sigma": 0.25}, {"op": "cropresize", "div": 2, "top": 18, "left": 7},
               {"op": "saltpepper", "seed": 99}, {"op": "perlin", "r": 2, "theta": ang[0], "phi": ang[1]}]
    _twins(_raw_batch(4, 2, 3, 36, 36, 52), entries, 2, "augment_chips_log 36x36")


def test_augment_parcels_log_roll():
    T = 6
    y = np.stack([PR.classes_field(16, 16, 50), PR.classes_field(16, 16, 51)])
    assert min(PR.label4(p)[1] for p in y) >= 2
    shifts = np.zeros(256, dtype=np.int32)
    shifts[1:] = np.random.default_rng(5).integers(-(T - 1), T, 255)
    assert (shifts != 0).any()
    _twins(_raw_batch(2, 2, T, 16, 16, 53, y), [{"op": "roll", "shifts": shifts}, {"op": "none"}], 2,
           "augment_parcels_log")


def test_augment_series_log():
    """A tswarp and a tspeaks sample at T = 6, and the two other series ops beside them."""
    C, T = 2, 6
    y = np.stack([PR.classes_field(16, 16, 60 + k) for k in range(5)])
    entries = []
    for k, op in enumerate(("tswarp", "tspeaks", "tsnoise", "tsdrift")):
        pos, drift, nscale = TS.hand_tables(C, T, 70 + k)
        entries.append({"op": op, "pos": pos, "drift": drift, "nscale": nscale, "seed": (1 << 40) + k})
    entries.append({"op": "fliplr"})
    _twins(_raw_batch(5, C, T, 16, 16, 54, y), entries, C, "augment_series_log")


def test_augment_log_bad_gain_is_refused():
    """log_gain = 0 is CN_ERR_ARG before anything is launched, through all three twins (they share one launcher)."""
    dev, L = _dev(), lib()
    B, C, T, H, W = 1, 1, 2, 4, 4
    x = torch.zeros((B, C, T, H, W), dtype=torch.int16, device=dev)
    y = torch.zeros((B, H, W), dtype=torch.int64, device=dev)
    table = np.zeros((B, 8), dtype=np.int32)
    td = torch.from_numpy(table).to(dev)
    out, yo = Flat(x.shape, dev), torch.full((B, H, W), -7, dtype=torch.int64, device=dev)
    head = (x.data_ptr(), 2, None, 0, y.data_ptr(), 4, out.ptr, None, yo.data_ptr(), table.ctypes.data, td.data_ptr(), None)
    tail = (None, None, B, C, T, H, W, SCALE, LO, HI, 0.0, FLOOR, stream())
    n0 = L.query("cn_launch_count", 0)
    for name, mid in (("cn_augment_chips_log_f32", ()), ("cn_augment_parcels_log_f32", (None, None, None)),
                      ("cn_augment_series_log_f32", (None, None, None, None, None, None, None, 0))):
        with pytest.raises(L.HipKernelError):
            L.call(name, *head, *mid, *tail)
    assert L.query("cn_launch_count", 0) == n0
    torch.cuda.synchronize()
    assert bool(out.buf.isnan().all()) and bool((yo == -7).all())


def test_default_apply_draws_and_writes_what_it_did():
    """DeviceAugmenter(seed=42).apply(batch) without the flag: torch.equal to cn_augment_chips_f32 called by hand with the
    plan a second generator of the same seed draws."""
    from cultionet_amd.augment import DeviceAugmenter

    dev, L = _dev(), lib()
    B, C, T, H, W = 8, 2, 3, 20, 20
    batch = _raw_batch(B, C, T, H, W, 55)
    mean, std = torch.from_numpy(MEAN3[:C]).to(dev), torch.from_numpy(STD3[:C]).to(dev)
    got = DeviceAugmenter(seed=42).apply(batch, mean, std)
    plan = DeviceAugmenter(seed=42).draw(B, T, H, W, C)
    assert len({plan.op(b) for b in range(B)}) >= 3 and not plan.has_parcel and not plan.has_series
    table = np.ascontiguousarray(plan.table)
    td, pd = torch.from_numpy(table).to(dev), torch.from_numpy(np.ascontiguousarray(plan.perlin)).to(dev)
    xo, bo = Flat((B, C, T, H, W), dev), Flat((B, H, W), dev)
    yo = torch.empty((B, H, W), dtype=torch.int64, device=dev)
    L.call("cn_augment_chips_f32", batch.x.data_ptr(), 2, batch.bdist.data_ptr(), 2, batch.y.data_ptr(), 4, xo.ptr, bo.ptr,
           yo.data_ptr(), table.ctypes.data, td.data_ptr(), pd.data_ptr(), mean.data_ptr(), std.data_ptr(), B, C, T, H, W,
           SCALE, LO, HI, stream())
    torch.cuda.synchronize()
    assert torch.equal(got.x, xo.t) and torch.equal(got.bdist, bo.t) and torch.equal(got.y, yo)


# ---------------------------------------------------------------------------------------------------------------------
# 4. DeviceFeeder(log_transform=True) and the Lightning hook
# ---------------------------------------------------------------------------------------------------------------------
def _host_batches():
    from cultionet_amd.data import Data
    from cultionet_amd.feeder import pin_batch

    out = []
    for k in range(2):
        g = np.random.default_rng(80 + k)
        x = LR.corner_raw((2, 3, 3 * 16 * 16), 2, 60 + k).reshape(2, 3, 3, 16, 16)
        out.append(pin_batch(Data(x=torch.from_numpy(x), y=torch.from_numpy(g.integers(-1, 4, (2, 16, 16))),
                                  bdist=torch.from_numpy(g.integers(0, 10001, (2, 16, 16)).astype(np.int16)))))
    return out


def _check_fed(b, h, what):
    LR.check(b.x.cpu().numpy(), LR.log_prepare_chips(h.x.numpy(), MEAN3, STD3), what)
    want_bd = P.prepare_chips_ref(h.bdist.numpy()[:, None], None, None, SCALE, LO, HI)[:, 0]
    assert torch.equal(b.bdist.cpu(), torch.from_numpy(want_bd)), what   # bdist is never transformed
    assert torch.equal(b.y.cpu(), h.y) and b.y.dtype == torch.int64, what


def test_feeder_and_lightning_hook_log_transform():
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.feeder import DeviceFeeder
    from cultionet_amd.lightning import CultionetLitModel

    dev = _dev()
    hosts = _host_batches()
    mean, std = torch.from_numpy(MEAN3), torch.from_numpy(STD3)
    for name, aug in (("plain prologue", None), ("augmenter at augment_prob 0", DeviceAugmenter(augment_prob=0.0))):
        feeder = DeviceFeeder(dev, mean=mean, std=std, augmenter=aug, log_transform=True)
        seen = 0
        for i, b in enumerate(feeder.iterate(hosts)):
            _check_fed(b, hosts[i], f"feeder {name} batch {i}")
            seen += 1
        assert seen == 2
    off = next(iter(DeviceFeeder(dev, mean=mean, std=std).iterate(hosts)))
    assert torch.equal(off.x.cpu(), torch.from_numpy(P.prepare_chips_ref(hosts[0].x.numpy(), MEAN3, STD3, SCALE, LO, HI)))

    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, dropout=0.0)
    lit.set_norm_values(mean, std, log_transform=True)
    on_dev = lambda h: Data(x=h.x.to(dev), y=h.y.to(dev), bdist=h.bdist.to(dev))
    lit.eval()
    _check_fed(lit.on_after_batch_transfer(on_dev(hosts[0])), hosts[0], "hook, plain branch")
    lit.set_augmenter(DeviceAugmenter(augment_prob=0.0))
    lit.train()
    _check_fed(lit.on_after_batch_transfer(on_dev(hosts[1])), hosts[1], "hook, augmenter branch")
    lit.set_norm_values(mean, std)  # the default switches it off again
    out = lit.on_after_batch_transfer(on_dev(hosts[1]))
    assert torch.equal(out.x.cpu(), torch.from_numpy(P.prepare_chips_ref(hosts[1].x.numpy(), MEAN3, STD3, SCALE, LO, HI)))


# ---------------------------------------------------------------------------------------------------------------------
# 5. NormValues.from_batches(log_transform=True)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "flat", "odd"])
def test_from_batches_log_transform(golden_dir, name):
    """On the golden's raw batches: equal to stats_from_counts on host-side counts exactly, and to the reference's own
    outputs within the bounds of tests/test_log_transform_ref.py (std 1e-6 relative; quantiles 2 fp32 ulp)."""
    from cultionet_amd import normalize as N
    from cultionet_amd.data import Data

    golden = dict(np.load(f"{golden_dir}/dataset_stats.npz"))
    golden_log = dict(np.load(f"{golden_dir}/dataset_stats_log.npz"))
    xs = SR.batches_of(golden, name)
    ys = SR.labels_for(xs)
    host = [Data(x=torch.from_numpy(x), y=torch.from_numpy(y)) for x, y in zip(xs, ys)]
    nv = N.NormValues.from_batches(host, "cuda", SR.CLASS_INFO, log_transform=True)
    records, hist = SR.device_counts(xs, N.bin_weights(log_transform=True), N.NBINS)
    want = N.NormValues.from_counts(records, hist, SR.label_counts(ys, SR.CLASS_INFO["edge_class"] + 1), SR.CLASS_INFO,
                                    log_transform=True)
    for k, v in want.data_dict.items():
        w = nv.data_dict[k]
        assert torch.equal(v, w) if isinstance(v, torch.Tensor) else v == w, k
    plain = N.NormValues.from_batches(host, "cuda", SR.CLASS_INFO)
    assert torch.equal(plain.dataset_crop_counts, nv.dataset_crop_counts)
    if name != "flat":
        assert not torch.equal(plain.dataset_mean, nv.dataset_mean)

    got = N.stats_from_counts(records, hist, np.zeros(6, dtype=np.int64), SR.CLASS_INFO, "median", 0.05, 0.95, True)
    assert np.array_equal(nv.dataset_std.reshape(-1).numpy(), got["std"].astype(np.float32))
    ref_std = golden_log[f"{name}_std"].astype(np.float64)
    nz = ref_std != 0
    assert np.all(got["std"][~nz] == 0)
    assert np.max(np.abs(got["std"][nz] / ref_std[nz] - 1), initial=0.0) <= SR.STD_RTOL
    q = np.stack([got["lower_bound"], got["mean"], got["upper_bound"]], axis=1)
    ref_q = golden_log[f"{name}_quantiles"]
    assert np.max(np.abs(q - ref_q.astype(np.float64)) / np.spacing(np.abs(ref_q)).astype(np.float64)) <= 2.0

    with pytest.raises(ValueError):
        N.DatasetStats(len(ref_std), SR.CLASS_INFO, "cuda", log_transform=True).finish(log_transform=False)
