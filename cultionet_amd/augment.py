"""Device-side training augmentation for raw batches (the fused prologues ``cn_augment_chips_f32``,
``cn_augment_parcels_f32`` and ``cn_augment_series_f32``, and the parcel labelling ``cn_label_parcels_i32``).

``EdgeDataset.get`` (data/datasets.py:443-488 of the reference) augments a labelled training sample with
probability ``augment_prob`` by ONE augmenter drawn uniformly from its list, between the ``/10000 -> clip`` step and the
z-score, per sample on the CPU. Here the same pipeline runs as one pass over the collated RAW batch on the device:

  * the discrete choices and small parameters (augment or not, which op, blur sigma, crop geometry, Perlin resolution and
    gradient angles, the noise seed) are drawn on the HOST by one seeded ``numpy.random.Generator`` and packed into a
    fixed-layout plan table (``AugmentPlan``), copied to the device on the stream the batch is staged on;
  * the kernels apply the plan; only the per-element noise of ``saltpepper`` is generated on the device, counter-based
    from the plan's seed, so the pass keeps no state and a given plan always gives the same batch.

Covered: rot90, rot180, rot270, fliplr, flipud, gaussian, saltpepper, cropresize, perlin (augment/augmenters.py:166-330).
The five parcel-based augmenters (tswarp, tsnoise, tsdrift, tspeaks, roll) warp each labelled parcel separately: they need
the connected components of the crop pixels of ``y``, which ``label_parcels`` computes on the device. ``roll``
(augment/augmenters.py:154-163) is an opt-in (``DeviceAugmenter(parcel_augmentations=("roll",))``): one shift per parcel is
drawn on the host into ``AugmentPlan.parcel``.

The four ``ts*`` augmenters (augment/augmenters.py:51-151, augment_time, augment/augmenter_utils.py:111-165) are a third
opt-in, ``DeviceAugmenter(series_augmentations=SERIES_AUGMENTATIONS)``. The reference runs them through ``tsaug``
(``TimeWarp``, ``Drift``, ``AddNoise``, with ``static_rand=True``). The work is split as for ``roll``:

  * the DEVICE op (``cn_augment_series_f32``) applies curves that arrive with the plan, per parcel slot ``label & 255``:
    source times ``pos`` [256, T], ``drift`` [256, C, T] and a noise scale ``nscale`` [256]; only the per-element normal
    noise is generated on the device, with the counter of ``saltpepper``. It is pinned to a float64 restatement and to the
    reference's own ``augment_time`` / ``insert_parcel`` / ``tspeaks`` code run with stand-in warpers
    (tools/make_series_golden.py, tests/golden/augment_series.npz);
  * the HOST draw produces the curves, following tsaug's published ``TimeWarp`` / ``Drift`` / ``AddNoise`` algorithms with
    the interpolators of ``cultionet_amd.curves`` (pinned to scipy's). ``static_rand=True`` is read as one random curve
    per ``augment`` call, i.e. per parcel, shared by all pixels of the parcel.

NOT pinned against the reference: the draw of the curves. The reference pins a fork of ``tsaug`` that is not installed
where this package is built and tested, so the draw has not been run against it; its random stream is unseeded upstream,
so only the distributions could agree in any case.
"""
from __future__ import annotations

import typing as T

import numpy as np
import torch

from . import _lib
from .curves import cubic_spline, pchip
from .data import Data
from .edges import _DTYPES, LOG_FLOOR, LOG_GAIN, SCALE_FACTOR, prepare_chips
from .engine import _stream

OPS = ("none", "rot90", "rot180", "rot270", "fliplr", "flipud", "gaussian", "saltpepper", "cropresize", "perlin")
OP_CODES = {name: code for code, name in enumerate(OPS)}
DEVICE_AUGMENTATIONS = OPS[1:]
HOST_AUGMENTATIONS = ("tswarp", "tsnoise", "tsdrift", "tspeaks", "roll")  # what ``augmentations=`` refuses
PARCEL_AUGMENTATIONS = ("roll",)  # opt-in through ``parcel_augmentations=``: they label the parcels of y first
PARCEL_OP_CODES = {name: len(OPS) + k for k, name in enumerate(PARCEL_AUGMENTATIONS)}
SERIES_AUGMENTATIONS = ("tswarp", "tsnoise", "tsdrift", "tspeaks")  # opt-in through ``series_augmentations=``
SERIES_OP_CODES = {name: len(OPS) + len(PARCEL_AUGMENTATIONS) + k for k, name in enumerate(SERIES_AUGMENTATIONS)}
SERIES_SLOTS = 256  # curves per sample, indexed by label & 255 as the shifts of ``roll``
SERIES_TMAX = 64  # longest series the device op holds; the shortest is 2
_NAMES = OPS + PARCEL_AUGMENTATIONS + SERIES_AUGMENTATIONS  # by op code

PLAN_WORDS = 8  # op, div, top, left, r, sigma (float bits), seed low word, seed high word
PERLIN_RES = (2, 5, 10)
PERLIN_RMAX = 10
PERLIN_FLOATS = 4 * (PERLIN_RMAX + 1) ** 2  # theta [2][r+1][r+1] then phi [2][r+1][r+1], compact, per sample
PARCEL_SHIFTS = 256  # shifts per sample, indexed by label & 255: the reference holds its segments as uint8
_Y_DTYPES = {torch.int32: 1, torch.int16: 2, torch.uint16: 3, torch.int64: 4}


class AugmentPlan:
    """What one batch's augmentation does, as host arrays: ``table`` int32 [B, PLAN_WORDS] and ``perlin`` float32
    [B, PERLIN_FLOATS] (angles; rows of samples that are not ``perlin`` stay zero), and ``parcel`` int32
    [B, PARCEL_SHIFTS] (the shift of parcel k at [k & 255]; rows of samples that are not ``roll`` stay zero), and
    ``series``, {b: (pos, drift, nscale)} for the samples that ``set`` gave a series op (None stands for an identity
    table; they are packed, for those samples only, when the plan is applied). A fresh plan is all ``none``."""

    def __init__(self, B: int):
        self.table = np.zeros((B, PLAN_WORDS), dtype=np.int32)
        self.perlin = np.zeros((B, PERLIN_FLOATS), dtype=np.float32)
        self.parcel = np.zeros((B, PARCEL_SHIFTS), dtype=np.int32)
        self._parcel_rows = np.zeros(B, dtype=bool)  # rows that set() gave a parcel op and its shifts
        self.series: T.Dict[int, T.Tuple[T.Optional[np.ndarray], T.Optional[np.ndarray], T.Optional[np.ndarray]]] = {}

    def __len__(self) -> int:
        return self.table.shape[0]

    def set(self, b: int, op: str, *, sigma: float = 0.0, div: int = 0, top: int = 0, left: int = 0, r: int = 0,
            theta: T.Optional[np.ndarray] = None, phi: T.Optional[np.ndarray] = None, seed: int = 0,
            shifts: T.Optional[np.ndarray] = None, pos: T.Optional[np.ndarray] = None,
            drift: T.Optional[np.ndarray] = None, nscale: T.Optional[np.ndarray] = None) -> "AugmentPlan":
        """Sample ``b`` gets ``op``. gaussian: sigma; cropresize: div, top, left; saltpepper: seed (64 bit);
        perlin: r and the angle tables theta, phi [2, r+1, r+1]; roll: shifts, 256 integers with shifts[0] == 0
        (parcel k rolls by shifts[k & 255]; their range against T is checked when the plan is applied);
        tswarp, tsnoise, tsdrift, tspeaks: float32 tables pos [256, T], drift [256, C, T], nscale [256] and the noise seed
        (a table left out is the identity: pos 0..T-1, drift 0, nscale 0; slot 0 must hold the identity; their values and
        their T and C against the batch are checked when the plan is applied)."""
        if op in SERIES_OP_CODES:
            tables = _series_tables(op, pos, drift, nscale)  # raises before the row is touched
        elif pos is not None or drift is not None or nscale is not None:
            raise ValueError(f"pos, drift and nscale belong to {SERIES_AUGMENTATIONS}, not to {op!r}")
        row = self.table[b]
        row[:] = 0
        self.perlin[b] = 0.0
        self.parcel[b] = 0
        self._parcel_rows[b] = False
        self.series.pop(int(b), None)
        if op in SERIES_OP_CODES:
            row[0] = SERIES_OP_CODES[op]
            row[6:8].view(np.uint32)[:] = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
            self.series[int(b)] = tables
            return self
        if op in PARCEL_OP_CODES:
            sh = np.asarray(shifts if shifts is not None else ())
            if sh.shape != (PARCEL_SHIFTS,) or not np.issubdtype(sh.dtype, np.integer):
                raise ValueError(f"{op} needs shifts: {PARCEL_SHIFTS} integers, the one of the background first")
            row[0] = PARCEL_OP_CODES[op]
            self.parcel[b] = sh
            self._parcel_rows[b] = True
            return self
        row[0] = OP_CODES[op]
        row[1], row[2], row[3], row[4] = div, top, left, r
        row[5:6].view(np.float32)[0] = sigma
        row[6:8].view(np.uint32)[:] = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        if op == "perlin":
            n = 2 * (r + 1) ** 2
            if not 1 <= r <= PERLIN_RMAX or np.size(theta) != n or np.size(phi) != n:
                raise ValueError("perlin needs 1 <= r <= 10 and angle tables theta, phi of shape [2, r+1, r+1]")
            self.perlin[b, :n] = np.asarray(theta, dtype=np.float32).reshape(-1)
            self.perlin[b, n:2 * n] = np.asarray(phi, dtype=np.float32).reshape(-1)
        return self

    def op(self, b: int) -> str:
        return _NAMES[int(self.table[b, 0])]

    def seed(self, b: int) -> int:
        lo, hi = (int(v) for v in self.table[b, 6:8].view(np.uint32))
        return (hi << 32) | lo

    @property
    def has_perlin(self) -> bool:
        return bool((self.table[:, 0] == OP_CODES["perlin"]).any())

    @property
    def has_parcel(self) -> bool:
        """Whether a sample was given a parcel op through ``set``: the batch is then labelled before it is augmented.
        (A parcel op code written into ``table`` by hand has no shifts; the entry point refuses it as an unknown op.)"""
        return bool((self._parcel_rows & (self.table[:, 0] >= len(OPS))).any())

    def series_rows(self) -> T.List[int]:
        """The samples that ``set`` gave a series op, in order: one row of the packed tables each."""
        lo = len(OPS) + len(PARCEL_AUGMENTATIONS)
        return [b for b in sorted(self.series) if lo <= int(self.table[b, 0]) < lo + len(SERIES_AUGMENTATIONS)]

    @property
    def has_series(self) -> bool:
        """Whether a sample was given a series op through ``set``: the batch is then labelled and goes through
        ``cn_augment_series_f32``. (A series op code written into ``table`` by hand has no tables; the entry points
        refuse it as an unknown op.)"""
        return bool(self.series) and bool(self.series_rows())

    def pack_series(self, C: int, T_: int) -> np.ndarray:
        """The tables of the series samples for a batch of C channels and T_ times, as the device op reads them: float32
        [rows, 256 * (T_ + C * T_ + 1)], per row pos [256, T_], drift [256, C, T_], nscale [256]."""
        rows = self.series_rows()
        return self._pack_series(C, T_, rows, np.empty((len(rows), SERIES_SLOTS * (T_ + C * T_ + 1)), dtype=np.float32))

    def _pack_series(self, C: int, T_: int, rows: T.Sequence[int], out: np.ndarray) -> np.ndarray:
        """``pack_series`` of the samples ``rows`` into ``out`` [len(rows), 256 * (T_ + C * T_ + 1)], every element of it."""
        out[:, SERIES_SLOTS * T_:] = 0.0
        for r, b in enumerate(rows):
            pos, drift, nscale = self.series[b]
            if pos is not None and pos.shape != (SERIES_SLOTS, T_):
                raise ValueError(f"sample {b}: pos is {pos.shape}, the batch needs {(SERIES_SLOTS, T_)}")
            if drift is not None and drift.shape != (SERIES_SLOTS, C, T_):
                raise ValueError(f"sample {b}: drift is {drift.shape}, the batch needs {(SERIES_SLOTS, C, T_)}")
            out[r, :SERIES_SLOTS * T_].reshape(SERIES_SLOTS, T_)[:] = np.arange(T_, dtype=np.float32) if pos is None else pos
            if drift is not None:
                out[r, SERIES_SLOTS * T_:SERIES_SLOTS * T_ * (1 + C)] = drift.reshape(-1)
            if nscale is not None:
                out[r, SERIES_SLOTS * T_ * (1 + C):] = nscale
        return out


def _series_tables(op, pos, drift, nscale):
    """The tables of a series op as ``AugmentPlan.set`` keeps them (copies; None where left out), shapes and dtypes checked."""
    out = []
    for name, a, ndim in (("pos", pos, 2), ("drift", drift, 3), ("nscale", nscale, 1)):
        if a is not None:
            a = np.asarray(a)
            if a.dtype != np.float32 or a.ndim != ndim or a.shape[0] != SERIES_SLOTS:
                raise ValueError(f"{op} needs {name} as float32 with {ndim} axes, the first of {SERIES_SLOTS} slots: pos "
                                 "[256, T], drift [256, C, T], nscale [256]")
            a = np.ascontiguousarray(a).copy()
        out.append(a)
    if out[0] is not None and out[1] is not None and out[0].shape[1] != out[1].shape[2]:
        raise ValueError(f"{op}: pos holds {out[0].shape[1]} times, drift {out[1].shape[2]}")
    return tuple(out)


class DeviceAugmenter:
    """``DeviceAugmenter(augment_prob=0.5, augmentations=DEVICE_AUGMENTATIONS, seed=42, parcel_augmentations=(),
    series_augmentations=())``: draws one plan per batch and applies it on the device. Hand it to
    ``DeviceFeeder(augmenter=...)`` or ``CultionetLitModel.set_augmenter``. ``parcel_augmentations`` (names of
    PARCEL_AUGMENTATIONS) and ``series_augmentations`` (names of SERIES_AUGMENTATIONS) join the candidates of the draw, in
    that order; a batch in which one of them is drawn is labelled on the device first (``label_parcels``).
    ``crop_value`` is the class of ``y`` whose connected components are the parcels."""

    def __init__(self, augment_prob: float = 0.5, augmentations: T.Sequence[str] = DEVICE_AUGMENTATIONS, seed: int = 42,
                 parcel_augmentations: T.Sequence[str] = (), crop_value: int = 1,
                 series_augmentations: T.Sequence[str] = ()):
        for name in augmentations:
            if name in HOST_AUGMENTATIONS:
                raise NotImplementedError(
                    f"{name!r} warps each labelled parcel on the host (connected components of y, tsaug): it has no "
                    "device counterpart; augment those samples per sample on the host and feed float batches")
            if name not in OP_CODES:
                raise KeyError(name)  # as AUGMENTER_METHODS[name] (augment/augmenters.py:341-357, 423)
        for name in parcel_augmentations:
            if name in SERIES_AUGMENTATIONS:
                raise NotImplementedError(
                    f"{name!r} is a tsaug transform (TimeWarp / Drift / AddNoise) applied per parcel, not a parcel shift: "
                    "enable it through series_augmentations=")
            if name not in PARCEL_OP_CODES:
                raise KeyError(name)
        for name in series_augmentations:
            if name not in SERIES_OP_CODES:
                raise KeyError(name)
        if not 0.0 <= augment_prob <= 1.0:
            raise ValueError("augment_prob must lie in [0, 1]")
        self.augment_prob = float(augment_prob)
        self.augmentations = tuple(augmentations)
        self.parcel_augmentations = tuple(parcel_augmentations)
        self.series_augmentations = tuple(series_augmentations)
        self.crop_value = int(crop_value)
        self.rng = np.random.default_rng(seed)

    def _candidates(self, H: int, W: int, T_: int = 2) -> T.Tuple[T.List[str], T.List[int]]:
        if H != W and ("rot90" in self.augmentations or "rot270" in self.augmentations):
            raise ValueError(f"rot90 / rot270 need square chips, got {H} x {W}: drop them from the augmentations")
        res = [r for r in PERLIN_RES if H % r == 0 and W % r == 0]
        names = [n for n in self.augmentations if n != "none" and (n != "perlin" or res)]
        if "cropresize" in names and (H < 2 or W < 2):
            names.remove("cropresize")
        if "gaussian" in names and (H < 2 or W < 2):
            names.remove("gaussian")
        series = self.series_augmentations if 2 <= T_ <= SERIES_TMAX else ()  # the device op holds 2 to 64 times
        return names + list(self.parcel_augmentations) + list(series), res

    def _draw_warp(self, T_: int) -> np.ndarray:
        """tsaug.TimeWarp(n_speed_change=n, max_speed_ratio=R), n and R per sample (augmenters.py:85-97), one curve per
        slot: n + 1 speeds with max / min = R, their running sum as the source time at the knots, PCHIP between."""
        rng = self.rng
        n = int(rng.integers(1, 3))
        R = float(rng.uniform(1.1, 1.5))
        a = rng.random((SERIES_SLOTS - 1, n + 1))
        a = a - (a.max(axis=1, keepdims=True) - R * a.min(axis=1, keepdims=True)) / (1.0 - R)
        values = np.concatenate((np.zeros((SERIES_SLOTS - 1, 1)), np.cumsum(a, axis=1)), axis=1)
        values = values / values[:, -1:] * (T_ - 1)
        knots = np.concatenate(([0.0], (0.5 + np.arange(n)) / n * (T_ - 1), [T_ - 1.0]))
        pos = np.empty((SERIES_SLOTS, T_), dtype=np.float32)
        pos[0] = np.arange(T_)
        pos[1:] = np.clip(pchip(knots, values, np.arange(T_)), 0.0, T_ - 1.0)
        return pos

    def _draw_drift(self, C: int, T_: int) -> np.ndarray:
        """tsaug.Drift(max_drift, n_drift_points=m), both per sample (augmenters.py:139-151), one curve per slot and
        channel: a random walk over m + 2 knots on [0, T_], a cubic spline through it, anchored at 0 and scaled so that
        its largest magnitude is max_drift (of the series' range, which the device op multiplies in)."""
        rng = self.rng
        max_drift = float(rng.uniform(0.05, 0.1))
        m = int(rng.integers(1, 6))
        anchors = np.cumsum(rng.normal(size=(SERIES_SLOTS - 1, C, m + 2)), axis=-1)
        curve = cubic_spline(np.linspace(0.0, T_, m + 2), anchors, np.arange(T_))
        curve = curve - curve[..., :1]
        curve = curve / np.abs(curve).max(axis=-1, keepdims=True) * max_drift
        drift = np.zeros((SERIES_SLOTS, C, T_), dtype=np.float32)
        drift[1:] = curve
        return drift

    def _draw_series(self, plan: AugmentPlan, b: int, name: str, C: int, T_: int) -> None:
        rng = self.rng
        pos = drift = None
        nscale = np.zeros(SERIES_SLOTS, dtype=np.float32)
        if name == "tsnoise":  # AddNoise(scale) is the warper itself: one scale per sample (augmenters.py:114-118)
            nscale[1:] = rng.uniform(0.01, 0.05)
        else:
            if name == "tsdrift":
                drift = self._draw_drift(C, T_)
            else:
                pos = self._draw_warp(T_)
            nscale[1:] = rng.uniform(0.01, 0.05, SERIES_SLOTS - 1)  # add_noise_: one draw per prop (augmenter_utils.py:151-153)
        plan.set(b, name, pos=pos, drift=drift, nscale=nscale, seed=int(rng.integers(0, 2 ** 63)))

    def draw(self, B: int, T_: int, H: int, W: int, C: T.Optional[int] = None) -> AugmentPlan:
        """The plan of one batch of B samples [C, T_, H, W]: B sequential per-sample draws from the augmenter's
        generator (augment or not as datasets.py:449, the op as datasets.py:451, then the op's own parameters). ``C`` is
        needed where ``tsdrift`` is a candidate, and required then: its curves are per channel."""
        names, res = self._candidates(H, W, T_)
        if C is None and "tsdrift" in names:
            raise ValueError("draw() needs the number of channels C when tsdrift is a candidate: its curves are per channel")
        plan = AugmentPlan(B)
        rng = self.rng
        for b in range(B):
            if not (rng.random() > 1.0 - self.augment_prob) or not names:
                continue
            name = names[int(rng.integers(len(names)))]
            if name == "gaussian":  # v2.GaussianBlur(kernel_size=3, sigma=(0.2, 0.5)): one sigma per call
                plan.set(b, name, sigma=float(rng.uniform(0.2, 0.5)))
            elif name == "saltpepper":
                plan.set(b, name, seed=int(rng.integers(0, 2 ** 63)))
            elif name == "cropresize":  # augmenters.py:247-248; v2.RandomCrop: uniform integer offsets
                divs = [d for d in (2, 4) if H // d >= 1 and W // d >= 1]
                div = int(divs[int(rng.integers(len(divs)))])
                h, w = H // div, W // div
                plan.set(b, name, div=div, top=int(rng.integers(0, H - h + 1)), left=int(rng.integers(0, W - w + 1)))
            elif name == "perlin":  # augmenters.py:172; augmenter_utils.py:272-275: angles 2 pi U[0, 1)
                r = int(res[int(rng.integers(len(res)))])
                ang = (2.0 * np.pi * rng.random((2, 2, r + 1, r + 1))).astype(np.float32)
                plan.set(b, name, r=r, theta=ang[0], phi=ang[1])
            elif name == "roll":  # augmenter_utils.py:180-182, one draw per prop; 255 is all np.uint8 segments can hold
                q = int(T_ * 0.25)
                shifts = np.zeros(PARCEL_SHIFTS, dtype=np.int32)
                shifts[1:] = rng.integers(-q, q + 1, PARCEL_SHIFTS - 1)
                plan.set(b, name, shifts=shifts)
            elif name in SERIES_OP_CODES:
                self._draw_series(plan, b, name, C, T_)
            else:
                plan.set(b, name)
        return plan

    def apply(self, batch: Data, mean: T.Optional[torch.Tensor] = None, std: T.Optional[torch.Tensor] = None,
              plan: T.Optional[AugmentPlan] = None, scale: float = 1.0 / SCALE_FACTOR, lo: float = 1e-9,
              hi: float = 1.0, log_transform: bool = False) -> Data:
        """Raw device batch -> prepared Data (x fp32 z-scored, bdist fp32, y int64) with ``plan`` (default: a fresh
        ``draw``) applied, on the current stream. A batch without labels passes through the plain prologue: the
        reference only augments labelled samples (datasets.py:448). ``log_transform``: the reference's
        ``--log-transform`` (datasets.py:481-484) on x, after the augmentation's last clip and before the z-score, in the
        same launches (the ``_log_f32`` entry points); bdist and y are not transformed, the draw is the same."""
        x = batch.x
        if not x.is_cuda:
            raise RuntimeError("DeviceAugmenter.apply needs a device batch")
        if x.dtype not in _DTYPES:
            raise TypeError(f"unsupported raw dtype {x.dtype}")
        kw = dict(batch.__dict__)
        bd = kw.get("bdist")
        y = kw.get("y")
        if y is None:
            kw["x"] = prepare_chips(x, mean, std, scale, lo, hi, log_transform)
            if bd is not None and bd.dtype != torch.float32:
                kw["bdist"] = prepare_chips(bd.reshape(bd.shape[0], 1, 1, *bd.shape[1:]), None, None, scale, lo,
                                            hi).reshape(bd.shape)
            return Data(**kw)
        B, C, Tn, H, W = x.shape
        if plan is None:
            plan = self.draw(B, Tn, H, W, C)
        if len(plan) != B:
            raise ValueError(f"the plan holds {len(plan)} samples, the batch {B}")
        codes = plan.table[:, 0]
        if H != W and bool(((codes == OP_CODES["rot90"]) | (codes == OP_CODES["rot270"])).any()):
            raise ValueError(f"rot90 / rot270 need square chips, got {H} x {W}")
        if y.dtype not in _Y_DTYPES:
            raise TypeError(f"unsupported label dtype {y.dtype}")
        if tuple(y.shape) != (B, H, W) or (bd is not None and tuple(bd.shape) != (B, H, W)):
            raise ValueError("y and bdist must be [B, H, W]")
        if bd is not None and bd.dtype not in _DTYPES:
            raise TypeError(f"unsupported raw bdist dtype {bd.dtype}")
        if bd is not None and (bd.dtype == torch.float32) != (x.dtype == torch.float32):
            raise TypeError("x and bdist must both be raw (one scale serves both)")
        dev = x.device
        x, y = x.contiguous(), y.contiguous()
        bd = bd.contiguous() if bd is not None else None
        m = mean.to(device=dev, dtype=torch.float32).reshape(-1).contiguous() if mean is not None else None
        s = std.to(device=dev, dtype=torch.float32).reshape(-1).contiguous() if std is not None else None
        if m is not None and m.numel() != C:
            raise ValueError("mean must hold one value per channel")
        # the plan goes through pinned memory so that its copy is one more asynchronous copy on this stream
        table_h = torch.from_numpy(np.ascontiguousarray(plan.table)).pin_memory()
        table_d = table_h.to(dev, non_blocking=True)
        perlin_d = None
        if plan.has_perlin:
            perlin_d = torch.from_numpy(np.ascontiguousarray(plan.perlin)).pin_memory().to(dev, non_blocking=True)
        x_out = torch.empty(x.shape, dtype=torch.float32, device=dev)
        bd_out = torch.empty(bd.shape, dtype=torch.float32, device=dev) if bd is not None else None
        y_out = torch.empty(y.shape, dtype=torch.int64, device=dev)
        head = (x.data_ptr(), _DTYPES[x.dtype], bd.data_ptr() if bd is not None else None,
                _DTYPES[bd.dtype] if bd is not None else 0, y.data_ptr(), _Y_DTYPES[y.dtype], x_out.data_ptr(),
                bd_out.data_ptr() if bd is not None else None, y_out.data_ptr(), table_h.data_ptr(),
                table_d.data_ptr(), perlin_d.data_ptr() if perlin_d is not None else None)
        tail = (m.data_ptr() if m is not None else None, s.data_ptr() if s is not None else None, B, C, Tn, H, W,
                float(scale), float(lo), float(hi)) + ((LOG_GAIN, LOG_FLOOR) if log_transform else ()) + (_stream(),)
        entry = "cn_augment_{}_log_f32" if log_transform else "cn_augment_{}_f32"
        parcel_h = parcel_d = None
        has_parcel = plan.has_parcel
        if has_parcel:
            parcel_h = torch.from_numpy(np.ascontiguousarray(plan.parcel)).pin_memory()
            parcel_d = parcel_h.to(dev, non_blocking=True)
        rows = plan.series_rows() if plan.series else ()
        if rows:  # four launches: label, x planes, x series, targets
            # the tables of the series samples only, and their sample indices behind them: one pinned array, one copy
            # written straight into the pinned array
            size = len(rows) * SERIES_SLOTS * (Tn + C * Tn + 1)
            series_h = torch.empty(size + len(rows), dtype=torch.float32, pin_memory=True)
            packed = series_h.numpy()
            plan._pack_series(C, Tn, rows, packed[:size].reshape(len(rows), -1))
            packed[size:].view(np.int32)[:] = rows
            series_d = series_h.to(dev, non_blocking=True)
            labels, _ = label_parcels(y, self.crop_value)
            _lib.call(entry.format("series"), *head, labels.data_ptr(),
                      parcel_h.data_ptr() if parcel_h is not None else None,
                      parcel_d.data_ptr() if parcel_d is not None else None, series_h.data_ptr(), series_d.data_ptr(),
                      series_h.data_ptr() + 4 * size, series_d.data_ptr() + 4 * size, len(rows), *tail)
        elif has_parcel:  # three launches: label, x, targets
            labels, _ = label_parcels(y, self.crop_value)
            _lib.call(entry.format("parcels"), *head, labels.data_ptr(), parcel_h.data_ptr(), parcel_d.data_ptr(), *tail)
        else:
            _lib.call(entry.format("chips"), *head, *tail)
        kw["x"], kw["y"] = x_out, y_out
        if bd is not None:
            kw["bdist"] = bd_out
        return Data(**kw)


def label_parcels(y: torch.Tensor, crop_value: int = 1) -> T.Tuple[torch.Tensor, torch.Tensor]:
    """The 4-connected components of ``y == crop_value``, per sample, on the current stream: ``y`` [B, H, W] device labels
    -> (labels int32 [B, H, W], counts int32 [B]). Background is 0 and the parcels are numbered 1..counts[b] in raster
    order of their first pixel, as ``scipy.ndimage.label(y[b] == crop_value)`` numbers them (data/datasets.py:463-465,
    before its ``np.uint8``)."""
    if not y.is_cuda:
        raise RuntimeError("label_parcels needs a device tensor")
    if y.dtype not in _Y_DTYPES:
        raise TypeError(f"unsupported label dtype {y.dtype}")
    if y.dim() != 3:
        raise ValueError("y must be [B, H, W]")
    y = y.contiguous()
    B, H, W = y.shape
    labels = torch.empty((B, H, W), dtype=torch.int32, device=y.device)
    counts = torch.empty((B,), dtype=torch.int32, device=y.device)
    if y.numel():
        _lib.call("cn_label_parcels_i32", y.data_ptr(), _Y_DTYPES[y.dtype], int(crop_value), labels.data_ptr(),
                  counts.data_ptr(), B, H, W, _stream())
    return labels, counts
