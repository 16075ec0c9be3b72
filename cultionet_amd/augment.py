"""Device-side training augmentation for raw batches (the fused prologues ``cn_augment_chips_f32`` and
``cn_augment_parcels_f32``, and the parcel labelling ``cn_label_parcels_i32``).

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
the connected components of the crop pixels of ``y``, which ``label_parcels`` computes on the device. Of the five, ``roll``
(augment/augmenters.py:154-163) is covered, as an opt-in (``DeviceAugmenter(parcel_augmentations=("roll",))``): one shift
per parcel is drawn on the host into ``AugmentPlan.parcel``. The four ``ts*`` augmenters are ``tsaug`` transforms and stay
on the host path (float batches prepared per sample).
"""
from __future__ import annotations

import typing as T

import numpy as np
import torch

from . import _lib
from .data import Data
from .edges import _DTYPES, SCALE_FACTOR, prepare_chips
from .engine import _stream

OPS = ("none", "rot90", "rot180", "rot270", "fliplr", "flipud", "gaussian", "saltpepper", "cropresize", "perlin")
OP_CODES = {name: code for code, name in enumerate(OPS)}
DEVICE_AUGMENTATIONS = OPS[1:]
HOST_AUGMENTATIONS = ("tswarp", "tsnoise", "tsdrift", "tspeaks", "roll")  # what ``augmentations=`` refuses
PARCEL_AUGMENTATIONS = ("roll",)  # opt-in through ``parcel_augmentations=``: they label the parcels of y first
PARCEL_OP_CODES = {name: len(OPS) + k for k, name in enumerate(PARCEL_AUGMENTATIONS)}
_TSAUG = ("tswarp", "tsnoise", "tsdrift", "tspeaks")

PLAN_WORDS = 8  # op, div, top, left, r, sigma (float bits), seed low word, seed high word
PERLIN_RES = (2, 5, 10)
PERLIN_RMAX = 10
PERLIN_FLOATS = 4 * (PERLIN_RMAX + 1) ** 2  # theta [2][r+1][r+1] then phi [2][r+1][r+1], compact, per sample
PARCEL_SHIFTS = 256  # shifts per sample, indexed by label & 255: the reference holds its segments as uint8
_Y_DTYPES = {torch.int32: 1, torch.int16: 2, torch.uint16: 3, torch.int64: 4}


class AugmentPlan:
    """What one batch's augmentation does, as host arrays: ``table`` int32 [B, PLAN_WORDS] and ``perlin`` float32
    [B, PERLIN_FLOATS] (angles; rows of samples that are not ``perlin`` stay zero), and ``parcel`` int32
    [B, PARCEL_SHIFTS] (the shift of parcel k at [k & 255]; rows of samples that are not ``roll`` stay zero). A fresh plan
    is all ``none``."""

    def __init__(self, B: int):
        self.table = np.zeros((B, PLAN_WORDS), dtype=np.int32)
        self.perlin = np.zeros((B, PERLIN_FLOATS), dtype=np.float32)
        self.parcel = np.zeros((B, PARCEL_SHIFTS), dtype=np.int32)
        self._parcel_rows = np.zeros(B, dtype=bool)  # rows that set() gave a parcel op and its shifts

    def __len__(self) -> int:
        return self.table.shape[0]

    def set(self, b: int, op: str, *, sigma: float = 0.0, div: int = 0, top: int = 0, left: int = 0, r: int = 0,
            theta: T.Optional[np.ndarray] = None, phi: T.Optional[np.ndarray] = None, seed: int = 0,
            shifts: T.Optional[np.ndarray] = None) -> "AugmentPlan":
        """Sample ``b`` gets ``op``. gaussian: sigma; cropresize: div, top, left; saltpepper: seed (64 bit);
        perlin: r and the angle tables theta, phi [2, r+1, r+1]; roll: shifts, 256 integers with shifts[0] == 0
        (parcel k rolls by shifts[k & 255]; their range against T is checked when the plan is applied)."""
        row = self.table[b]
        row[:] = 0
        self.perlin[b] = 0.0
        self.parcel[b] = 0
        self._parcel_rows[b] = False
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
        return (OPS + PARCEL_AUGMENTATIONS)[int(self.table[b, 0])]

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


class DeviceAugmenter:
    """``DeviceAugmenter(augment_prob=0.5, augmentations=DEVICE_AUGMENTATIONS, seed=42, parcel_augmentations=())``: draws
    one plan per batch and applies it on the device. Hand it to ``DeviceFeeder(augmenter=...)`` or
    ``CultionetLitModel.set_augmenter``. ``parcel_augmentations`` (names of PARCEL_AUGMENTATIONS) join the candidates of
    the draw; a batch in which one of them is drawn is labelled on the device first (``label_parcels``).
    ``crop_value`` is the class of ``y`` whose connected components are the parcels."""

    def __init__(self, augment_prob: float = 0.5, augmentations: T.Sequence[str] = DEVICE_AUGMENTATIONS, seed: int = 42,
                 parcel_augmentations: T.Sequence[str] = (), crop_value: int = 1):
        for name in augmentations:
            if name in HOST_AUGMENTATIONS:
                raise NotImplementedError(
                    f"{name!r} warps each labelled parcel on the host (connected components of y, tsaug): it has no "
                    "device counterpart; augment those samples per sample on the host and feed float batches")
            if name not in OP_CODES:
                raise KeyError(name)  # as AUGMENTER_METHODS[name] (augment/augmenters.py:341-357, 423)
        for name in parcel_augmentations:
            if name in _TSAUG:
                raise NotImplementedError(
                    f"{name!r} is a tsaug transform (TimeWarp / Drift / AddNoise) applied per parcel: it has no device "
                    "counterpart yet; augment those samples per sample on the host and feed float batches")
            if name not in PARCEL_OP_CODES:
                raise KeyError(name)
        if not 0.0 <= augment_prob <= 1.0:
            raise ValueError("augment_prob must lie in [0, 1]")
        self.augment_prob = float(augment_prob)
        self.augmentations = tuple(augmentations)
        self.parcel_augmentations = tuple(parcel_augmentations)
        self.crop_value = int(crop_value)
        self.rng = np.random.default_rng(seed)

    def _candidates(self, H: int, W: int) -> T.Tuple[T.List[str], T.List[int]]:
        if H != W and ("rot90" in self.augmentations or "rot270" in self.augmentations):
            raise ValueError(f"rot90 / rot270 need square chips, got {H} x {W}: drop them from the augmentations")
        res = [r for r in PERLIN_RES if H % r == 0 and W % r == 0]
        names = [n for n in self.augmentations if n != "none" and (n != "perlin" or res)]
        if "cropresize" in names and (H < 2 or W < 2):
            names.remove("cropresize")
        if "gaussian" in names and (H < 2 or W < 2):
            names.remove("gaussian")
        return names + list(self.parcel_augmentations), res

    def draw(self, B: int, T_: int, H: int, W: int) -> AugmentPlan:
        """The plan of one batch of B samples [C, T_, H, W]: B sequential per-sample draws from the augmenter's
        generator (augment or not as datasets.py:449, the op as datasets.py:451, then the op's own parameters)."""
        names, res = self._candidates(H, W)
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
            else:
                plan.set(b, name)
        return plan

    def apply(self, batch: Data, mean: T.Optional[torch.Tensor] = None, std: T.Optional[torch.Tensor] = None,
              plan: T.Optional[AugmentPlan] = None, scale: float = 1.0 / SCALE_FACTOR, lo: float = 1e-9,
              hi: float = 1.0) -> Data:
        """Raw device batch -> prepared Data (x fp32 z-scored, bdist fp32, y int64) with ``plan`` (default: a fresh
        ``draw``) applied, on the current stream. A batch without labels passes through the plain prologue: the
        reference only augments labelled samples (datasets.py:448)."""
        x = batch.x
        if not x.is_cuda:
            raise RuntimeError("DeviceAugmenter.apply needs a device batch")
        if x.dtype not in _DTYPES:
            raise TypeError(f"unsupported raw dtype {x.dtype}")
        kw = dict(batch.__dict__)
        bd = kw.get("bdist")
        y = kw.get("y")
        if y is None:
            kw["x"] = prepare_chips(x, mean, std, scale, lo, hi)
            if bd is not None and bd.dtype != torch.float32:
                kw["bdist"] = prepare_chips(bd.reshape(bd.shape[0], 1, 1, *bd.shape[1:]), None, None, scale, lo,
                                            hi).reshape(bd.shape)
            return Data(**kw)
        B, C, Tn, H, W = x.shape
        if plan is None:
            plan = self.draw(B, Tn, H, W)
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
                float(scale), float(lo), float(hi), _stream())
        if plan.has_parcel:  # three launches: label, x, targets
            parcel_h = torch.from_numpy(np.ascontiguousarray(plan.parcel)).pin_memory()
            parcel_d = parcel_h.to(dev, non_blocking=True)
            labels, _ = label_parcels(y, self.crop_value)
            _lib.call("cn_augment_parcels_f32", *head, labels.data_ptr(), parcel_h.data_ptr(), parcel_d.data_ptr(), *tail)
        else:
            _lib.call("cn_augment_chips_f32", *head, *tail)
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
