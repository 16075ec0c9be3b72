#!/usr/bin/env python
"""Writes tests/golden/augment_series.npz: what the reference's own augment_time (cultionet/augment/augmenter_utils.py:
111-165, through SegmentParcel and insert_parcel, :57-108) makes of two small samples for each of aug = tswarp, tsnoise,
tsdrift, tspeaks, called once per prop in label order as AugmentTimeMixin.forward does (augment/augmenters.py:51-63),
followed by the x.clip(1e-9, 1) of AugmenterModule.__call__ (:25-35).

    python tools/make_series_golden.py /path/to/reference/src

The reference module is executed from where it lies, with the stand-in modules of tools/make_augment_golden.py and the
Prop / Sample stand-ins and label planes of tools/make_parcel_golden.py. `tsaug` is not installed (the reference pins a
fork of it), and augment_time takes its warper as an argument, so the warpers are stand-ins written here, with tsaug's
`augment(X)` interface on X [(h w), T, C]:
  PosWarper     np.interp(pos, arange(T), series) per pixel and channel, pos the table row of the current prop
  DriftWarper   series + drift * (max - min), drift [C, T] the table row of the current prop
  Nothing       X unchanged
and the module's `AddNoise` name is replaced by a stand-in that adds n * scale * (max - min), n the counter-based normal of
the device op at the element's index in the sample (tests/augment_ref.py::normal_noise); for that it is told the box of
the current prop. Its `scale` is the one augment_time draws itself (np.random.uniform(0.01, 0.05), seeded here) and is
recorded as the prop's nscale; for tsnoise, where AddNoise is the warper, one scale serves every prop.

What the fixture pins to the reference's program text: the layout `(h w) t c`, the two halves of tspeaks, the order warp
then noise, the clip(0, 1) and the insertion rule. It does not pin how tsaug draws its curves.

The sample's x is handed over as float64 (the float32 values of (x_raw / 10000).clip(1e-9, 1), widened): the reference
then computes every step in float64 and its result is rounded to float32 once, by AugmenterModule.__call__. Fed float32,
F.interpolate alone would compute the halves of tspeaks in float32, and the recorded output would carry those roundings
(the float64 restatement of tests/ts_ref.py then meets tspeaks within 5.9e-8 instead of 3.0e-8; the other three ops do
not change).

Cases (arrays `<case>_x_raw` int16 [1, C, T, H, W], `_x` float32, `_y` int64 [H, W], `_labels` int32 (scipy's, unwrapped),
`_pos` float32 [256, T], `_drift` float32 [256, C, T], indexed by the uint8 segment value; per aug `_<aug>_nscale` float32
[256], `_<aug>_seed` int64, `_<aug>_out` float32 [1, C, T, H, W]):
  small    12 x 12, C 2, T 12: five parcels, one L-shaped whose bbox covers another parcel
  lattice  34 x 34, C 1, T 12: 289 parcels, so that the uint8 wrap folds 256.. onto 0, 1, ...
"""
import os
import sys

import numpy as np
import torch
from einops import rearrange
from scipy.ndimage import label as nd_label

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from augment_ref import normal_noise  # noqa: E402
from make_augment_golden import load_reference  # noqa: E402
from make_parcel_golden import Prop, Sample, lattice_y, small_y  # noqa: E402

AUGS = ("tswarp", "tsnoise", "tsdrift", "tspeaks")
STATE = {}  # the current prop, the sample's shape and noise seed, the nscale table being recorded


class PosWarper:
    def __init__(self, pos):
        self.pos = pos

    def augment(self, X):
        N, T, C = X.shape
        out = np.empty((N, T, C), dtype=np.float64)
        for i in range(N):
            for c in range(C):
                out[i, :, c] = np.interp(self.pos[STATE["prop"].label], np.arange(T), X[i, :, c])
        return out


class DriftWarper:
    def __init__(self, drift):
        self.drift = drift

    def augment(self, X):
        rng = X.max(axis=1, keepdims=True) - X.min(axis=1, keepdims=True)
        return X + self.drift[STATE["prop"].label].T.astype(np.float64)[None] * rng   # [C, T] -> [1, T, C]


class Nothing:
    def augment(self, X):
        return X


class CounterNoise:
    """Stands in for tsaug.AddNoise(scale): X + n * scale * (max - min) per series and channel."""

    def __init__(self, scale):
        self.scale = float(np.float32(scale))  # as the plan's float32 table holds it

    def augment(self, X):
        C, T, H, W = STATE["shape"]
        r0, c0, r1, c1 = STATE["prop"].bbox
        n = normal_noise(STATE["seed"], C * T * H * W).reshape(C, T, H, W)[:, :, r0:r1, c0:c1]
        n = rearrange(n, "c t h w -> (h w) t c")
        STATE["nscale"][STATE["prop"].label] = self.scale
        return X + n * self.scale * (X.max(axis=1, keepdims=True) - X.min(axis=1, keepdims=True))


def tables(C, T, seed):
    """One table of source times and one of drifts per case, any monotone / bounded curves: they are inputs here."""
    g = np.random.default_rng(seed)
    pos = np.tile(np.arange(T, dtype=np.float32), (256, 1))
    p = np.cumsum(g.random((256, T)) + 0.05, axis=1)
    p = (p - p[:, :1]) / (p[:, -1:] - p[:, :1]) * (T - 1)
    p[::4] = np.round(p[::4])
    pos[1:] = np.clip(p[1:], 0, T - 1)
    drift = np.zeros((256, C, T), dtype=np.float32)
    drift[1:] = g.uniform(-0.1, 0.1, (255, C, T))
    return pos, drift


def run(ref, name, y, C, T, seed, out):
    H, W = y.shape
    g = np.random.default_rng(seed)
    x_raw = g.integers(-20, 11000, (1, C, T, H, W)).astype(np.int16)  # below 0 and above 10000: both clips matter
    x = (torch.from_numpy(x_raw) / 10000.0).clip(1e-9, 1)              # data/datasets.py:443
    labels = nd_label(y == 1)[0]
    segments = np.uint8(labels)
    props = [Prop(segments, v) for v in np.unique(segments) if v != 0]
    pos, drift = tables(C, T, seed + 1)
    out.update({f"{name}_x_raw": x_raw, f"{name}_x": x.numpy(), f"{name}_y": y, f"{name}_labels": labels.astype(np.int32),
                f"{name}_pos": pos, f"{name}_drift": drift})
    for a, aug in enumerate(AUGS):
        np.random.seed(seed + 10 + a)  # augment_time draws its noise scale from the global generator
        STATE.update(shape=(C, T, H, W), seed=int(g.integers(0, 2 ** 63)), nscale=np.zeros(256, dtype=np.float32))
        warper = {"tswarp": PosWarper(pos), "tspeaks": PosWarper(pos), "tsdrift": DriftWarper(drift),
                  "tsnoise": CounterNoise(np.random.uniform(0.01, 0.05))}[aug]
        sample = Sample(x.double().clone(), segments)
        for p in props:
            STATE["prop"] = p
            sample = ref.augment_time(sample, p, add_noise=aug != "tsnoise", warper=warper, aug=aug)
        result = sample.x.float().clip(1e-9, 1)
        nscale = STATE["nscale"]
        assert result.dtype == torch.float32 and (nscale[[p.label for p in props]] > 0).all() and nscale[0] == 0
        out.update({f"{name}_{aug}_nscale": nscale.copy(), f"{name}_{aug}_seed": np.int64(STATE["seed"]),
                    f"{name}_{aug}_out": result.numpy()})
        changed = float((result != x).float().mean())
        print(name, aug, "props", len(props), "changed", round(changed, 3), "nscale", sorted(set(nscale.tolist()))[:3])


def main():
    ref = load_reference(sys.argv[1])
    ref.AddNoise = CounterNoise
    out = {}
    run(ref, "small", small_y(), 2, 12, 31, out)
    run(ref, "lattice", lattice_y(), 1, 12, 32, out)
    dst = os.path.join(ROOT, "tests", "golden", "augment_series.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
