#!/usr/bin/env python
"""Writes tests/golden/augment_roll.npz: what the reference's own roll_time (cultionet/augment/augmenter_utils.py:168-193,
through insert_parcel, :88-108) makes of two small samples, called once per prop in label order as Roll.forward does
(augment/augmenters.py:154-163), followed by the x.clip(1e-9, 1) of AugmenterModule.__call__ (:25-35).

    python tools/make_parcel_golden.py /path/to/reference/src

The reference module is executed from where it lies, with the stand-in modules of tools/make_augment_golden.py
(augmenters.py itself pulls in torchvision and is not imported). skimage is not needed: the props are stand-ins with
`.label` and `.bbox`, computed from np.uint8(scipy.ndimage.label(y == 1)[0]) as EdgeDataset.get computes its segments
(data/datasets.py:463-466) -- one prop per distinct non-zero value, its bbox the union over that value's pixels, which is
what regionprops returns. The shift drawn for each prop is recorded by wrapping rng.choice.

Cases (arrays `<case>_x_raw` int16 [1, C, T, H, W], `_x` float32 = (x_raw / 10000).clip(1e-9, 1) as the reference is fed,
`_y` int64 [H, W], `_labels` int32 (scipy's, unwrapped), `_segments` uint8, `_prop_labels` and `_prop_shifts` int64 [props],
`_out` float32 [1, C, T, H, W]):
  small    12 x 12, C 2, T 12: five parcels, one L-shaped whose bbox covers another parcel, two that touch diagonally
  lattice  34 x 34, C 1, T 12: y[::2, ::2] = 1, 289 parcels, so that the uint8 wrap folds 256.. onto 0, 1, ...
"""
import os
import sys

import numpy as np
import torch
from scipy.ndimage import label as nd_label

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_augment_golden import load_reference  # noqa: E402


class Prop:
    def __init__(self, segments, value):
        rows, cols = np.nonzero(segments == value)
        self.label = int(value)
        self.bbox = (int(rows.min()), int(cols.min()), int(rows.max()) + 1, int(cols.max()) + 1)


class Sample:
    """The attributes of cultionet.data.Data that roll_time and insert_parcel touch."""

    def __init__(self, x, segments):
        self.x, self.segments = x, segments
        self.num_time = x.shape[2]


class RecordingRng:
    def __init__(self, seed):
        self.rng, self.drawn = np.random.default_rng(seed), []

    def choice(self, a):
        self.drawn.append(int(self.rng.choice(a)))
        return self.drawn[-1]


def small_y():
    y = np.zeros((12, 12), dtype=np.int64)
    y[1:7, 1] = 1
    y[6, 1:6] = 1          # an L: bbox rows 1-6, cols 1-5
    y[2:4, 3:5] = 1        # a block inside that bbox, not touching the L
    y[0, 11] = 1
    y[1, 10] = 1           # touches (0, 11) diagonally only
    y[8:11, 7:11] = 1
    y[7, 7:11] = 2         # edge class
    y[11, 0:3] = -1        # unlabelled
    return y


def lattice_y():
    y = np.zeros((34, 34), dtype=np.int64)
    y[::2, ::2] = 1
    return y


def run(ref, name, y, C, T, seed, out):
    H, W = y.shape
    g = np.random.default_rng(seed)
    x_raw = g.integers(-20, 11000, (1, C, T, H, W)).astype(np.int16)  # below 0 and above 10000: both clips matter
    x = (torch.from_numpy(x_raw) / 10000.0).clip(1e-9, 1)              # data/datasets.py:443
    labels = nd_label(y == 1)[0]
    segments = np.uint8(labels)
    props = [Prop(segments, v) for v in np.unique(segments) if v != 0]
    sample, rng = Sample(x.clone(), segments), RecordingRng(seed + 1)
    for p in props:
        sample = ref.roll_time(sample, p, rng=rng)
    result = sample.x.float().clip(1e-9, 1)
    assert len(rng.drawn) == len(props) and result.dtype == torch.float32
    out.update({f"{name}_x_raw": x_raw, f"{name}_x": x.numpy(), f"{name}_y": y, f"{name}_labels": labels.astype(np.int32),
                f"{name}_segments": segments, f"{name}_prop_labels": np.array([p.label for p in props]),
                f"{name}_prop_shifts": np.array(rng.drawn), f"{name}_out": result.numpy()})
    print(name, "parcels", int(labels.max()), "props", len(props), "shifts", sorted(set(rng.drawn)))


def main():
    ref = load_reference(sys.argv[1])
    out = {}
    run(ref, "small", small_y(), 2, 12, 21, out)
    run(ref, "lattice", lattice_y(), 1, 12, 22, out)
    dst = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "augment_roll.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
