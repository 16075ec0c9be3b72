#!/usr/bin/env python
"""Time the parcel side of the device augmentation stage on raw int16 batches (default [8, 3, 12, 100, 100] and
[32, 3, 12, 100, 100], bdist int16, y int64).

    python tools/parcel_time.py [--out FILE] [--iters 200] [--repeats 7] [--batches 8 32] [--labels random blocks]
                                 [--variants fliplr roll label tswarp tsdrift tspeaks tsnoise]

Variants, alternated inside every repeat so that they see the same machine state:
  fliplr       DeviceAugmenter.apply with every sample `fliplr` (two launches; the figure the parent commit has too)
  roll         apply with every sample `roll` (three launches: label, x, targets)
  label        label_parcels alone (one launch and its two output allocations)
  tswarp, tsdrift, tspeaks, tsnoise
               apply with every sample that series op, its curves drawn once beforehand as DeviceAugmenter.draw draws them
               (four launches: label, x planes, x series, targets; the call packs and copies the tables of all B samples)
  draw_tswarp, draw_tsdrift
               DeviceAugmenter.draw alone for a batch of that op: host time only, nothing runs on the device
for two kinds of label plane: `random` (each pixel crop with probability 0.5: many small parcels) and `blocks` (rectangular
fields 8 to 24 pixels on a side between one-pixel edges: few large parcels, as training chips have them).
Each figure is the time between two HIP events around `iters` back-to-back calls on one stream, divided by `iters`,
warmed by untimed calls; one JSON line per variant with median, min and max over the repeats, in microseconds per call."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cultionet_amd  # noqa: E402


def blocks(B, H, W, rng):
    """Rows of rectangular fields (crop, 1) separated by one-pixel edges (2)."""
    y = np.full((B, H, W), 2, dtype=np.int64)
    for b in range(B):
        h = 0
        while h < H:
            dh = int(rng.integers(8, 25))
            w = 0
            while w < W:
                dw = int(rng.integers(8, 25))
                y[b, h:min(h + dh, H), w:min(w + dw, W)] = int(rng.random() < 0.8)  # some fields are background
                w += dw + 1
            h += dh + 1
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--labels", nargs="+", default=["random", "blocks"], choices=["random", "blocks"])
    series = ["tswarp", "tsdrift", "tspeaks", "tsnoise"]
    ap.add_argument("--variants", nargs="+", default=["fliplr", "roll", "label", "tswarp", "tsdrift", "tspeaks"],
                    choices=["fliplr", "roll", "label", "draw_tswarp", "draw_tsdrift"] + series)
    ap.add_argument("--chip", type=int, nargs=4, default=[3, 12, 100, 100], help="C T H W")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cultionet_amd.configure_runtime()
    if not torch.cuda.is_available():
        raise SystemExit("parcel_time.py measures on the GPU; there is none here")
    from cultionet_amd.augment import AugmentPlan, DeviceAugmenter, label_parcels
    from cultionet_amd.data import Data

    C, T, H, W = args.chip
    aug = DeviceAugmenter()
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(1)
    variants = {}
    parcels = {}
    for B in args.batches:
        x = torch.randint(0, 10000, (B, C, T, H, W), generator=g).to(torch.int16).cuda()
        bd = torch.randint(0, 10001, (B, H, W), generator=g).to(torch.int16).cuda()
        mean, std = torch.rand(C, generator=g).cuda() * 0.3, torch.rand(C, generator=g).cuda() * 0.2 + 0.05
        flip, roll = AugmentPlan(B), AugmentPlan(B)
        q = int(T * 0.25)
        for b in range(B):
            flip.set(b, "fliplr")
            shifts = np.zeros(256, dtype=np.int32)
            shifts[1:] = rng.integers(-q, q + 1, 255)
            roll.set(b, "roll", shifts=shifts)
        drawers = {v: DeviceAugmenter(augment_prob=1.0, augmentations=(), series_augmentations=(v,), seed=2) for v in series}
        plans = {v: drawers[v].draw(B, T, H, W, C) for v in series if v in args.variants}
        for kind in args.labels:
            y = blocks(B, H, W, rng) if kind == "blocks" else (rng.random((B, H, W)) < 0.5).astype(np.int64)
            yd = torch.from_numpy(y).cuda()
            batch = Data(x=x, y=yd, bdist=bd)
            parcels[f"{kind}/{B}"] = float(label_parcels(yd)[1].float().mean())
            fns = {"fliplr": lambda batch=batch, m=mean, s=std, p=flip: aug.apply(batch, m, s, plan=p),
                   "roll": lambda batch=batch, m=mean, s=std, p=roll: aug.apply(batch, m, s, plan=p),
                   "label": lambda yd=yd: label_parcels(yd)}
            fns.update({v: lambda batch=batch, m=mean, s=std, p=p: aug.apply(batch, m, s, plan=p) for v, p in plans.items()})
            fns.update({f"draw_{v}": lambda d=drawers[v], B=B: d.draw(B, T, H, W, C) for v in ("tswarp", "tsdrift")})
            variants.update({f"{v}/{kind}/{B}": fns[v] for v in args.variants})

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters, (time.perf_counter() - t0) * 1e6 / args.iters

    for fn in variants.values():  # warm every variant: code objects, allocator pools
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    dev = {k: [] for k in variants}
    host = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            d, h = window(fn)
            dev[k].append(d)
            host[k].append(h)
    lines = []
    for k in variants:
        op, kind, B = k.split("/")
        lines.append(json.dumps({"variant": op, "labels": kind, "shape": [int(B), C, T, H, W], "iters": args.iters,
                                 "repeats": args.repeats, "parcels_per_sample": round(parcels[f"{kind}/{B}"], 1),
                                 "device_us": {"median": round(float(np.median(dev[k])), 2), "min": round(min(dev[k]), 2),
                                               "max": round(max(dev[k]), 2)},
                                 "host_us": {"median": round(float(np.median(host[k])), 2)}}))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
