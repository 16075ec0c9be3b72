#!/usr/bin/env python
"""Time the device augmentation stage against the plain prologue on one raw batch (default [8, 3, 12, 100, 100] int16,
bdist int16, y int64: the flagship training batch as the feeder stages it).

    python tools/augment_time.py [--out FILE] [--iters 200] [--repeats 7]

Variants, alternated inside every repeat so that they see the same machine state:
  plain        what the feeder does without an augmenter: cn_prepare_chips_f32 on x, again on bdist (y is int64 already)
  none         DeviceAugmenter.apply with an all-`none` plan
  mixed        apply with plans drawn by the default augmenter (augment_prob 0.5, nine ops), a fresh plan every call
  <op>         apply with every sample of the batch given that op
Each figure is the time between two HIP events around `iters` back-to-back calls on one stream, divided by `iters`
(device events, work ends in a synchronise; warmed by one untimed round): it includes the allocation of the outputs, the
plan's host-to-device copy and any host time the device waits for. `host_us` is the host clock over the same window.
One JSON line per variant: median, min and max over the repeats, in microseconds per call."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cultionet_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 3, 12, 100, 100])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cultionet_amd.configure_runtime()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py measures on the GPU; there is none here")
    from cultionet_amd.augment import DEVICE_AUGMENTATIONS, AugmentPlan, DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import prepare_chips

    B, C, T, H, W = args.shape
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 10000, (B, C, T, H, W), generator=g).to(torch.int16).cuda()
    bd = torch.randint(0, 10001, (B, H, W), generator=g).to(torch.int16).cuda()
    y = torch.randint(-1, 3, (B, H, W), generator=g).cuda()
    mean, std = torch.rand(C, generator=g).cuda() * 0.3, torch.rand(C, generator=g).cuda() * 0.2 + 0.05
    batch = Data(x=x, y=y, bdist=bd)
    aug = DeviceAugmenter()
    rng = np.random.default_rng(0)

    def plan_of(op):
        plan = AugmentPlan(B)
        res = [r for r in (2, 5, 10) if H % r == 0 and W % r == 0]
        for b in range(B):
            if op == "gaussian":
                plan.set(b, op, sigma=float(rng.uniform(0.2, 0.5)))
            elif op == "saltpepper":
                plan.set(b, op, seed=int(rng.integers(0, 2 ** 63)))
            elif op == "cropresize":
                div = (2, 4)[b % 2]
                plan.set(b, op, div=div, top=int(rng.integers(0, H - H // div + 1)), left=int(rng.integers(0, W - W // div + 1)))
            elif op == "perlin":
                r = res[b % len(res)]
                a = (2 * np.pi * rng.random((2, 2, r + 1, r + 1))).astype(np.float32)
                plan.set(b, op, r=r, theta=a[0], phi=a[1])
            else:
                plan.set(b, op)
        return plan

    def plain():
        prepare_chips(x, mean, std)
        prepare_chips(bd.reshape(B, 1, 1, H, W))

    variants = {"plain": plain, "none": lambda p=AugmentPlan(B): aug.apply(batch, mean, std, plan=p),
                "mixed": lambda: aug.apply(batch, mean, std)}
    for op in DEVICE_AUGMENTATIONS:
        if op in ("rot90", "rot270") and H != W:
            continue
        if op == "perlin" and not [r for r in (2, 5, 10) if H % r == 0 and W % r == 0]:
            continue
        variants[op] = lambda p=plan_of(op): aug.apply(batch, mean, std, plan=p)

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
        lines.append(json.dumps({"variant": k, "shape": args.shape, "iters": args.iters, "repeats": args.repeats,
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
