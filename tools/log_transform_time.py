#!/usr/bin/env python
"""Time the log-transform prologues against the plain ones (the pattern of tools/augment_time.py).

    python tools/log_transform_time.py [--out FILE] [--iters 200] [--repeats 7] [--hidden 32] [--scenes 10]

Prologue, on one raw batch (default int16 [8, 3, 12, 100, 100], the flagship training batch as the feeder stages it),
variants alternated inside every repeat so that they see the same machine state:
  prepare / prepare_log     prepare_chips(x, mean, std) without and with log_transform=True
  augment / augment_log     DeviceAugmenter.apply with an all-`none` plan, without and with it
  window / window_log       cn_window_chips(_log)_f32 alone on the 36 windows of the `predict` block's scene
Each figure is the time between two HIP events around `iters` back-to-back calls on one stream, divided by `iters`; it
includes the allocation of the output. One JSON line per variant: median, min and max over the repeats, microseconds.

Predict: Mpixel/s of SlidingWindowPredictor on the scene of bench.py's `predict` block (int16 [4, 25, 600, 600], window
100 + 2 x 5, all 36 windows in one batch), fp32 and bf16-mixed, without and with log_transform=True; host clock over
`scenes` scenes after four warm-up scenes, as bench.py times it."""
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
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--scenes", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cultionet_amd.configure_runtime()
    if not torch.cuda.is_available():
        raise SystemExit("log_transform_time.py measures on the GPU; there is none here")
    from cultionet_amd import _lib
    from cultionet_amd import synthetic as S
    from cultionet_amd.augment import AugmentPlan, DeviceAugmenter
    from cultionet_amd.data import Data
    from cultionet_amd.edges import LOG_FLOOR, LOG_GAIN, prepare_chips
    from cultionet_amd.engine import _stream
    from cultionet_amd.lightning import CultionetLitModel
    from cultionet_amd.predict import SlidingWindowPredictor, window_origins

    B, C, T, H, W = args.shape
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 10000, (B, C, T, H, W), generator=g).to(torch.int16).cuda()
    bd = torch.randint(0, 10001, (B, H, W), generator=g).to(torch.int16).cuda()
    y = torch.randint(-1, 3, (B, H, W), generator=g).cuda()
    mean, std = torch.rand(C, generator=g).cuda() * 0.3, torch.rand(C, generator=g).cuda() * 0.2 + 0.05
    batch = Data(x=x, y=y, bdist=bd)
    aug, plan = DeviceAugmenter(), AugmentPlan(B)

    HS, ws, pad = 600, 100, 5
    SC, ST, SS = 4, 25, ws + 2 * pad
    scene = (torch.rand(SC, ST, HS, HS, generator=torch.Generator().manual_seed(11)) * 10000.0).to(torch.int16).cuda()
    rc = torch.tensor(window_origins(HS, HS, ws), dtype=torch.int32).cuda()
    smean, sstd = torch.rand(SC, generator=g).cuda() * 0.3, torch.rand(SC, generator=g).cuda() * 0.2 + 0.05
    wout = torch.empty((rc.shape[0], SC, ST, SS, SS), device="cuda")

    def window(log):
        a = (scene.data_ptr(), 2, wout.data_ptr(), rc.data_ptr(), rc.shape[0], SC, ST, HS, HS, SS, pad, smean.data_ptr(),
             sstd.data_ptr(), 1e-4, 1e-9, 1.0)
        if log:
            _lib.call("cn_window_chips_log_f32", *a, LOG_GAIN, LOG_FLOOR, _stream())
        else:
            _lib.call("cn_window_chips_f32", *a, _stream())

    variants = {"prepare": lambda: prepare_chips(x, mean, std),
                "prepare_log": lambda: prepare_chips(x, mean, std, log_transform=True),
                "augment": lambda: aug.apply(batch, mean, std, plan=plan),
                "augment_log": lambda: aug.apply(batch, mean, std, plan=plan, log_transform=True),
                "window": lambda: window(False), "window_log": lambda: window(True)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    for fn in variants.values():  # warm every variant: code objects, allocator pools
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    dev = {k: [] for k in variants}
    for _ in range(args.repeats):
        for k, fn in variants.items():
            dev[k].append(timed(fn))
    lines = []
    for k in variants:
        elems = wout.numel() if k.startswith("window") else x.numel()
        lines.append(json.dumps({"variant": k, "elements": elems, "iters": args.iters, "repeats": args.repeats,
                                 "device_us": {"median": round(float(np.median(dev[k])), 2), "min": round(min(dev[k]), 2),
                                               "max": round(max(dev[k]), 2)}}))

    lit = CultionetLitModel(in_channels=SC, in_time=ST, hidden_channels=args.hidden, dropout=0.0)
    model = lit.cultionet_model.mask_model
    model.load_state_dict(S.seeded_state_dict(model.state_dict()))
    lit = lit.to("cuda").eval()
    for prec in ("32-true", "bf16-mixed"):
        rates = {}
        for rep in range(3):  # the two settings alternated
            for log in (False, True):
                sp = SlidingWindowPredictor(lit, window_size=ws, padding=pad, batch_size=36, precision=prec,
                                            pixels_per_launch=0, mean=smean, std=sstd, log_transform=log)
                for _ in range(4):
                    sp.predict_scene(scene)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.scenes):
                    sp.predict_scene(scene)
                torch.cuda.synchronize()
                rates.setdefault(log, []).append(HS * HS * args.scenes / (time.perf_counter() - t0) / 1e6)
        for log in (False, True):
            lines.append(json.dumps({"variant": f"predict_{prec}" + ("_log" if log else ""), "hidden": args.hidden,
                                     "scenes": args.scenes,
                                     "mpixel_per_s": {"median": round(float(np.median(rates[log])), 2),
                                                      "min": round(min(rates[log]), 2), "max": round(max(rates[log]), 2)}}))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
