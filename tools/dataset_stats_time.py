#!/usr/bin/env python
"""Time the dataset-statistics pass on one raw int16 batch (default [8, 3, 12, 100, 100], y int64 [8, 100, 100]).

    python tools/dataset_stats_time.py [--out FILE] [--iters 200] [--repeats 7] [--batch 8] [--kinds smooth random]

The yardstick is the host-to-device copy of the same pinned batch: NormValues.from_batches counts batch i while batch
i+1 is copied, so the pass is hidden when it takes less than the copy. Figures, alternated inside every repeat so that they
see the same machine state, each the time between two HIP events around `iters` back-to-back calls on one stream divided by
`iters`, warmed by untimed calls, with median, min and max over the repeats, in microseconds:
  add         DatasetStats.add: the three launches (histogram, batch reduce, label counts)
  hist        cn_chip_hist_u32 alone
  reduce      cn_hist_batch_reduce alone (on an already counted batch histogram: the same scan and the same stores)
  labels      cn_label_counts_i64 alone
  h2d         x and y from pinned memory to the device, non_blocking, into existing tensors
for two kinds of reflectance: `smooth` (a level per plane plus pixel noise of 150 counts: neighbouring values share bins,
as stored chips do) and `random` (uniform over 0..10000: every bin of every block is hit, the most the flush can cost).
`ratio` = add / h2d. As context, one CPU figure per kind: tests/stats_ref.py (sorted-array float64 restatement, numpy) over
the same batch, once, by the host clock. The reference's own CPU pass is not measured here.
One JSON line per figure."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cultionet_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--chip", type=int, nargs=4, default=[3, 12, 100, 100], help="C T H W")
    ap.add_argument("--kinds", nargs="+", default=["smooth", "random"], choices=["smooth", "random"])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cultionet_amd.configure_runtime()
    if not torch.cuda.is_available():
        raise SystemExit("dataset_stats_time.py measures on the GPU; there is none here")
    import stats_ref as R
    from cultionet_amd import _lib
    from cultionet_amd.data import Data
    from cultionet_amd.normalize import NBINS, DatasetStats

    B, (C, T, H, W) = args.batch, args.chip
    class_info = {"max_crop_class": 1, "edge_class": 2}
    g = np.random.default_rng(0)
    fns, host_x = {}, {}
    y_host = torch.from_numpy(g.choice(np.array([-1, 0, 1, 2]), (B, H, W), p=[0.05, 0.55, 0.3, 0.1])).pin_memory()
    for kind in args.kinds:
        if kind == "smooth":
            x = g.normal(2000, 900, (B, C, T, 1, 1)) + g.normal(0, 150, (B, C, T, H, W))
            x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
        else:
            x = g.integers(0, 10001, (B, C, T, H, W)).astype(np.int16)
        host_x[kind] = x
        xh = torch.from_numpy(x).pin_memory()
        xd, yd = xh.cuda(), y_host.cuda()
        stats = DatasetStats(C, class_info, "cuda")
        batch = Data(x=xd, y=yd)
        s = torch.cuda.current_stream().cuda_stream
        L = T * H * W

        def add(stats=stats, batch=batch):
            stats._filled = 0  # rewrite record 0: no chunk copy inside a window
            stats.add(batch)

        fns[f"add/{kind}"] = add
        full, alone = (torch.zeros(C * NBINS, dtype=torch.int32, device="cuda") for _ in range(2))
        fns[f"hist/{kind}"] = lambda xd=xd, h=alone: _lib.call("cn_chip_hist_u32", xd.data_ptr(), 2, h.data_ptr(), B, C, L,
                                                               NBINS, s)
        _lib.call("cn_chip_hist_u32", xd.data_ptr(), 2, full.data_ptr(), B, C, L, NBINS, s)
        work = torch.empty_like(full)

        def reduce(st=stats, full=full, work=work):
            work.copy_(full)  # the reduce pass zeroes what it reads; the refill is a 120 KB device copy inside the window
            _lib.call("cn_hist_batch_reduce", work.data_ptr(), st._hist.data_ptr(), st._weights.data_ptr(),
                      st._records.data_ptr(), 0, 1, C, NBINS, s)

        fns[f"reduce/{kind}"] = reduce
        fns[f"labels/{kind}"] = lambda yd=yd, st=stats: _lib.call("cn_label_counts_i64", yd.data_ptr(), 4, yd.numel(),
                                                                  st._labels.data_ptr(), st.nlab, s)

        def h2d(xh=xh, xd=xd, yd=yd):
            xd.copy_(xh, non_blocking=True)
            yd.copy_(y_host, non_blocking=True)

        fns[f"h2d/{kind}"] = h2d

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.repeats):
        for k, fn in fns.items():
            times[k].append(window(fn))
    lines = []
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        what, kind = k.split("/")
        row = {"figure": what, "values": kind, "shape": [B, C, T, H, W], "iters": args.iters, "repeats": args.repeats,
               "device_us": {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}}
        if what == "add":
            row["ratio_to_h2d"] = round(med[k] / med[f"h2d/{kind}"], 3)
        lines.append(json.dumps(row))
    for kind in args.kinds:
        t0 = time.perf_counter()
        R.dataset_stats([host_x[kind]])
        lines.append(json.dumps({"figure": "stats_ref_cpu", "values": kind, "shape": [B, C, T, H, W],
                                 "host_ms_once": round((time.perf_counter() - t0) * 1e3, 1)}))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
