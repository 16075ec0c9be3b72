#!/usr/bin/env python
"""Writes tests/golden/dataset_stats_log.npz: what the reference's own Variance(method='median') and Quantile(r=1024 * 6)
(cultionet/utils/stats.py:236-683) make of the raw batches of tests/golden/dataset_stats.npz when the dataset is built
with log_transform=True, fed as NormValues.from_dataset feeds them (utils/normalize.py:142-143, 173-177, 193-199) after
EdgeDataset.get (data/datasets.py:443, 481-484):
    x = (raw.float() / 10000).clip(1e-9, 1);  x = torch.log(x * 50.0 + 1.0).clamp_min(1e-9)
rearranged 'b c t h w -> (b t h w) c', stat_var.add(x), stat_q.add(x), then std(), quantiles(0.05 / 0.5 / 0.95), mean().

    python tools/make_stats_log_golden.py /path/to/reference/src

The companion of tools/make_stats_golden.py: the same three cases (small, flat, odd; read from its fixture, so the raw
batches are stored once), the same arrays per case (`<case>_std`, `_mean` float32 [C]; `<case>_quantiles` float32 [C, 3];
`<case>_batch_medians` float32 [batches, C]) and `<case>_dev` float64 [4]: the largest deviation of
tests/log_transform_ref.py's float64 restatement from these fp32 outputs -- std relative; quantiles, mean and batch medians
in fp32 ulp at the magnitude of the reference's value. Every case stays at or below 12288 rows, the most the sketch holds
without discarding; the tool asserts samplerate == 1.0. The file is written with fixed zip timestamps.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import log_transform_ref as LR  # noqa: E402
import stats_ref as R  # noqa: E402
from make_stats_golden import MAX_ROWS, QUANTILES, load_reference, save  # noqa: E402


def ulps(got64, want32):
    """|got - want| in units of the fp32 spacing at |want|."""
    want32 = np.asarray(want32, dtype=np.float32)
    return np.abs(got64 - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def run(ref, name, batches, out):
    stat_var, stat_q = ref.Variance(method="median"), ref.Quantile(r=1024 * 6)
    medians = []
    for raw in batches:
        x = (torch.from_numpy(raw).float() / 10000.0).clip(1e-9, 1)          # data/datasets.py:443
        x = torch.log(x * 50.0 + 1.0).clamp_min(1e-9)                       # data/datasets.py:481-484
        x = x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])                # 'b c t h w -> (b t h w) c'
        medians.append(x.median(dim=0)[0].numpy().copy())
        stat_var.add(x)
        stat_q.add(x)
    rows = sum(b.size // b.shape[1] for b in batches)
    assert rows <= MAX_ROWS and stat_q.samplerate == 1.0 and len(stat_q.data) == 1 and stat_q.count == rows
    got = {"std": stat_var.std().numpy(), "mean": stat_q.mean().numpy(),
           "quantiles": stat_q.quantiles(list(QUANTILES)).numpy(), "batch_medians": np.stack(medians)}
    assert all(v.dtype == np.float32 for v in got.values())
    fed = [LR.prepared_log(b) for b in batches]
    allrows = np.concatenate(fed)
    std = R.variance_median_std(fed)
    nz = got["std"] != 0
    assert np.all(std[~nz] == 0)
    dev = np.array([np.max(np.abs(std[nz] / got["std"][nz] - 1), initial=0.0),
                    np.max(ulps(R.sketch_quantiles(allrows, QUANTILES), got["quantiles"])),
                    np.max(ulps(R.sketch_mean(allrows), got["mean"])),
                    np.max(ulps(np.stack([R.lower_median(f) for f in fed]), got["batch_medians"]))])
    print(f"{name}: rows {rows}, std {got['std']}, restatement off by std {dev[0]:.2e} rel, quantiles {dev[1]:.3f}, "
          f"mean {dev[2]:.3f}, batch medians {dev[3]:.3f} fp32 ulp")
    out.update({f"{name}_{k}": v for k, v in got.items()})
    out[f"{name}_dev"] = dev


def main():
    ref = load_reference(sys.argv[1])
    plain = dict(np.load(os.path.join(ROOT, "tests", "golden", "dataset_stats.npz")))
    out = {"quantiles": np.array(QUANTILES)}
    for name in ("small", "flat", "odd"):
        run(ref, name, R.batches_of(plain, name), out)
    dst = os.path.join(ROOT, "tests", "golden", "dataset_stats_log.npz")
    save(dst, out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
