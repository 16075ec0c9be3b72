#!/usr/bin/env python
"""Writes tests/golden/dataset_stats.npz: what the reference's own Variance(method='median') and Quantile(r=1024 * 6)
(cultionet/utils/stats.py:236-683) make of small raw batches, fed exactly as NormValues.from_dataset feeds them
(utils/normalize.py:142-143, 173-177, 193-199): x = (raw.float() / 10000).clip(1e-9, 1) (data/datasets.py:443) rearranged
'b c t h w -> (b t h w) c', stat_var.add(x), stat_q.add(x), then std(), quantiles(0.05 / 0.5 / 0.95) and mean().

    python tools/make_stats_golden.py /path/to/reference/src

utils/stats.py imports only numpy and torch and is executed from where it lies, loaded by path. normalize.py itself is
not imported (it pulls in rich, joblib and the data package): the class-count formulas of its lines 180-191 are restated
in tests/stats_ref.py, with nothing of the reference to pin them.

Every case stays at or below 12288 rows, the most the sketch holds without discarding: above that the reference's
quantiles are a randomized approximation and pin nothing. The tool asserts samplerate == 1.0 and a single level.

Cases (arrays `<case>_x<i>` raw batches [B, C, T, H, W]; `<case>_std`, `_mean` float32 [C]; `<case>_quantiles` float32
[C, 3] at 0.05, 0.5, 0.95; `<case>_batch_medians` float32 [batches, C], a.median(dim=0)[0] of each fed batch, the call
Variance.add makes; `<case>_dev` float64 [4]: the largest deviation of tests/stats_ref.py from these outputs -- std
relative, quantiles, mean and batch medians absolute):
  small  C 3, int16, batches [2,3,3,32,32], [1,3,3,32,32], [1,3,3,32,32]: 12288 rows; channel 0 in multiples of 50 (heavy
         ties); negatives, 0, 10000, values above 10000 and -32768 / 32767 in every channel
  flat   C 2, int16, one batch [1,2,2,8,8]: channel 0 all <= 0 (every value 1e-9, std 0), channel 1 all 10000
  odd    C 5, int16, two batches [3,5,3,7,5]: L = 105, planes start at odd element offsets
The file is written with fixed zip timestamps, so a rerun reproduces it byte for byte.
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stats_ref as R  # noqa: E402

QUANTILES = (0.05, 0.5, 0.95)
MAX_ROWS = 12288


def load_reference(src):
    spec = importlib.util.spec_from_file_location("cultionet_utils_stats", os.path.join(src, "cultionet", "utils", "stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def smooth(g, shape, centre, spread):
    """Reflectance-like planes: a per-plane level plus pixel noise."""
    level = g.normal(centre, spread, shape[:3] + (1, 1))
    return level + g.normal(0, spread / 4, shape)


def small_batches():
    g = np.random.default_rng(2024)
    out = []
    for B in (2, 1, 1):
        shape = (B, 3, 3, 32, 32)
        x = np.empty(shape)
        x[:, 0] = np.round(smooth(g, shape, 2500, 900)[:, 0] / 50) * 50
        x[:, 1] = smooth(g, shape, 4200, 1500)[:, 1]
        x[:, 2] = smooth(g, shape, 300, 500)[:, 2]           # about a quarter below 0
        x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
        for c in range(3):                                   # the clip's corners, in every channel of every batch
            flat = x[:, c].reshape(-1)
            flat[g.choice(flat.size, 9, replace=False)] = [-32768, -1, 0, 1, 9999, 10000, 10001, 12500, 32767]
            x[:, c] = flat.reshape(x[:, c].shape)
        out.append(x)
    return out


def flat_batches():
    g = np.random.default_rng(7)
    x = np.empty((1, 2, 2, 8, 8), dtype=np.int16)
    x[:, 0] = g.choice(np.array([0, -1, -250, -32768], dtype=np.int16), (1, 2, 8, 8))
    x[:, 1] = 10000
    return [x]


def odd_batches():
    g = np.random.default_rng(99)
    return [np.clip(np.round(smooth(g, (3, 5, 3, 7, 5), 1800, 700)), -32768, 32767).astype(np.int16) for _ in range(2)]


def run(ref, name, batches, out):
    stat_var, stat_q = ref.Variance(method="median"), ref.Quantile(r=1024 * 6)
    medians = []
    for raw in batches:
        x = (torch.from_numpy(raw).float() / 10000.0).clip(1e-9, 1)          # data/datasets.py:443
        x = x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])                # 'b c t h w -> (b t h w) c'
        medians.append(x.median(dim=0)[0].numpy().copy())
        stat_var.add(x)
        stat_q.add(x)
    rows = sum(b.size // b.shape[1] for b in batches)
    assert rows <= MAX_ROWS and stat_q.samplerate == 1.0 and len(stat_q.data) == 1 and stat_q.count == rows
    got = {"std": stat_var.std().numpy(), "mean": stat_q.mean().numpy(),
           "quantiles": stat_q.quantiles(list(QUANTILES)).numpy(), "batch_medians": np.stack(medians)}
    assert all(v.dtype == np.float32 for v in got.values())
    # how far the float64 restatement is from the reference's fp32 arithmetic
    fed = [R.prepared(b) for b in batches]
    allrows = np.concatenate(fed)
    std = R.variance_median_std(fed)
    nz = got["std"] != 0
    assert np.all(std[~nz] == 0)
    dev = np.array([np.max(np.abs(std[nz] / got["std"][nz] - 1), initial=0.0),
                    np.max(np.abs(R.sketch_quantiles(allrows, QUANTILES) - got["quantiles"])),
                    np.max(np.abs(R.sketch_mean(allrows) - got["mean"])),
                    np.max(np.abs(np.stack([R.lower_median(f) for f in fed]) - got["batch_medians"]))])
    print(f"{name}: rows {rows}, std {got['std']}, restatement off by std {dev[0]:.2e} rel, quantiles {dev[1]:.2e}, "
          f"mean {dev[2]:.2e}, batch medians {dev[3]:.2e} abs")
    for i, b in enumerate(batches):
        out[f"{name}_x{i}"] = b
    out.update({f"{name}_{k}": v for k, v in got.items()})
    out[f"{name}_dev"] = dev


def save(dst, arrays):
    """np.savez_compressed with fixed member timestamps."""
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    ref = load_reference(sys.argv[1])
    out = {"quantiles": np.array(QUANTILES)}
    run(ref, "small", small_batches(), out)
    run(ref, "flat", flat_batches(), out)
    run(ref, "odd", odd_batches(), out)
    dst = os.path.join(ROOT, "tests", "golden", "dataset_stats.npz")
    save(dst, out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
