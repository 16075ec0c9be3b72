"""numpy float64 restatement of what NormValues.from_dataset (utils/normalize.py:118-213) computes, written from SORTED
ARRAYS of the values the reference is fed -- no histogram anywhere, so it shares nothing with cultionet_amd.normalize or
the kernels. tests/test_stats_ref.py pins it to the reference's own Variance / Quantile outputs
(tests/golden/dataset_stats.npz).

The normalize.py formulas for the class counts cannot be executed from the reference (the module pulls in rich, joblib and
the data package); `class_counts` restates lines 180-191 one to one.
"""
import numpy as np


def prepared(x_raw):
    """EdgeDataset.get's (x / 10000).clip(1e-9, 1) in fp32 (data/datasets.py:443), rearranged 'b c t h w -> (b t h w) c'
    (normalize.py:173) and widened to float64."""
    x = np.asarray(x_raw).astype(np.float32) / np.float32(10000.0)
    x = np.clip(x, np.float32(1e-9), np.float32(1.0))
    return np.moveaxis(x, 1, -1).reshape(-1, x.shape[1]).astype(np.float64)


def lower_median(a):
    """a.median(dim=0)[0] of torch: the element of sorted rank (n - 1) // 2."""
    s = np.sort(a, axis=0)
    return s[(len(s) - 1) // 2]


def variance_median_std(batches):
    """Variance(method='median'): add() per batch, then std() (utils/stats.py:642-683). batches: arrays [rows, C]."""
    count, mean, cmom2 = 0, None, None
    for a in batches:
        if len(a) == 0:
            continue
        m = lower_median(a)
        centred = ((a - m) ** 2).sum(axis=0)
        if mean is None:
            count, mean, cmom2 = len(a), m.copy(), centred
            continue
        oldcount = count
        count += len(a)
        new_frac = float(len(a)) / count
        delta = (m - mean) * new_frac
        mean = mean + delta
        cmom2 = cmom2 + centred
        cmom2 = cmom2 + delta ** 2 * (new_frac * oldcount)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(cmom2 / np.float64(count - 1))


def sketch_quantiles(rows, q):
    """Quantile.quantiles(q) (utils/stats.py:519-575) while the sketch holds every sample at weight 1: np.interp over
    [min, sorted samples, max] at cumulative weights [0, (i - 0.5) / n, 1]. q goes through fp32, as torch.tensor(q)."""
    s = np.sort(rows, axis=0)
    n = len(s)
    xp = np.concatenate([[0.0], (np.arange(1, n + 1) - 0.5) / n, [1.0]])
    q = np.atleast_1d(np.asarray(q, dtype=np.float32)).astype(np.float64)
    out = np.empty((s.shape[1], len(q)))
    for c in range(s.shape[1]):
        out[c] = np.interp(q, xp, np.concatenate([s[:1, c], s[:, c], s[-1:, c]]))
    return out


def sketch_mean(rows):
    """Quantile.mean() (utils/stats.py:455-456) at samplerate 1: the plain mean."""
    return rows.sum(axis=0) / len(rows)


def class_counts(ys, max_crop_class, edge_class):
    """normalize.py:148-149 and 180-191 over the label arrays of every batch."""
    crop_counts = np.zeros(max_crop_class + 1, dtype=np.int64)
    edge_counts = np.zeros(2, dtype=np.int64)
    for y in ys:
        y = np.asarray(y).astype(np.int64)
        crop_counts[0] += ((y == 0) | (y == edge_class)).sum()
        for i in range(1, edge_class):
            crop_counts[i] += (y == i).sum()
        edge_counts[0] += ((y >= 0) & (y != edge_class)).sum()
        edge_counts[1] += (y == edge_class).sum()
    return crop_counts, edge_counts


def dataset_stats(x_batches, centering="median", lower_quantile=0.05, upper_quantile=0.95):
    """x_batches: raw integer arrays [B, C, T, H, W] -> dict of float64 [C] arrays, as from_dataset orders its work."""
    fed = [prepared(x) for x in x_batches]
    rows = np.concatenate(fed)
    q = sketch_quantiles(rows, [lower_quantile, 0.5, upper_quantile])
    return {"std": variance_median_std(fed), "mean": sketch_mean(rows) if centering == "mean" else q[:, 1],
            "lower_bound": q[:, 0], "upper_bound": q[:, 2]}


# ---- integer restatement of the device counts, from sorted ranks and plain sums (no float anywhere) ----------------
def device_counts(x_batches, weights, nbins=10001):
    """What cn_chip_hist_u32 + cn_hist_batch_reduce leave: (records [batches, C, 7] int64, dataset histogram [C, nbins])."""
    C = x_batches[0].shape[1]
    hist = np.zeros((C, nbins), dtype=np.int64)
    records = np.zeros((len(x_batches), C, 7), dtype=np.int64)
    w = [int(v) for v in weights]
    for i, x in enumerate(x_batches):
        bins = np.clip(np.asarray(x).astype(np.int64), 0, nbins - 1)
        for c in range(C):
            b = np.sort(bins[:, c].reshape(-1))
            h = np.bincount(b, minlength=nbins)
            hist[c] += h
            s1 = sum(int(h[k]) * w[k] for k in np.nonzero(h)[0])
            s2 = sum(int(h[k]) * w[k] * w[k] for k in np.nonzero(h)[0])
            words = [len(b), int(h[0]), int(b[(len(b) - 1) // 2]), s1 & (2 ** 64 - 1), s1 >> 64, s2 & (2 ** 64 - 1), s2 >> 64]
            records[i, c] = np.array(words, dtype=np.uint64).astype(np.int64)
    return records, hist


def label_counts(ys, nlab):
    out = np.zeros(nlab + 2, dtype=np.int64)
    for y in ys:
        y = np.asarray(y).astype(np.int64).reshape(-1)
        out[0] += (y < 0).sum()
        out[-1] += (y >= nlab).sum()
        for v in range(nlab):
            out[1 + v] += (y == v).sum()
    return out


# ---- shared by tests/test_stats_ref.py and tests/test_dataset_stats_gpu.py ------------------------------------------
STD_RTOL, ABS_TOL, HOST_RTOL = 1e-6, 2.4e-7, 1e-12  # derived in tests/test_stats_ref.py
CLASS_INFO = {"max_crop_class": 2, "edge_class": 3}


def batches_of(golden, name):
    out = []
    while f"{name}_x{len(out)}" in golden:
        out.append(golden[f"{name}_x{len(out)}"])
    return out


def labels_for(batches, seed=5):
    """Label planes [B, H, W] with -1, 0, crop classes 1 and 2, the edge class 3 and a value above it."""
    g = np.random.default_rng(seed)
    return [g.choice(np.array([-1, 0, 1, 2, 3, 4]), (x.shape[0],) + x.shape[3:], p=[0.1, 0.4, 0.2, 0.1, 0.15, 0.05])
            for x in batches]
