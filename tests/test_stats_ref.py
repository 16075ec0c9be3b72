"""tests/stats_ref.py against the reference's own Variance / Quantile outputs (tests/golden/dataset_stats.npz, written by
tools/make_stats_golden.py), and the host half of cultionet_amd.normalize against tests/stats_ref.py. No GPU.

Bounds. The golden is the reference's fp32 arithmetic over at most 12288 rows, the restatement is float64:
* std within 1e-6 relative (fp32 sums of up to 12288 squares); where the reference is exactly 0 the restatement is 0;
* quantiles, mean and batch medians within 2.4e-7 absolute, 4 fp32 ulp at 1.0.
Measured when the fixture was written (its `<case>_dev` arrays, checked below): std 8.5e-8, quantiles 3.0e-8, mean
2.3e-8, batch medians 0 -- each below a fifth of its bound.
* stats_from_counts works from integer counts and rounds each batch's centred sum once, the restatement sums float64
  squares of sorted values: 1e-12 relative between the two.
"""
import numpy as np
import pytest
import torch

import stats_ref as R
from stats_ref import ABS_TOL, CLASS_INFO, HOST_RTOL, STD_RTOL, batches_of, labels_for

CASES = ("small", "flat", "odd")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(f"{golden_dir}/dataset_stats.npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_meets_the_reference(golden, name):
    fed = [R.prepared(b) for b in batches_of(golden, name)]
    rows = np.concatenate(fed)
    assert len(rows) <= 12288  # beyond this the reference's sketch subsamples and pins nothing
    std, want = R.variance_median_std(fed), golden[f"{name}_std"].astype(np.float64)
    q = R.sketch_quantiles(rows, golden["quantiles"])
    mean = R.sketch_mean(rows)
    med = np.stack([R.lower_median(f) for f in fed])
    dev = np.array([np.max(np.abs(std[want != 0] / want[want != 0] - 1), initial=0.0),
                    np.max(np.abs(q - golden[f"{name}_quantiles"])), np.max(np.abs(mean - golden[f"{name}_mean"])),
                    np.max(np.abs(med - golden[f"{name}_batch_medians"]))])
    print(name, "std rel", dev[0], "quantiles", dev[1], "mean", dev[2], "batch medians", dev[3])
    assert np.all(std[want == 0] == 0)
    assert dev[0] <= STD_RTOL and np.all(dev[1:] <= ABS_TOL)
    assert np.all(golden[f"{name}_dev"] <= np.array([STD_RTOL, ABS_TOL, ABS_TOL, ABS_TOL]) / 5)


def test_flat_case_is_what_it_says(golden):
    assert np.array_equal(golden["flat_std"], [0, 0])
    assert np.array_equal(golden["flat_quantiles"], np.float32([[1e-9] * 3, [1.0] * 3]))


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= HOST_RTOL * np.abs(b))


@pytest.mark.parametrize("centering", ["median", "mean"])
@pytest.mark.parametrize("name", CASES)
def test_host_half_meets_the_restatement(golden, name, centering):
    from cultionet_amd import normalize as N

    batches = batches_of(golden, name)
    ys = labels_for(batches)
    nlab = CLASS_INFO["edge_class"] + 1
    records, hist = R.device_counts(batches, N.bin_weights(), N.NBINS)
    got = N.stats_from_counts(records, hist, R.label_counts(ys, nlab), CLASS_INFO, centering, 0.05, 0.95)
    want = R.dataset_stats(batches, centering, 0.05, 0.95)
    for k in ("std", "mean", "lower_bound", "upper_bound"):
        assert close(got[k], want[k]), (k, got[k], want[k])
    if name == "flat":
        assert np.array_equal(got["std"], [0, 0])
    crop, edge = R.class_counts(ys, **CLASS_INFO)
    assert np.array_equal(got["crop_counts"], crop) and np.array_equal(got["edge_counts"], edge)
    assert crop.sum() > 0 and edge.min() > 0

    nv = N.NormValues.from_counts(records, hist, R.label_counts(ys, nlab), CLASS_INFO, centering)
    C = batches[0].shape[1]
    assert nv.num_channels == C
    for field, k in (("dataset_mean", "mean"), ("dataset_std", "std"), ("lower_bound", "lower_bound"),
                     ("upper_bound", "upper_bound")):
        t = getattr(nv, field)
        assert t.dtype == torch.float32 and tuple(t.shape) == (1, C, 1, 1, 1)
        assert np.array_equal(t.reshape(-1).numpy(), got[k].astype(np.float32))
    assert nv.dataset_crop_counts.dtype == torch.int64 and nv.dataset_edge_counts.dtype == torch.int64
    assert tuple(nv.dataset_crop_counts.shape) == (CLASS_INFO["max_crop_class"] + 1,)


def test_quantiles_at_the_ends_and_between_samples():
    """np.interp's three regimes: below the first sample, above the last, and a q that lands between two samples."""
    from cultionet_amd import normalize as N

    x = np.array([100, 100, 300, 700, 700, 900, 10000, -5], dtype=np.int16).reshape(1, 1, 1, 2, 4)
    records, hist = R.device_counts([x], N.bin_weights(), N.NBINS)
    rows = R.prepared(x)
    for q in (0.0, 0.01, 0.0625, 0.3, 0.5, 0.77, 0.9375, 0.99, 1.0):
        got = N.stats_from_counts(records, hist, np.zeros(3, dtype=np.int64), {"max_crop_class": 0, "edge_class": 0},
                                  "median", q, q)["lower_bound"]
        assert close(got, R.sketch_quantiles(rows, q)[:, 0]), q


def test_bin_weights_are_exact():
    from cultionet_amd import normalize as N

    v, w = N.bin_values(), N.bin_weights()
    assert v[0] == np.float64(np.float32(1e-9)) and v[-1] == 1.0 and w[0] == 0 and w[-1] == 2 ** N.WEIGHT_SHIFT
    assert np.array_equal(w[1:] * 2.0 ** -N.WEIGHT_SHIFT, v[1:]) and w.max() < 2 ** 40
    t = torch.arange(N.NBINS).float() / 10000.0  # the reference's own arithmetic
    assert np.array_equal(t.clip(1e-9, 1).double().numpy(), v)


def test_class_info_where_the_reference_would_raise():
    from cultionet_amd import normalize as N

    with pytest.raises(ValueError):
        N.stats_from_counts(np.zeros((0, 1, 7)), np.zeros((1, N.NBINS)), np.zeros(6), {"max_crop_class": 1, "edge_class": 3})


def test_norm_values_file_round_trip(tmp_path, golden):
    pytest.importorskip("joblib")
    import joblib

    from cultionet_amd import normalize as N

    batches = batches_of(golden, "odd")
    records, hist = R.device_counts(batches, N.bin_weights(), N.NBINS)
    nv = N.NormValues.from_counts(records, hist, R.label_counts(labels_for(batches), 4), CLASS_INFO)
    path = tmp_path / "last.norm"
    nv.to_file(path)
    raw = joblib.load(path)  # what the reference's from_file hands to its constructor (normalize.py:114-116)
    assert set(raw) == {"dataset_mean", "dataset_std", "dataset_crop_counts", "dataset_edge_counts", "num_channels",
                        "lower_bound", "upper_bound"}
    back = N.NormValues.from_file(path)
    for k, v in nv.data_dict.items():
        w = back.data_dict[k]
        assert torch.equal(v, w) if isinstance(v, torch.Tensor) else v == w


def test_transform_round_trip(golden):
    from cultionet_amd import normalize as N
    from cultionet_amd.data import Data

    batches = batches_of(golden, "small")
    records, hist = R.device_counts(batches, N.bin_weights(), N.NBINS)
    nv = N.NormValues.from_counts(records, hist, np.zeros(5, dtype=np.int64), CLASS_INFO)
    x = torch.from_numpy(R.prepared(batches[1]).T.reshape(1, 3, 3, 32, 32).astype(np.float32))
    z = nv(Data(x=x))
    assert torch.allclose(z.x, (x - nv.dataset_mean) / nv.dataset_std)
    assert torch.allclose(nv.inverse_transform(z).x, x, atol=1e-6)
