"""The log transform's restatement (tests/log_transform_ref.py) against torch's own fp32 arithmetic, the log-domain bin
tables of cultionet_amd.normalize, and the host half of the dataset statistics in the log domain against brute force and
against the reference's own Variance / Quantile outputs (tests/golden/dataset_stats_log.npz, written by
tools/make_stats_log_golden.py). No GPU.

Bounds.
* Restatement against torch, before the z-score: 1 fp32 ulp. The restatement rounds the float64 logarithm once (half an
  ulp); torch's fp32 log is within 0.5001 ulp of float64 on all 10001 bin arguments (measured 0.50008, asserted below).
  The comparison feeds both the SAME fp32 v = (x / 10000).clip(1e-9, 1). The device prologue's v is x * fp32(1e-4)
  instead, which differs from the division in its last bit at 3186 of the 10001 bins (tests/test_pointwise_ref.py bounds
  that distance for the plain domain); through the two roundings of t and u that moves w by up to 4 ulp at 32 bins. That
  figure is printed here, not asserted: the GPU tests compare the kernels with the restatement of their own v.
* After the z-score: |inv| (ulp(w) + ulp(w - m)) + 2 ulp(z): one ulp between the two w, half an ulp on each side for the
  subtraction, and on z half an ulp for torch's division against one ulp for the fp32 reciprocal and the product.
* stats_from_counts against brute force: 1e-12 relative, the plain domain's bound (tests/test_stats_ref.py).
* Against the reference: std 1e-6 relative; mean, quantiles and batch medians 2 fp32 ulp at the value's magnitude (the
  reference accumulates in fp32 and the values reach 3.93). Measured when the fixture was written: std 6.0e-8, mean 1.21
  ulp (small), quantiles 0.5 ulp (odd), batch medians 0.
"""
import numpy as np
import pytest
import torch

import log_transform_ref as LR
import stats_ref as R
from stats_ref import CLASS_INFO, HOST_RTOL, STD_RTOL, batches_of, labels_for

CASES = ("small", "flat", "odd")
F = np.float32
FLOOR32 = F(1e-9)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(f"{golden_dir}/dataset_stats.npz"))


@pytest.fixture(scope="module")
def golden_log(golden_dir):
    return dict(np.load(f"{golden_dir}/dataset_stats_log.npz"))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the restatement against torch
# ---------------------------------------------------------------------------------------------------------------------
def test_torch_log_is_within_half_an_ulp_on_every_bin():
    """torch's fp32 log against float64 on the 10001 arguments u = fp32(fp32(v * 50) + 1) a stored reflectance can give:
    at most 0.5001 ulp (measured 0.50008)."""
    k = torch.arange(10001).float()
    u = (k / 10000.0).clip(1e-9, 1) * 50.0 + 1.0
    got = torch.log(u).double().numpy()
    want = np.log(u.double().numpy())
    err = np.max(np.abs(got - want)[1:] / LR.ulp32(want[1:]))
    print("torch log vs float64, worst ulp:", err)
    assert got[0] == 0.0 and want[0] == 0.0 and u[0] == 1.0
    assert err <= 0.5001


def test_restatement_meets_torch():
    """EdgeDataset.get's three lines with torch CPU fp32 on int16 [2,3,3,21,13], each channel holding -32768, -1, 0, 1,
    9999, 10000, 10001 and 32767."""
    x = LR.corner_raw((2, 3, 3, 21, 13), 2, 11)
    for c in range(3):
        assert set((-32768, -1, 0, 1, 9999, 10000, 10001, 32767)) <= set(x[:, c].reshape(-1).tolist())
    mean = np.array([0.9, 2.1, 0.004], dtype=np.float32)
    std = np.array([0.43, 0.88, 0.05], dtype=np.float32)
    v_t = (torch.from_numpy(x).float() / 10000.0).clip(1e-9, 1)                 # data/datasets.py:443
    w_t = torch.log(v_t * 50.0 + 1.0).clamp_min(1e-9)                           # data/datasets.py:481-484
    z_t = (w_t - torch.from_numpy(mean).view(1, 3, 1, 1, 1)) / torch.from_numpy(std).view(1, 3, 1, 1, 1)

    exp = LR.log_zscore(v_t.numpy(), mean, std)
    ulp = LR.ulp32(exp["w64"])
    d_w = np.max(np.abs(exp["w32"].astype(np.float64) - w_t.double().numpy()) / ulp)
    print("restatement vs torch, w: worst ulp", d_w)
    assert d_w <= 1.0
    low = x <= 0
    assert low.any() and (exp["w32"][low].view(np.uint32) == FLOOR32.view(np.uint32)).all()
    assert (w_t.numpy()[low].view(np.uint32) == FLOOR32.view(np.uint32)).all()
    assert exp["floor_at"][low].all()

    m = mean.astype(np.float64).reshape(1, 3, 1, 1, 1)
    inv = 1.0 / std.astype(np.float64).reshape(1, 3, 1, 1, 1)
    bound = inv * (ulp + LR.ulp32(np.abs(exp["w64"] - m) + ulp)) + 2 * LR.ulp32(np.abs(exp["z64"]) * (1 + 2.0 ** -20))
    d_z = np.max(np.abs(exp["out"].astype(np.float64) - z_t.double().numpy()) / bound)
    print("restatement vs torch, z: worst err / bound", d_z)
    assert d_z <= 1.0

    # the device prologue's v (x * fp32(1e-4)) instead of torch's division: reported, see the module docstring
    dev_v = LR.log_prepare_chips(x, None, None)
    print("prologue's v instead of torch's: w differs by up to",
          np.max(np.abs(dev_v["w32"].astype(np.float64) - w_t.double().numpy()) / ulp), "ulp")
    assert (dev_v["w32"][low].view(np.uint32) == FLOOR32.view(np.uint32)).all()


def test_an_fma_would_not_pass():
    """The tolerance separates the two roundings of t and u from a contracted fma(v, 50, 1). On stored integers the two
    forms give another fp32 u at 181 bins, and at the 23 lowest of them (38, 39, 40, 61, ...: fma_sensitive_bins) the fused
    form misses the bound, by up to 3.5 times without a z-score (measured). corner_raw plants eight
    of those bins in every plane the GPU tests prepare. (Off the integer grid, after an augmentation, a flip at the lowest
    bins costs hundreds of ulp of w: u moves by 2^-23 where w is 0.005.)"""
    bins = LR.fma_sensitive_bins()
    k = np.arange(1, 10001, dtype=np.float32)
    v = np.clip(k * F(1e-4), F(1e-9), F(1))
    exp = LR.log_zscore(v.reshape(1, 1, -1), None, None)
    fused = np.log((v.astype(np.float64) * 50.0 + 1.0).astype(np.float32).astype(np.float64)).astype(np.float32)
    ratio = np.abs(fused.astype(np.float64) - exp["z64"].reshape(-1)) / exp["tol"].reshape(-1)
    print("fma form: err / tol > 1 at", int((ratio > 1).sum()), "bins, worst", ratio.max(), "; sensitive bins", bins[:8])
    assert len(bins) >= 8 and bins[0] == 38 and np.all(ratio[bins - 1] > 1.0) and ratio.max() > 3
    x = LR.corner_raw((2, 3, 3, 21, 13), 2, 11)
    for c in range(3):
        assert set(bins[:8].tolist()) <= set(x[0, c].reshape(-1).tolist())


# ---------------------------------------------------------------------------------------------------------------------
# 2. bin tables
# ---------------------------------------------------------------------------------------------------------------------
def test_log_bin_tables():
    from cultionet_amd import normalize as N

    v, w = N.bin_values(log_transform=True), N.bin_weights(log_transform=True)
    assert v.dtype == np.float64 and w.dtype == np.int64 and v.shape == w.shape == (N.NBINS,)
    assert np.all(np.diff(v[1:]) > 0) and v[1] > v[0]
    assert v[0] == np.float64(FLOOR32) and 0.004987 < v[1] < 0.004988 and 3.931825 < v[-1] < 3.931826
    assert N.LOG_WEIGHT_SHIFT == 31 and N.weight_shift(True) == 31 and N.weight_shift(False) == N.WEIGHT_SHIFT
    assert w[0] == 0 and np.array_equal(w[1:] * 2.0 ** -31, v[1:]) and w.max() < 2 ** 34 < 2 ** 40
    t = (torch.arange(N.NBINS).float() / 10000.0).clip(1e-9, 1)  # the reference's own arithmetic
    assert np.array_equal(torch.log(t * 50.0 + 1.0).clamp_min(1e-9).double().numpy(), v)


def test_default_bin_tables_are_unchanged():
    from cultionet_amd import normalize as N

    k = np.arange(N.NBINS, dtype=np.float32)
    v = np.clip(k / np.float32(10000.0), np.float32(1e-9), np.float32(1.0)).astype(np.float64)
    w = np.round(v * 2.0 ** 37).astype(np.int64)
    w[0] = 0
    for got_v, got_w in ((N.bin_values(), N.bin_weights()), (N.bin_values(False), N.bin_weights(log_transform=False))):
        assert np.array_equal(got_v, v) and np.array_equal(got_w, w)


# ---------------------------------------------------------------------------------------------------------------------
# 3. stats_from_counts(log_transform=True) against brute force
# ---------------------------------------------------------------------------------------------------------------------
def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= HOST_RTOL * np.abs(b))


@pytest.mark.parametrize("centering", ["median", "mean"])
@pytest.mark.parametrize("name", CASES)
def test_host_half_meets_brute_force(golden, name, centering):
    from cultionet_amd import normalize as N

    batches = batches_of(golden, name)
    ys = labels_for(batches)
    nlab = CLASS_INFO["edge_class"] + 1
    records, hist = R.device_counts(batches, N.bin_weights(log_transform=True), N.NBINS)
    got = N.stats_from_counts(records, hist, R.label_counts(ys, nlab), CLASS_INFO, centering, 0.05, 0.95,
                              log_transform=True)
    want = LR.dataset_stats_log(batches, centering, 0.05, 0.95)
    for k in ("std", "mean", "lower_bound", "upper_bound"):
        assert close(got[k], want[k]), (k, got[k], want[k])
    if name == "flat":
        assert np.array_equal(got["std"], [0, 0])
    plain = N.stats_from_counts(*R.device_counts(batches, N.bin_weights(), N.NBINS), R.label_counts(ys, nlab), CLASS_INFO,
                                centering, 0.05, 0.95)
    if name != "flat":
        assert not np.allclose(plain["mean"], got["mean"])
    assert np.array_equal(plain["crop_counts"], got["crop_counts"])
    assert np.array_equal(plain["edge_counts"], got["edge_counts"])

    nv = N.NormValues.from_counts(records, hist, R.label_counts(ys, nlab), CLASS_INFO, centering, log_transform=True)
    for field, k in (("dataset_mean", "mean"), ("dataset_std", "std"), ("lower_bound", "lower_bound"),
                     ("upper_bound", "upper_bound")):
        t = getattr(nv, field)
        assert t.dtype == torch.float32 and tuple(t.shape) == (1, batches[0].shape[1], 1, 1, 1)
        assert np.array_equal(t.reshape(-1).numpy(), got[k].astype(np.float32))
    assert set(nv.data_dict) == {"dataset_mean", "dataset_std", "dataset_crop_counts", "dataset_edge_counts",
                                 "num_channels", "lower_bound", "upper_bound"}  # no new key in a .norm file


# ---------------------------------------------------------------------------------------------------------------------
# 4. pinned to the reference
# ---------------------------------------------------------------------------------------------------------------------
def ulps(got64, want32):
    want32 = np.asarray(want32, dtype=np.float32)
    return np.abs(got64 - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


def reference_deviation(batches, golden_log, name):
    """[std relative, quantiles, mean, batch medians in fp32 ulp] of the float64 brute force from the reference's outputs."""
    fed = [LR.prepared_log(b) for b in batches]
    rows = np.concatenate(fed)
    assert len(rows) <= 12288  # beyond this the reference's sketch subsamples and pins nothing
    std, want = R.variance_median_std(fed), golden_log[f"{name}_std"].astype(np.float64)
    assert np.all(std[want == 0] == 0)
    return np.array([np.max(np.abs(std[want != 0] / want[want != 0] - 1), initial=0.0),
                     np.max(ulps(R.sketch_quantiles(rows, golden_log["quantiles"]), golden_log[f"{name}_quantiles"])),
                     np.max(ulps(R.sketch_mean(rows), golden_log[f"{name}_mean"])),
                     np.max(ulps(np.stack([R.lower_median(f) for f in fed]), golden_log[f"{name}_batch_medians"]))])


REF_BOUNDS = np.array([STD_RTOL, 2.0, 2.0, 2.0])


@pytest.mark.parametrize("name", CASES)
def test_brute_force_meets_the_reference(golden, golden_log, name):
    dev = reference_deviation(batches_of(golden, name), golden_log, name)
    print(name, "std rel", dev[0], "quantiles", dev[1], "mean", dev[2], "batch medians", dev[3], "(fp32 ulp)")
    assert np.all(dev <= REF_BOUNDS)
    assert np.all(golden_log[f"{name}_dev"] <= REF_BOUNDS)  # what the tool measured when it wrote the fixture


@pytest.mark.parametrize("name", CASES)
def test_host_half_meets_the_reference(golden, golden_log, name):
    """stats_from_counts(log_transform=True) itself against the reference's outputs, with the same bounds."""
    from cultionet_amd import normalize as N

    batches = batches_of(golden, name)
    records, hist = R.device_counts(batches, N.bin_weights(True), N.NBINS)
    q = golden_log["quantiles"]
    med = N.stats_from_counts(records, hist, np.zeros(6, dtype=np.int64), CLASS_INFO, "median", q[0], q[2], True)
    mean = N.stats_from_counts(records, hist, np.zeros(6, dtype=np.int64), CLASS_INFO, "mean", q[0], q[2], True)
    want_std = golden_log[f"{name}_std"].astype(np.float64)
    nz = want_std != 0
    assert np.all(med["std"][~nz] == 0)
    assert np.max(np.abs(med["std"][nz] / want_std[nz] - 1), initial=0.0) <= STD_RTOL
    got_q = np.stack([med["lower_bound"], med["mean"], med["upper_bound"]], axis=1)
    assert np.max(ulps(got_q, golden_log[f"{name}_quantiles"])) <= 2.0
    assert np.max(ulps(mean["mean"], golden_log[f"{name}_mean"])) <= 2.0
    values = N.bin_values(True)
    assert np.max(ulps(values[records[:, :, 2]], golden_log[f"{name}_batch_medians"])) <= 2.0


def test_flat_case_is_what_it_says(golden_log):
    assert np.array_equal(golden_log["flat_std"], [0, 0])
    top = torch.log(torch.tensor(1.0) * 50.0 + 1.0).numpy()
    assert np.array_equal(golden_log["flat_quantiles"], np.float32([[1e-9] * 3, [top] * 3]))


# ---------------------------------------------------------------------------------------------------------------------
# the keyword where no GPU is needed to see it
# ---------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_in_every_signature():
    import inspect

    from cultionet_amd import normalize as N
    from cultionet_amd.augment import DeviceAugmenter
    from cultionet_amd.edges import LOG_FLOOR, LOG_GAIN, prepare_chips
    from cultionet_amd.feeder import DeviceFeeder
    from cultionet_amd.lightning import LightningModuleMixin
    from cultionet_amd.predict import SlidingWindowPredictor

    for fn in (prepare_chips, DeviceAugmenter.apply, DeviceFeeder.__init__, LightningModuleMixin.set_norm_values,
               SlidingWindowPredictor.__init__, N.NormValues.from_batches, N.NormValues.from_counts,
               N.DatasetStats.__init__, N.stats_from_counts, N.bin_values, N.bin_weights):
        assert inspect.signature(fn).parameters["log_transform"].default is False, fn
    assert inspect.signature(N.DatasetStats.finish).parameters["log_transform"].default is None
    assert (LOG_GAIN, LOG_FLOOR) == (50.0, 1e-9)
