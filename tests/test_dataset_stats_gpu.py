"""Dataset statistics on the device (cn_chip_hist_u32, cn_hist_batch_reduce, cn_label_counts_i64,
cultionet_amd.normalize) against tests/stats_ref.py, itself pinned to the reference's own Variance / Quantile by
tests/test_stats_ref.py.

Conditions:
* everything the device writes is an integer: records, dataset histogram and label counts are torch.equal to the numpy
  restatement (bincount, sorted rank, integer moments), the batch histogram is all zero after the reduce pass, and a second
  run gives the same bytes;
* finish() meets the recorded outputs of the reference within the bounds of tests/test_stats_ref.py (std 1e-6 relative and 0
  where the reference is 0; mean and quantiles 2.4e-7 absolute); stats_from_counts over the device's counts meets
  tests/stats_ref.py at 1e-12 relative in float64, and finish() stores exactly those figures rounded to float32;
* prepare_chips with the computed mean / std leaves a per-channel median of 0 within the four fp32 roundings of a value in
  [0, 1] (raw * 1e-4f, the stored mean, the subtraction, the division): 4 * 6e-8 / std.
"""
import numpy as np
import pytest
import torch

import stats_ref as R
from stats_ref import ABS_TOL, CLASS_INFO, HOST_RTOL, STD_RTOL, batches_of, labels_for

pytestmark = pytest.mark.gpu

NLAB = CLASS_INFO["edge_class"] + 1


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(f"{golden_dir}/dataset_stats.npz"))


def smooth_i16(shape, seed):
    g = np.random.default_rng(seed)
    level = g.normal(2000, 900, shape[:3] + (1, 1))
    return np.clip(np.round(level + g.normal(0, 150, shape)), -32768, 32767).astype(np.int16)


def extra_batches(name):
    g = np.random.default_rng(3)
    if name == "u16":  # 65535 and the clamp at 10000
        x = g.integers(0, 65536, (2, 2, 2, 9, 11)).astype(np.uint16)
        x.reshape(-1)[[0, 7, 395]] = [65535, 0, 10000]
        return [torch.from_numpy(x)]
    if name == "i32":  # both ends of int32, and values whose low 16 bits alone would be in range
        x = g.integers(-20000, 30000, (1, 3, 2, 10, 7)).astype(np.int32)
        x.reshape(-1)[[0, 1, 2, 3, 139, 140]] = [-2 ** 31, 2 ** 31 - 1, 65536 + 5, -65536 + 5, 2 ** 31 - 1, -2 ** 31]
        return [torch.from_numpy(x)]
    if name == "blocks":  # 240000 values per channel: seven blocks per channel meet in the global flush
        return [torch.from_numpy(smooth_i16((2, 3, 12, 100, 100), 4))]
    if name == "one_bin":  # every value in one bin: every LDS atomic of a block goes to one address
        return [torch.full((2, 2, 3, 64, 64), 1234, dtype=torch.int16), torch.full((1, 2, 3, 64, 64), -7, dtype=torch.int16)]
    raise KeyError(name)


def batches(golden, name):
    if name in ("small", "flat", "odd"):
        return [torch.from_numpy(b) for b in batches_of(golden, name)]
    return extra_batches(name)


def count(xs, ys=None, record_chunk=256):
    from cultionet_amd.data import Data
    from cultionet_amd.normalize import DatasetStats

    stats = DatasetStats(xs[0].shape[1], CLASS_INFO, "cuda", record_chunk=record_chunk)
    for i, x in enumerate(xs):
        stats.add(Data(x=x.cuda(), y=None if ys is None else ys[i].cuda()))
    out = stats.counts()
    assert not stats._batch_hist.any()  # the reduce pass leaves the batch histogram zeroed
    return stats, out


@pytest.fixture(scope="module")
def counted(golden):
    """name -> (host batches, label planes, DatasetStats, counts): every case is counted once."""
    cache = {}

    def get(name):
        if name not in cache:
            xs = batches(golden, name)
            ys = [torch.from_numpy(y) for y in labels_for([x.numpy() for x in xs])]
            cache[name] = (xs, ys) + count(xs, ys, record_chunk=2 if name == "small" else 256)
        return cache[name]

    return get


@pytest.mark.parametrize("name", ["small", "flat", "odd", "u16", "i32", "blocks", "one_bin"])
def test_counts_equal_numpy(counted, name):
    from cultionet_amd.normalize import NBINS, bin_weights

    xs, ys, _, (records, hist, labels) = counted(name)
    want_records, want_hist = R.device_counts([x.numpy() for x in xs], bin_weights(), NBINS)
    assert records.dtype == np.int64 and hist.dtype == np.int64
    assert torch.equal(torch.from_numpy(hist), torch.from_numpy(want_hist))
    assert torch.equal(torch.from_numpy(records), torch.from_numpy(want_records))
    assert torch.equal(torch.from_numpy(labels), torch.from_numpy(R.label_counts([y.numpy() for y in ys], NLAB)))
    _, (records2, hist2, labels2) = count(xs, ys)
    assert records2.tobytes() == records.tobytes() and hist2.tobytes() == hist.tobytes()
    assert labels2.tobytes() == labels.tobytes()


def test_integer_moments_with_unit_weights():
    """The record's moments over w_k = k: S1 = sum of the clamped values, S2 = sum of their squares."""
    from cultionet_amd import _lib

    x = torch.from_numpy(smooth_i16((2, 2, 3, 21, 13), 8))
    nbins = 4000  # below the data's range: the clamp at nbins - 1 takes part
    w = np.arange(nbins, dtype=np.int64)
    want_records, want_hist = R.device_counts([x.numpy()], w, nbins)
    xd = x.cuda()
    bh = torch.zeros(2 * nbins, dtype=torch.int32, device="cuda")
    dh = torch.zeros(2 * nbins, dtype=torch.int64, device="cuda")
    rec = torch.zeros(3 * 2 * 7, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.call("cn_chip_hist_u32", xd.data_ptr(), 2, bh.data_ptr(), 2, 2, 3 * 21 * 13, nbins, s)
    _lib.call("cn_hist_batch_reduce", bh.data_ptr(), dh.data_ptr(), torch.from_numpy(w).cuda().data_ptr(), rec.data_ptr(),
              2, 3, 2, nbins, s)
    assert torch.equal(dh.cpu().reshape(2, nbins), torch.from_numpy(want_hist))
    got = rec.cpu().reshape(3, 2, 7)
    assert torch.equal(got[2], torch.from_numpy(want_records[0])) and not got[:2].any() and not bh.any()
    clamped = np.clip(x.numpy().astype(np.int64), 0, nbins - 1)
    assert got[2, :, 3].tolist() == clamped.sum(axis=(0, 2, 3, 4)).tolist()
    assert got[2, :, 5].tolist() == (clamped ** 2).sum(axis=(0, 2, 3, 4)).tolist()


@pytest.mark.parametrize("centering", ["median", "mean"])
@pytest.mark.parametrize("name", ["small", "flat", "odd"])
def test_finish_meets_reference_and_restatement(golden, counted, name, centering):
    from cultionet_amd.normalize import stats_from_counts

    xs, ys, stats, counts = counted(name)
    nv = stats.finish(centering, 0.05, 0.95)
    C = xs[0].shape[1]
    got = {k: getattr(nv, f).reshape(-1).double().numpy() for k, f in
           (("std", "dataset_std"), ("mean", "dataset_mean"), ("lower_bound", "lower_bound"), ("upper_bound", "upper_bound"))}
    assert nv.num_channels == C and tuple(nv.dataset_mean.shape) == (1, C, 1, 1, 1) and nv.dataset_std.dtype == torch.float32
    # the reference's recorded outputs
    ref_std = golden[f"{name}_std"].astype(np.float64)
    q = golden[f"{name}_quantiles"].astype(np.float64)
    ref_mean = golden[f"{name}_mean"].astype(np.float64) if centering == "mean" else q[:, 1]
    nz = ref_std != 0
    dev = [np.max(np.abs(got["std"][nz] / ref_std[nz] - 1), initial=0.0), np.max(np.abs(got["mean"] - ref_mean)),
           np.max(np.abs(got["lower_bound"] - q[:, 0])), np.max(np.abs(got["upper_bound"] - q[:, 2]))]
    print(name, centering, "std rel", dev[0], "mean", dev[1], "lower", dev[2], "upper", dev[3])
    assert np.all(got["std"][~nz] == 0)
    assert dev[0] <= STD_RTOL and max(dev[1:]) <= ABS_TOL
    # the restatement, in float64 from the device's counts and in the float32 finish() stores
    want = R.dataset_stats([x.numpy() for x in xs], centering, 0.05, 0.95)
    f64 = stats_from_counts(*counts, CLASS_INFO, centering, 0.05, 0.95)
    for k in got:
        assert np.all(np.abs(f64[k] - want[k]) <= HOST_RTOL * np.abs(want[k])), k
        assert np.array_equal(got[k], f64[k].astype(np.float32).astype(np.float64)), k
    crop, edge = R.class_counts([y.numpy() for y in ys], **CLASS_INFO)
    assert torch.equal(nv.dataset_crop_counts, torch.from_numpy(crop))
    assert torch.equal(nv.dataset_edge_counts, torch.from_numpy(edge))


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.int16], ids=["i64", "u8", "i16"])
def test_label_counts(dtype):
    from cultionet_amd.data import Data
    from cultionet_amd.normalize import DatasetStats

    g = np.random.default_rng(11)
    values = [0, 1, 2, 3, 4, 200] if dtype == torch.uint8 else [-1, 0, 1, 2, 3, 4, 200]
    y = g.choice(np.array(values), (3, 37, 29))  # 3219 labels: a ragged last thread
    y[0, :20] = 3                                # long runs of one class, as label planes have them
    yt = torch.from_numpy(y).to(dtype)
    stats = DatasetStats(1, CLASS_INFO, "cuda")
    x = torch.zeros((3, 1, 1, 37, 29), dtype=torch.int16, device="cuda")
    stats.add(Data(x=x, y=yt.cuda()))
    stats.add(Data(x=x, y=yt.cuda()))
    _, _, labels = stats.counts()
    assert torch.equal(torch.from_numpy(labels), torch.from_numpy(2 * R.label_counts([y], NLAB)))
    nv = stats.finish()
    crop, edge = R.class_counts([y, y], **CLASS_INFO)
    assert torch.equal(nv.dataset_crop_counts, torch.from_numpy(crop))
    assert torch.equal(nv.dataset_edge_counts, torch.from_numpy(edge))


def test_errors():
    from cultionet_amd import _lib
    from cultionet_amd.data import Data
    from cultionet_amd.normalize import DatasetStats

    stats = DatasetStats(2, CLASS_INFO, "cuda")
    with pytest.raises(TypeError):
        stats.add(Data(x=torch.zeros((1, 2, 1, 4, 4), device="cuda")))
    with pytest.raises(ValueError):
        stats.add(Data(x=torch.zeros((1, 3, 1, 4, 4), dtype=torch.int16, device="cuda")))
    with pytest.raises(ValueError):
        DatasetStats(2, {"max_crop_class": 1, "edge_class": 3}, "cuda")
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    x = torch.zeros(64, dtype=torch.int16, device="cuda")
    h = torch.zeros(16385, dtype=torch.int64, device="cuda")
    for nbins in (1, 16385):
        assert lib.cn_chip_hist_u32(x.data_ptr(), 2, h.data_ptr(), 1, 1, 64, nbins, s) == -1
        assert lib.cn_hist_batch_reduce(h.data_ptr(), h.data_ptr(), h.data_ptr(), h.data_ptr(), 0, 1, 1, nbins, s) == -1
    assert lib.cn_chip_hist_u32(x.data_ptr(), 0, h.data_ptr(), 1, 1, 32, 100, s) == -1          # f32
    assert lib.cn_chip_hist_u32(x.data_ptr(), 2, h.data_ptr(), 2 ** 16, 1, 2 ** 16, 100, s) == -1  # B * L = 2^32
    for index in (4, 5, -1):  # a table of four records
        assert lib.cn_hist_batch_reduce(h.data_ptr(), h.data_ptr(), h.data_ptr(), h.data_ptr(), index, 4, 1, 100, s) == -1
    assert lib.cn_label_counts_i64(x.data_ptr(), 2, 64, h.data_ptr(), 0, s) == -1
    assert lib.cn_label_counts_i64(x.data_ptr(), 2, 64, h.data_ptr(), 1023, s) == -1
    torch.cuda.synchronize()
    assert not h.any()  # nothing was launched


def test_from_batches_equals_add_in_order():
    from cultionet_amd.data import Data
    from cultionet_amd.feeder import pin_batch
    from cultionet_amd.normalize import NormValues

    xs = [torch.from_numpy(smooth_i16((b, 3, 3, 16, 15), 20 + b)) for b in (2, 1, 3, 2)]
    ys = [torch.from_numpy(y) for y in labels_for([x.numpy() for x in xs], seed=6)]
    host = [pin_batch(Data(x=x, y=y)) for x, y in zip(xs, ys)]
    assert all(b.x.is_pinned() for b in host)
    nv = NormValues.from_batches(host, "cuda", CLASS_INFO, centering="mean")
    stats, _ = count(xs, ys)
    want = stats.finish("mean")
    for k, v in want.data_dict.items():
        w = nv.data_dict[k]
        assert torch.equal(v, w) if isinstance(v, torch.Tensor) else v == w, k
    reordered = NormValues.from_batches(host[::-1], "cuda", CLASS_INFO, centering="mean")
    assert torch.equal(reordered.dataset_mean, nv.dataset_mean)  # the histogram does not depend on order ...
    assert not torch.equal(reordered.dataset_std, nv.dataset_std)  # ... upstream's std estimator does


def test_prepare_chips_centres_the_small_case(golden, counted):
    from cultionet_amd.edges import prepare_chips

    xs, _, stats, _ = counted("small")
    nv = stats.finish()
    x = torch.cat(xs).cuda()
    z = prepare_chips(x, nv.dataset_mean, nv.dataset_std)
    torch.cuda.synchronize()
    z = z.cpu().double().numpy()
    std = nv.dataset_std.reshape(-1).double().numpy()
    for c in range(3):
        med = np.median(z[:, c])  # 12288 values: the mean of the two middle ones, as the 0.5 quantile is
        print("channel", c, "median", med, "bound", 4 * 6e-8 / std[c])
        assert abs(med) <= 4 * 6e-8 / std[c]
