"""Dataset normalization statistics, counted on the device (NormValues.from_dataset, utils/normalize.py:118-213).

The reference runs every training batch through ``Variance(method='median')`` and ``Quantile(r=6144)``
(utils/stats.py:236-683) on the CPU before the first step. Here the raw integer batches are counted where the feed path
already has them: stored reflectances pass through ``(x / 10000).clip(1e-9, 1)`` (data/datasets.py:443), so a channel
takes at most 10001 distinct values and a per-channel histogram over ``bin = clamp(v, 0, 10000)`` holds everything
``from_dataset`` reads.

  * ``DatasetStats.add`` enqueues three launches per batch (``cn_chip_hist_u32``, ``cn_hist_batch_reduce``,
    ``cn_label_counts_i64``) and never synchronises; everything the device writes is an integer.
  * ``DatasetStats.finish`` copies the counts once and does all floating-point arithmetic on the host, in float64
    (``stats_from_counts``, which needs no GPU).

What comes out: ``dataset_std`` replays the reference's estimator batch by batch (per-batch lower median, centred second
moment, its Chan-style update), so like upstream's it depends on how the dataset is cut into batches and on their order.
Quantiles follow the sketch's definition at the point where the sketch still holds every sample (sorted samples at
cumulative weights (i - 0.5) / n between the minimum at 0 and the maximum at 1); above 12288 rows the reference's own
quantiles are a randomized approximation of these. The value of bin k is ``float32(clip(k / 10000, 1e-9, 1))``, the
reference's own fp32 value, widened to float64.

``log_transform=True`` (the reference's ``--log-transform``: the statistics dataset is built with it too,
scripts/cultionet.py:630-721) changes the VALUE of a bin and nothing on the device: EdgeDataset.get feeds
``log(x * 50 + 1).clamp_min(1e-9)`` of the clipped value (data/datasets.py:481-484), a strictly increasing map of the bins
above 0, so the histograms, the per-batch lower-median bins and the quantile bins are the same, and
``cn_hist_batch_reduce`` takes its weights as a table. The caller says so where the counts are made (``DatasetStats``,
``from_batches``) and where they are read (``stats_from_counts``, ``from_counts``); a ``.norm`` file gains no key.
"""
from __future__ import annotations

import typing as T
from fractions import Fraction

import numpy as np
import torch

from .data import Data

NBINS = 10_001           # bins 0..10000 of clamp(v, 0, 10000)
REC_WORDS = 7            # int64 words of one (batch, channel) record of cn_hist_batch_reduce
WEIGHT_SHIFT = 37        # every fp32 value in [1e-4, 1] is a multiple of 2^-37
LOG_WEIGHT_SHIFT = 31    # every log-domain value of a bin k >= 1, in [0.004987, 3.931826], is a multiple of 2^-31
RECORD_CHUNK = 256       # batches per device record table
_XDTYPES = {torch.int32: 1, torch.int16: 2, torch.uint16: 3}
_YDTYPES = {torch.int32: 1, torch.int16: 2, torch.uint16: 3, torch.int64: 4}


def weight_shift(log_transform: bool = False) -> int:
    return LOG_WEIGHT_SHIFT if log_transform else WEIGHT_SHIFT


def bin_values(log_transform: bool = False) -> np.ndarray:
    """float64 [NBINS]: what EdgeDataset.get makes of a stored k, in fp32 as the reference holds it (datasets.py:443);
    with ``log_transform`` its torch.log(x * 50.0 + 1.0).clamp_min(1e-9) of that (datasets.py:481-484), computed by torch
    itself in fp32. Bin 0 is 1e-9 in both domains."""
    k = np.arange(NBINS, dtype=np.float32)
    v = np.clip(k / np.float32(10000.0), np.float32(1e-9), np.float32(1.0))
    if log_transform:
        v = torch.log(torch.from_numpy(v) * 50.0 + 1.0).clamp_min(1e-9).numpy()
    return v.astype(np.float64)


def bin_weights(log_transform: bool = False) -> np.ndarray:
    """int64 [NBINS]: bin_values() * 2^37 (2^31 in the log domain), exact for k >= 1; bin 0 (1e-9, no such multiple) has
    weight 0 and is carried by its own count in the record."""
    v, shift = bin_values(log_transform), weight_shift(log_transform)
    w = np.round(v * 2.0 ** shift).astype(np.int64)
    assert np.array_equal(w[1:].astype(np.float64) * 2.0 ** -shift, v[1:]) and w.max() < 2 ** 40
    w[0] = 0
    return w


def _check_classes(class_info: T.Dict[str, int]) -> T.Tuple[int, int]:
    max_crop, edge = int(class_info["max_crop_class"]), int(class_info["edge_class"])
    if edge < 0 or max_crop < 0:
        raise ValueError("class_info: max_crop_class and edge_class must not be negative")
    if edge - 1 > max_crop:  # normalize.py:183-184 would index crop_counts past its end
        raise ValueError(f"edge_class - 1 = {edge - 1} is beyond max_crop_class = {max_crop}")
    return max_crop, edge


def _replay_variance(records: np.ndarray, values: np.ndarray, shift: int = WEIGHT_SHIFT) -> float:
    """Variance(method='median').add over one channel's records in order, then .std() (stats.py:642-683)."""
    v0 = Fraction(float(values[0]))
    count, mean, cmom2 = 0, None, 0.0
    for n, h0, mbin, s1lo, s1hi, s2lo, s2hi in records.tolist():
        if n == 0:
            continue
        s1 = (s1hi << 64) | (s1lo & 0xFFFFFFFFFFFFFFFF)
        s2 = (s2hi << 64) | (s2lo & 0xFFFFFFFFFFFFFFFF)
        m = Fraction(float(values[mbin]))
        # sum_{k>=1} h_k (val_k - m)^2 + h_0 (1e-9 - m)^2, exactly, rounded once
        centred = (Fraction(s2, 1 << (2 * shift)) - 2 * m * Fraction(s1, 1 << shift) + (n - h0) * m * m
                   + h0 * (v0 - m) ** 2)
        centred, m = float(centred), float(values[mbin])
        if mean is None:
            count, mean, cmom2 = n, m, centred
            continue
        oldcount = count
        count += n
        new_frac = float(n) / count
        delta = (m - mean) * new_frac
        mean += delta
        cmom2 += centred
        cmom2 += delta * delta * (new_frac * oldcount)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.sqrt(np.float64(cmom2) / np.float64(count - 1)))


def _hist_quantile(hist: np.ndarray, cum: np.ndarray, values: np.ndarray, q: float) -> float:
    """Quantile.quantiles(q) (stats.py:519-575) while the sketch holds every sample: np.interp over the sorted samples
    s_1..s_n at (i - 0.5) / n, the minimum at 0 and the maximum at 1. q is rounded to fp32 as torch.tensor(q) does."""
    n = int(cum[-1])
    if n == 0:
        return float("nan")
    q = float(np.float32(q))

    def sample(i):  # s_i, 1 <= i <= n
        return float(values[int(np.searchsorted(cum, i, side="left"))])

    i = int(np.floor(q * n + 0.5))  # s_i is the last sample at or below q
    if i <= 0:
        return sample(1)
    if i >= n:
        return sample(n)
    lo, hi = sample(i), sample(i + 1)
    x_lo, x_hi = (i - 0.5) / n, (i + 0.5) / n
    return lo + (hi - lo) * ((q - x_lo) / (x_hi - x_lo))


def stats_from_counts(records: np.ndarray, hist: np.ndarray, label_counts: np.ndarray, class_info: T.Dict[str, int],
                      centering: str = "median", lower_quantile: float = 0.05, upper_quantile: float = 0.95,
                      log_transform: bool = False) -> T.Dict[str, np.ndarray]:
    """The host half of DatasetStats.finish, float64 throughout; runs without a GPU.

    records: int64 [batches, C, 7] as cn_hist_batch_reduce writes them with bin_weights(log_transform), the same flag as
    here; hist: [C, NBINS] counts of the whole dataset; label_counts: int64 [edge_class + 3] = {y < 0, y == 0, ...,
    y == edge_class, y > edge_class}.
    """
    max_crop, edge = _check_classes(class_info)
    records = np.asarray(records, dtype=np.int64).reshape(-1, hist.shape[0], REC_WORDS)
    hist = np.asarray(hist).astype(np.int64)
    values, shift = bin_values(log_transform), weight_shift(log_transform)
    C = hist.shape[0]
    out = {k: np.zeros(C) for k in ("std", "mean", "lower_bound", "upper_bound")}
    for c in range(C):
        cum = np.cumsum(hist[c])
        out["std"][c] = _replay_variance(records[:, c], values, shift)
        if centering == "mean":  # Quantile.mean(), stats.py:455-456
            out["mean"][c] = float(np.dot(hist[c].astype(np.float64), values) / cum[-1]) if cum[-1] else float("nan")
        else:                    # Quantile.median()
            out["mean"][c] = _hist_quantile(hist[c], cum, values, 0.5)
        out["lower_bound"][c] = _hist_quantile(hist[c], cum, values, lower_quantile)
        out["upper_bound"][c] = _hist_quantile(hist[c], cum, values, upper_quantile)
    # normalize.py:180-191, literally
    lc = np.asarray(label_counts, dtype=np.int64)
    below, of = int(lc[0]), lc[1:edge + 2]
    crop = np.zeros(max_crop + 1, dtype=np.int64)
    crop[0] += of[0] + (of[edge] if edge != 0 else 0)      # (y == 0) | (y == edge_class)
    for i in range(1, edge):
        crop[i] += of[i]
    edges = np.zeros(2, dtype=np.int64)
    edges[0] = int(lc.sum()) - below - int(of[edge])        # (y >= 0) & (y != edge_class)
    edges[1] = of[edge]
    out["crop_counts"], out["edge_counts"] = crop, edges
    return out


def _c5(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).float().reshape(1, -1, 1, 1, 1)


class NormValues:
    """Normalization values: the fields, shapes and file format of the reference's class (utils/normalize.py:26-116)."""

    def __init__(self, dataset_mean: torch.Tensor, dataset_std: torch.Tensor, dataset_crop_counts: torch.Tensor,
                 dataset_edge_counts: torch.Tensor, num_channels: int, lower_bound: T.Optional[torch.Tensor] = None,
                 upper_bound: T.Optional[torch.Tensor] = None):
        self.dataset_mean = dataset_mean
        self.dataset_std = dataset_std
        self.dataset_crop_counts = dataset_crop_counts
        self.dataset_edge_counts = dataset_edge_counts
        self.num_channels = num_channels
        self.lower_bound = lower_bound
        self.upper_bound = upper_bound

    def __repr__(self):
        return "NormValues(" + ", ".join(f"{k}={v}" for k, v in self.data_dict.items()) + ")"

    def __call__(self, batch: Data) -> Data:
        return self.transform(batch)

    def transform(self, batch: Data) -> Data:
        """z = (x - mean) / std on a copy of the batch."""
        out = batch.copy()
        out.x = (out.x - self.dataset_mean.to(device=out.x.device)) / self.dataset_std.to(device=out.x.device)
        return out

    def inverse_transform(self, batch: Data) -> Data:
        out = batch.copy()
        out.x = self.dataset_std.to(device=out.x.device) * out.x + self.dataset_mean.to(device=out.x.device)
        return out

    @property
    def data_dict(self) -> dict:
        return {
            "dataset_mean": self.dataset_mean,
            "dataset_std": self.dataset_std,
            "dataset_crop_counts": self.dataset_crop_counts,
            "dataset_edge_counts": self.dataset_edge_counts,
            "num_channels": self.num_channels,
            "lower_bound": self.lower_bound,
            "upper_bound": self.upper_bound,
        }

    def to_file(self, filename, compress: str = "zlib") -> None:
        import joblib

        joblib.dump(self.data_dict, filename, compress=compress)

    @classmethod
    def from_file(cls, filename) -> "NormValues":
        import joblib

        return cls(**joblib.load(filename))

    @classmethod
    def from_counts(cls, records, hist, label_counts, class_info, centering: str = "median",
                    lower_quantile: float = 0.05, upper_quantile: float = 0.95,
                    log_transform: bool = False) -> "NormValues":
        s = stats_from_counts(records, hist, label_counts, class_info, centering, lower_quantile, upper_quantile,
                              log_transform)
        return cls(dataset_mean=_c5(s["mean"]), dataset_std=_c5(s["std"]), lower_bound=_c5(s["lower_bound"]),
                   upper_bound=_c5(s["upper_bound"]), dataset_crop_counts=torch.from_numpy(s["crop_counts"]),
                   dataset_edge_counts=torch.from_numpy(s["edge_counts"]), num_channels=len(s["mean"]))

    @classmethod
    def from_batches(cls, host_batches: T.Iterable[Data], device: T.Union[str, torch.device],
                     class_info: T.Dict[str, int], centering: str = "median", lower_quantile: float = 0.05,
                     upper_quantile: float = 0.95, log_transform: bool = False) -> "NormValues":
        """from_dataset over raw host batches: batch i+1 is pinned and copied on a copy stream while batch i is counted on
        the current stream (the double buffering of DeviceFeeder.iterate). ``log_transform``: statistics of the values a
        dataset built with ``log_transform=True`` feeds (datasets.py:481-484), for ``DeviceFeeder(log_transform=True)``."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("NormValues.from_batches counts on a GPU; use stats_from_counts for host-side counts")
        copy_stream = torch.cuda.Stream(device=device)

        def stage(host):
            with torch.cuda.stream(copy_stream):
                kw = {}
                for k in ("x", "y"):
                    v = getattr(host, k, None)
                    if v is not None:
                        v = v if v.is_cuda or v.is_pinned() else v.pin_memory()
                        kw[k] = v.to(device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            return Data(**kw), ev

        stats = None
        it = iter(host_batches)
        try:
            nxt = stage(next(it))
        except StopIteration:
            raise ValueError("NormValues.from_batches needs at least one batch") from None
        with torch.cuda.device(device):
            while nxt is not None:
                batch, ev = nxt
                try:
                    nxt = stage(next(it))
                except StopIteration:
                    nxt = None
                cur = torch.cuda.current_stream(device)
                cur.wait_event(ev)
                for v in (batch.x, batch.y):
                    if v is not None:
                        v.record_stream(cur)
                if stats is None:
                    stats = DatasetStats(batch.x.shape[1], class_info, device, log_transform=log_transform)
                stats.add(batch)
            return stats.finish(centering, lower_quantile, upper_quantile)


class DatasetStats:
    """Streaming counts of raw device batches; ``add`` and ``finish`` work on the current stream."""

    def __init__(self, num_channels: int, class_info: T.Dict[str, int], device: T.Union[str, torch.device],
                 record_chunk: int = RECORD_CHUNK, log_transform: bool = False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("DatasetStats counts on a GPU (there is no CPU path; see stats_from_counts)")
        self.class_info = dict(class_info)
        self.log_transform = bool(log_transform)  # decides the weights of the records, so it is fixed here
        _, edge = _check_classes(class_info)
        self.num_channels, self.nlab, self.chunk = int(num_channels), edge + 1, int(record_chunk)
        C = self.num_channels
        # one int64 buffer, so that finish() is one copy: dataset histogram | label counts | record table
        sizes = (C * NBINS, self.nlab + 2, self.chunk * C * REC_WORDS)
        self._buf = torch.zeros(sum(sizes), dtype=torch.int64, device=self.device)
        self._hist, self._labels, self._records = self._buf.split(sizes)
        self._batch_hist = torch.zeros(C * NBINS, dtype=torch.int32, device=self.device)  # uint32 words
        self._weights = torch.from_numpy(bin_weights(self.log_transform)).to(self.device)
        self._filled = 0                             # records in the device table
        self._host_records: T.List[np.ndarray] = []  # full chunks, already on the host

    def add(self, batch: Data) -> None:
        from . import _lib
        from .engine import _stream

        x, y = batch.x, getattr(batch, "y", None)
        if x.dtype not in _XDTYPES:
            raise TypeError(f"DatasetStats counts raw integer reflectances (int32, int16, uint16), not {x.dtype}")
        if x.dim() != 5 or x.shape[1] != self.num_channels:
            raise ValueError(f"x must be [B, {self.num_channels}, T, H, W], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("DatasetStats.add needs a device batch")
        C = self.num_channels
        if self._filled == self.chunk:  # the one copy a full chunk costs
            self._host_records.append(self._records.cpu().numpy().reshape(self.chunk, C, REC_WORDS))
            self._filled = 0
        x = x.contiguous()
        stream = _stream()
        _lib.call("cn_chip_hist_u32", x.data_ptr(), _XDTYPES[x.dtype], self._batch_hist.data_ptr(), x.shape[0], C,
                  int(x[0, 0].numel()), NBINS, stream)
        _lib.call("cn_hist_batch_reduce", self._batch_hist.data_ptr(), self._hist.data_ptr(), self._weights.data_ptr(),
                  self._records.data_ptr(), self._filled, self.chunk, C, NBINS, stream)
        self._filled += 1
        if y is not None:
            y = (y if y.dtype in _YDTYPES else y.long()).contiguous()
            _lib.call("cn_label_counts_i64", y.data_ptr(), _YDTYPES[y.dtype], y.numel(), self._labels.data_ptr(),
                      self.nlab, stream)

    def counts(self) -> T.Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(records [batches, C, 7], dataset histogram [C, NBINS], label counts) on the host: one copy."""
        C = self.num_channels
        used = C * NBINS + self.nlab + 2 + self._filled * C * REC_WORDS
        host = self._buf[:used].cpu().numpy()
        hist, labels, rec = np.split(host, [C * NBINS, C * NBINS + self.nlab + 2])
        records = np.concatenate(self._host_records + [rec.reshape(self._filled, C, REC_WORDS)])
        return records, hist.reshape(C, NBINS), labels

    def finish(self, centering: str = "median", lower_quantile: float = 0.05, upper_quantile: float = 0.95,
               log_transform: T.Optional[bool] = None) -> NormValues:
        """``log_transform`` defaults to the constructor's; another value is refused, since the records were summed with
        that domain's weights."""
        if log_transform is not None and bool(log_transform) != self.log_transform:
            raise ValueError(f"these counts were made with log_transform={self.log_transform}")
        records, hist, labels = self.counts()
        return NormValues.from_counts(records, hist, labels, self.class_info, centering, lower_quantile, upper_quantile,
                                      self.log_transform)
