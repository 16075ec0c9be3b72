"""Scratch layer of the engine: every persistent scratch buffer -- the deferred weight-gradient slice sums with their
arena, and the grow-or-reuse pools of the weight-gradient, PreTimeReduction and BatchNorm kernels.

Layer order runtime -> params -> scratch -> tape -> engine: this module imports from ``runtime`` and ``params``.
"""
from __future__ import annotations

import os
import struct
import typing as T

import torch

from . import _lib, runtime
from .params import _bump_ws_epoch
from .runtime import _main_stream, _py_op, _side_state, _state, _stream


# ---------------------------------------------------------------------------
# deferred weight-gradient slice sums (csrc/cn_slicesum.h)
# ---------------------------------------------------------------------------
# A many-split weight gradient leaves partial dW slices in scratch; `dW += sum(slices)` is needed by the optimizer (or by
# the gradient bucket's all-reduce), not by the next backward node. During a backward pass the library appends those
# sums to a table instead of launching them (34 fp32 / 68 bf16 dependent launches per step), and ONE batched launch per
# flush -- per ready bucket under data parallelism, else one per step -- adds them all. Since the slices must survive
# until then, every weight-gradient call of the pass takes its scratch from an arena that only moves forward.
# CN_DEFER_SUMS=0: the sums run right behind their contraction as in rounds 1-4.
_DEFER_SUMS = os.environ.get("CN_DEFER_SUMS", "1") != "0"
_SS_CAP = 512            # records per backward pass (64 bytes each)
_SS_BLOCK = 64 << 20     # floats per arena block (256 MB)
# Pending slices are summed as soon as this many floats are waiting (CN_SUM_FLUSH_MB, default 128 MB): they are then
# still in the 256 MB Infinity Cache, and the pass does not end with ONE 0.6 GB reduction behind the last weight gradient
# on the stream that finishes last (fp32, same box: all-at-the-end 386.4 chips/s against 387.5 with the 34 immediate
# sums). 0 = only the final flush.
_SS_FLUSH_FLOATS = int(float(os.environ.get("CN_SUM_FLUSH_MB", "128")) * (1 << 20) / 4)


class _SliceSums:
    """Per-device state of the deferred sums: pinned host table the library writes, its device copy, the arena."""

    def __init__(self, dev: torch.device):
        self.dev = dev
        self.host = torch.zeros(_SS_CAP * 64, dtype=torch.uint8).pin_memory()
        self.table = torch.zeros(_SS_CAP * 64, dtype=torch.uint8, device=dev)
        self.uploaded: T.Dict[T.Tuple[int, int], bytes] = {}  # record range -> bytes the device copy holds for it
        self.upload_ev = torch.cuda.Event()                    # (re-)recorded behind every table upload
        self.writer: T.Any = None    # the launch plan that rewrote the host table last (None: an eager pass)
        self.blocks: T.List[torch.Tensor] = []
        self.active = False
        self.reset()

    def reset(self) -> None:
        self.cur, self.off, self.seen, self.flushed, self.pending = 0, 0, 0, 0, 0

    def _commit(self) -> None:
        """Move the arena past the slices of the records appended since the last call (a call whose sum was not
        deferred leaves nothing behind: its scratch is reused by the next call, as stream order allows)."""
        n = _lib.query("cn_slice_sums_count")
        if n <= self.seen or not self.blocks:
            return
        raw = bytes(self.host[self.seen * 64:n * 64].numpy())
        base = self.blocks[self.cur].data_ptr()
        for i in range(n - self.seen):
            part, _dw, stride, _n, nslices = struct.unpack_from("<QQqqi", raw, i * 64)
            end = (part - base) // 4 + stride * nslices
            if 0 <= end <= self.blocks[self.cur].numel():
                self.off = max(self.off, (end + 63) // 64 * 64)
            self.pending += stride * nslices
        self.seen = n

    def take(self, need: int) -> T.Tuple[int, int]:
        self._commit()
        if 0 < _SS_FLUSH_FLOATS <= self.pending:
            flush_slice_sums()
        need = int(need)
        while True:
            if self.cur >= len(self.blocks):
                # (no workspace-epoch bump: a block that is ADDED moves nothing a recorded plan points at)
                self.blocks.append(torch.empty(max(_SS_BLOCK, need), dtype=torch.float32, device=self.dev))
            blk = self.blocks[self.cur]
            if blk.numel() - self.off >= need:
                return blk.data_ptr() + 4 * self.off, need
            if self.off == 0:  # an oversized request in front of a standard block
                torch.cuda.synchronize(self.dev)
                self.blocks[self.cur] = torch.empty(need, dtype=torch.float32, device=self.dev)
                _bump_ws_epoch()
                continue
            self.cur, self.off = self.cur + 1, 0


def _ss_state() -> T.Optional[_SliceSums]:
    """The active deferral state of this thread (None: sums run immediately)."""
    return _state.slice_sums


def _sum_stream() -> int:
    """Handle of the stream every weight gradient of the pass runs on (the side stream, or the compute stream when the
    overlap is off): the batched sums are stream-ordered behind the contractions that wrote their slices."""
    if runtime._OVERLAP_WGRAD:
        return _side_state(_main_stream().device)["stream"].cuda_stream
    return _stream()


class deferring_slice_sums:
    """Context manager around one backward pass: weight-gradient slice sums into ``store.flat_grad`` are collected and
    run by flush_slice_sums() (called on exit, and by the data-parallel bucket logic before a bucket is reduced)."""

    def __init__(self, store: "ParamStore"):
        self.store = store
        self.on = False

    def __enter__(self):
        if not _DEFER_SUMS or _ss_state() is not None or not self.store.flat_grad.is_cuda:
            return self
        # One state PER STORE (tables, arena): a launch plan recorded for one trainer bakes these addresses in, and a
        # second trainer of the process (tests run an eager and a replayed one side by side) must not rewrite them.
        st = getattr(self.store, "_slice_sums", None)
        if st is None:
            st = self.store._slice_sums = _SliceSums(self.store.flat_grad.device)
        if st.active:  # a pass over this store is already collecting (another thread): that one keeps the arena
            return self
        st.reset()
        st.active = True
        # the library is about to rewrite the host table: an upload still in flight (enqueued by the previous eager pass,
        # or by a replayed plan, which re-records the event) must have read it first
        if not st.upload_ev.query():
            st.upload_ev.synchronize()
        if runtime._recorder is None:
            st.writer = None
        _state.slice_sums = st
        _lib.call("cn_slice_sums_begin", st.host.data_ptr(), _SS_CAP, self.store.flat_grad.data_ptr(),
                  self.store.numel)
        self.on = True
        return self

    def __exit__(self, *exc):
        if self.on:
            try:
                if exc[0] is None:
                    flush_slice_sums()
            finally:
                _lib.call("cn_slice_sums_end")
                _state.slice_sums.active = False
                _state.slice_sums = None
        return False


def flush_slice_sums() -> None:
    """ONE launch adding every pending slice sum into the flat gradient, on the weight gradients' stream."""
    st = _ss_state()
    if st is None:
        return
    st._commit()
    n = _lib.query("cn_slice_sums_count")
    first = st.flushed
    if n <= first:
        return
    now = st.host.numpy().reshape(-1, 64)[first:n, :60].tobytes()  # (without the block dealing the run call writes)
    # a recorded plan always refreshes the device copy: eager steps in between (other shapes) may have changed it
    upload = 0 if (st.uploaded.get((first, n)) == now and runtime._recorder is None) else 1
    sobj = _side_state(st.dev)["stream"] if runtime._OVERLAP_WGRAD else _main_stream()
    stream = _sum_stream()
    _lib.call("cn_slice_sums_run", st.host.data_ptr(), st.table.data_ptr(), first, n - first, upload, stream)
    if upload:  # the device copy of every overlapping range is no longer what `uploaded` says
        for k in [k for k in st.uploaded if k[0] < n and first < k[1]]:
            del st.uploaded[k]
        st.uploaded[(first, n)] = now
        _py_op(st.upload_ev.record, sobj)  # (a plan entry too: the next eager pass waits for a replay's upload)
    st.pending = 0
    st.flushed = n
    # every slice handed out so far has been consumed by a launch that is now enqueued on the weight gradients' stream,
    # and whatever takes scratch next runs behind it on the same stream: the arena starts over (it used to
    # grow to the whole pass's slices, ~0.6 GB per fp32 step, and never shrank)
    st.cur, st.off = 0, 0


# ---------------------------------------------------------------------------
# persistent scratch pools: one buffer per key, replaced by a larger one when a caller needs more
# ---------------------------------------------------------------------------

def _zeroed_scratch(n: int, dev: torch.device) -> torch.Tensor:
    """A scratch buffer whose ticket-counter head must be zero before its first launch, zeroed ON THE STREAM THAT WILL
    USE IT. ``torch.zeros`` fills on torch's current (compute) stream, but these buffers are keyed to the
    weight-gradient side stream or an auxiliary stream, which had only waited for an event recorded BEFORE the
    allocation: the fill raced the first ticketed kernel. ``cn_fill_f32`` on ``_stream()`` is ordered by construction;
    a recycled block is safe because that stream already waits for everything the compute stream enqueued earlier."""
    ws = torch.empty(n, dtype=torch.float32, device=dev)
    _lib.call("cn_fill_f32", ws.data_ptr(), n, 0.0, _stream())
    return ws


def _grown(pool: T.Dict, key, need: int, dev: torch.device, zeroed: bool) -> torch.Tensor:
    """``pool[key]`` with room for ``need`` floats: the buffer that is there, or a new one (zero-filled through
    _zeroed_scratch when ``zeroed``) that replaces it. Every (re)allocation bumps the workspace epoch."""
    ws = pool.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:  # growing: the old buffer may still be in use by launches in flight on any stream
            torch.cuda.synchronize(dev)
        ws = pool[key] = _zeroed_scratch(need, dev) if zeroed else torch.empty(need, dtype=torch.float32, device=dev)
        _bump_ws_epoch()
    return ws


_WS_FLOATS = 16 << 20  # persistent weight-gradient scratch (64 MB): aligned operand copies + partial dW slices


def _pad_ws(*tensors: torch.Tensor) -> T.Tuple[T.Optional[int], int]:
    """(pointer, floats) of the weight-gradient scratch: room for aligned copies of odd-sized operands plus the
    partial-dW slices of many-split launches. One persistent buffer per device (launches are stream-ordered)."""
    need = _WS_FLOATS
    for t in tensors:
        H, W = t.shape[-2], t.shape[-1]
        if (H * W) % 4 or (W & 1):
            need += t.shape[0] * t.shape[1] * (H * (W + 1) + 3)
    dev = tensors[0].device
    ss = _ss_state()
    if ss is not None:  # deferred slice sums: this call's slices must outlive the next call
        return ss.take(need)
    pool = _state.ws_pool
    if pool is None:
        pool = _state.ws_pool = {}
    ws = _grown(pool, dev, need, dev, zeroed=False)
    return ws.data_ptr(), ws.numel()


_pt_ws: T.Dict[T.Tuple, torch.Tensor] = {}


def _pretime_ws(need: int, dev: torch.device) -> torch.Tensor:
    """Scratch of the fused PreTimeReduction calls, one per (device, stream): zero-filled once (ticket counters at its
    head; every launch leaves them zero)."""
    return _grown(_pt_ws, (dev, _stream()), need, dev, zeroed=True)


_WS16_MAX_FLOATS = 96 << 20  # cap of the weight-gradient scratch (384 MB); the pixel split shrinks to fit


def _ws16(need: int, dev: torch.device, pool_name: str = "wgrad") -> T.Tuple[int, int]:
    """(pointer, floats) of a persistent fp32 scratch of the bf16 kernels. One buffer per (device, purpose): the
    weight-gradient slices live on the side stream, BatchNorm partial sums on the main stream."""
    need = int(min(max(need, 1 << 20), _WS16_MAX_FLOATS))
    if pool_name == "wgrad":
        ss = _ss_state()
        if ss is not None:  # deferred slice sums: this call's slices must outlive the next call
            return ss.take(need)
    pool = _state.ws16_pool
    if pool is None:
        pool = _state.ws16_pool = {}
    # ("wgrad" / "side" live on the ONE weight-gradient stream; every other pool belongs to the stream that launches)
    key = (dev, pool_name) if pool_name in ("wgrad", "side") else (dev, pool_name, _state.stream_override)
    # zero-filled: the single-launch reductions keep their ticket counters in the first words of these buffers
    # (zero on entry, left zero on exit)
    ws = _grown(pool, key, need, dev, zeroed=True)
    return ws.data_ptr(), ws.numel()


def _bn_ws16(C: int, dev: torch.device, pool_name: str = "bn") -> int:
    return _ws16(_lib.query("cn_bn_workspace_floats_bf16", C), dev, pool_name)[0]


_bng_ws: T.Dict[T.Tuple, torch.Tensor] = {}


def _bn_group_ws16(G: int, C: int, dev: torch.device) -> int:
    """Scratch of the grouped BatchNorm calls on the COMPUTE stream (launches are stream-ordered): ticket counters
    (zeroed ONCE here; every launch leaves them zero), finalize slices, backward coefficients, partial rows."""
    need = int(_lib.query("cn_bn_group_workspace_floats_bf16", G, C))
    # (at least 1M floats: a buffer that is there is never smaller, so it is replaced exactly when it is below ``need``)
    return _grown(_bng_ws, (dev, _stream()), max(need, 1 << 20), dev, zeroed=True).data_ptr()
