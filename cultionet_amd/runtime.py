"""Runtime layer of the engine: per-thread state, stream selection, the weight-gradient side stream and the auxiliary
stream, the allocator, and the layout predicates every op uses.

Bottom of the layer order runtime -> params -> scratch -> tape -> engine: it imports ``torch`` and ``_lib`` only.
``_OVERLAP_WGRAD`` and ``_recorder`` are rebound at run time; other modules read them as ``runtime.<name>``.
"""
from __future__ import annotations

import ctypes
import os
import threading
import typing as T

import torch

from . import _lib


class _ThreadState(threading.local):
    """Everything the engine keeps per thread. The class attributes are what a fresh thread sees; fields that hold a
    list or dict are created by their first user, so threads never share one."""

    main_stream = None          # torch's current stream, cached by using_store for its scope
    main_handle = None          # ... and its HIP handle
    stream_override = None      # handle launches go to instead (inside side_stream / a spawn() branch)
    stream_obj_override = None  # ... and its torch stream object
    bf16 = False                # mixed_precision(): the model body runs in bf16 NHWC
    branch = None               # the _Branch whose sub-graph is being recorded by spawn()
    no_branches = False         # branch_streams(False): spawn() runs inline
    alloc_sinks = None          # lists that _alloc() files every buffer in (holding_allocations)
    keepalive = None            # the _KeepAlive deferring frees while branches are open
    open_branches = None        # branches whose backward is in flight (between bwd_join and bwd_fork)
    tape = None                 # the current Tape (recording)
    store = None                # the active ParamStore (using_store)
    slice_sums = None           # the _SliceSums collecting this thread's backward pass
    ws_pool = None              # device -> fp32 weight-gradient scratch (_pad_ws)
    ws16_pool = None            # (device, purpose[, stream]) -> scratch of the bf16 kernels (_ws16)


_state = _ThreadState()


# ---- launch-plan recording (cultionet_amd/replay.py) ----------------------------------------------------------------
# While a plan is being recorded, every stream / event operation and every host-side torch call that launches work is
# routed through _py_op so that the plan can repeat it; C-ABI calls are captured by a recording _lib.call.
_recorder: T.Optional[T.List] = None


def _py_op(fn: T.Callable, *args) -> None:
    """Run ``fn(*args)`` now and, while a launch plan is being recorded, append it to the plan."""
    fn(*args)
    if _recorder is not None:
        _recorder.append((1, fn, args))


def _main_stream() -> "torch.cuda.Stream":
    """torch's current stream, looked up once per ``using_store`` scope (a forward, a backward or a whole native step:
    the stream cannot change inside one) -- ``torch.cuda.current_stream()`` costs ~11 us, and at ~420 launches per step
    that was a third of the host's enqueue time."""
    ms = _state.main_stream
    return ms if ms is not None else torch.cuda.current_stream()


def _stream() -> int:
    """HIP stream handle the next launch goes to: the side stream inside a ``side_stream`` block, else torch's
    current stream."""
    ov = _state.stream_override
    if ov is not None:
        return ov
    h = _state.main_handle
    return h if h is not None else torch.cuda.current_stream().cuda_stream


def _check(t: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError("cultionet_amd ops need device tensors (MI355X); there is no CPU fallback")
    if t.dtype == torch.bfloat16:
        # mixed-precision path: bf16 activations are NHWC (logical shape [B,C,H,W], channel stride 1)
        if t.dim() != 4 or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(3) % 8 or t.data_ptr() % 16:
            raise RuntimeError("bf16 activations must be NHWC views (channels innermost, 16-byte aligned slices)")
        return t
    if t.dtype != torch.float32:
        raise RuntimeError(f"fp32 (or bf16 NHWC) tensor expected, got {t.dtype}")
    return t


def is16(t: torch.Tensor) -> bool:
    return t.dtype == torch.bfloat16


def ld(t: torch.Tensor) -> int:
    """Pixel stride (elements) of a bf16 NHWC activation held as a logical [B,C,H,W] view."""
    return t.stride(3)


def _dense16(t: torch.Tensor) -> bool:
    """Pixels of all images form ONE run of rows with stride ld (kernels take P = B*H*W rows)."""
    B, _, H, W = t.shape
    l = t.stride(3)
    return (H == 1 or t.stride(2) == W * l) and (B == 1 or t.stride(0) == H * W * l)


class mixed_precision:
    """Context manager: run the TowerUNet body (encoder .. tower heads) in bf16 NHWC with fp32 accumulation,
    statistics and parameters -- the reference's precision="16-mixed" (model.py:168-186) on MI355X MFMA."""

    def __init__(self, enabled: bool = True):
        self.enabled = bool(enabled)

    def __enter__(self):
        self.prev = _state.bf16
        _state.bf16 = self.enabled
        return self

    def __exit__(self, *exc):
        _state.bf16 = self.prev
        return False


def bf16_enabled() -> bool:
    return bool(_state.bf16)


def bstride(t: torch.Tensor) -> int:
    """Batch stride of an NCHW(-like) buffer whose inner dims are dense."""
    return t.stride(0) if t.shape[0] > 1 else int(t[0].numel())


def _dense_inner(t: torch.Tensor) -> bool:
    exp = 1
    for d in range(t.dim() - 1, 0, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            return False
        exp *= t.shape[d]
    return True


def _rows(t: torch.Tensor) -> int:
    return t.shape[0] * t.shape[2] * t.shape[3]


# ---------------------------------------------------------------------------
# weight gradients on a side stream
# ---------------------------------------------------------------------------
# In backward only dx feeds the next node; dW (and bias gradients) are needed by the optimizer alone. Their launches
# go to a second HIP stream that waits for the node's dy, so the launch-shaped layers of the coarse levels (25x25,
# 13x13: a fraction of the 256 CUs each) run beside the dx chain instead of in front of it. The main stream joins
# the side stream once, before the gradient exchange / optimizer. CN_OVERLAP_WGRAD=0 keeps everything on one stream.
_OVERLAP_WGRAD = os.environ.get("CN_OVERLAP_WGRAD", "1") == "1"
_side_streams: T.Dict[T.Any, T.Dict[str, T.Any]] = {}


def overlap_wgrad(enabled: bool) -> bool:
    """Switch the weight-gradient side stream on / off at run time (bench.py's isolated per-kernel pass); returns the
    previous setting. Pending side-stream work is joined first."""
    global _OVERLAP_WGRAD
    prev = _OVERLAP_WGRAD
    join_side_stream()
    _OVERLAP_WGRAD = bool(enabled)
    return prev


def _priority_stream(dev, lowest: bool) -> "torch.cuda.Stream":
    """A stream at the LOWEST or the highest priority the device offers, created through the C ABI
    (torch.cuda.Stream can only ask for normal or higher) and wrapped as a torch ExternalStream for events /
    record_stream.
    Lowest: the weight-gradient stream. Its kernels (one wave per SIMD, hundreds of microseconds each) must not take CUs
    from the data-gradient chain on the compute stream, which is the critical path. (A normal-priority stream and a
    CU-masked one were measured against it and removed: DESIGN.md section 2.) Highest: the auxiliary stream
    (_aux_stream)."""
    handle = ctypes.c_void_p()
    rng = (ctypes.c_int * 2)()
    with torch.cuda.device(dev):
        _lib.call("cn_stream_priority_range", rng)
        _lib.call("cn_stream_create", int(rng[0 if lowest else 1]), None, 0, ctypes.byref(handle))
    return torch.cuda.ExternalStream(handle.value, device=dev)


def _side_state(dev) -> T.Dict[str, T.Any]:
    st = _side_streams.get(dev)
    if st is None:
        st = {"stream": _priority_stream(dev, lowest=True), "event": torch.cuda.Event(), "dirty": False}
        _side_streams[dev] = st
    return st


class side_stream:
    """Context manager: enqueue the enclosed launches on the side stream, ordered after everything enqueued so far on
    the current stream. ``tensors`` are the buffers those launches read (kept from being recycled by the caching
    allocator until the side stream has passed them)."""

    def __init__(self, *tensors: torch.Tensor):
        self.tensors = tensors
        self.ctx = None

    def __enter__(self):
        if not _OVERLAP_WGRAD:
            return self
        main = _main_stream()
        st = _side_state(main.device)
        cur = _state.stream_obj_override or main  # (inside spawn(): the branch's stream)
        if cur is main:
            _py_op(st["event"].record, main)
            _py_op(st["stream"].wait_event, st["event"])
        else:  # a fresh event: st["event"] may still be pending on the compute stream's behalf
            ev = torch.cuda.Event()
            _py_op(ev.record, cur)
            _py_op(st["stream"].wait_event, ev)
        st["dirty"] = True
        self.st = st
        self.prev = (_state.stream_override, _state.stream_obj_override)
        # launches go through the C ABI with an explicit stream handle: redirect _stream() instead of switching torch's
        # current stream (a torch.cuda.stream() context costs ~15 us of host time per layer). torch allocations made
        # inside the block still belong to the main stream: nothing inside may rely on a torch op (fills go through
        # cn_fill_f32 on the side stream).
        self.ctx = True
        _state.stream_override = st["stream"].cuda_stream
        _state.stream_obj_override = st["stream"]
        return self

    def __exit__(self, *exc):
        if self.ctx is not None:
            _state.stream_override, _state.stream_obj_override = self.prev
            for t in self.tensors:
                if t is not None:
                    t.record_stream(self.st["stream"])
        return False


def join_side_stream() -> None:
    """Make the current stream wait for every weight-gradient launch issued so far."""
    if not torch.cuda.is_available():
        return
    main = _main_stream()
    st = _side_streams.get(main.device)
    if st is not None and st["dirty"]:
        _py_op(main.wait_stream, st["stream"])
        st["dirty"] = False


def side_stream_event() -> T.Optional["torch.cuda.Event"]:
    """An event recorded on the weight-gradient side stream now (None when nothing is pending there): lets another
    stream -- the RCCL bucket stream -- wait for the gradients issued so far without stalling the compute stream."""
    if not torch.cuda.is_available():
        return None
    st = _side_streams.get(_main_stream().device)
    if st is None or not st["dirty"]:
        return None
    ev = torch.cuda.Event()
    ev.record(st["stream"])
    return ev


_aux_streams: T.Dict[T.Any, T.List["torch.cuda.Stream"]] = {}


# Hardware queues of one process (round 6, profiles/r06_hw_queues.txt). The HIP runtime keeps a pool of up to
# GPU_MAX_HW_QUEUES hardware queues PER STREAM PRIORITY, and this chip runs a process's queues concurrently
# only while there are at most SEVEN of them: with an eighth the queues are time-sliced and the whole step runs 1.5-1.9x
# slower (that is the "auxiliary streams + bucket collectives" slowdown of rounds 4-5: a torch.distributed process group
# brings six normal-priority streams with it -- 6 + the weight-gradient stream's lowest-priority queue + two
# highest-priority auxiliary queues = 9). The engine therefore owns exactly one queue per extra priority -- the
# weight-gradient stream (lowest) and ONE auxiliary stream for every spawn() (highest) -- and the process is expected to
# cap the normal pool at 5 (cultionet_amd.configure_runtime): 5 + 1 + 1 = 7 whatever the process group creates.
_HW_QUEUE_BUDGET = 7


def _hw_queue_cap() -> int:
    try:
        return int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))  # (unset: the runtime's default of 4)
    except ValueError:
        return 4


def branch_streams_allowed() -> bool:
    """spawn() runs its sub-graph on the auxiliary stream unless that could push the process over the hardware-queue
    budget: with a torch.distributed process group alive (six normal-priority streams of its own) the auxiliary stream
    needs GPU_MAX_HW_QUEUES <= 5 (cap + weight-gradient queue + auxiliary queue <= 7). Checked LIVE at every spawn()
    (ADVICE r4), so it follows the group's lifetime and covers the drop-in mode under Lightning's own DDP;
    ``engine.branch_streams(False)`` switches spawn() off for a scope. One-rank RCCL group, same box: bf16 2249 chips/s
    with the auxiliary stream at 5 queues against 2162 without it at 8 (single process 2279-2285); at 6 queues 1396."""
    if _state.no_branches:
        return False
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized():
        return _hw_queue_cap() + 2 <= _HW_QUEUE_BUDGET
    return True


class branch_streams:
    """Context manager: allow (default) / forbid spawn() to use auxiliary streams on this thread for a scope."""

    def __init__(self, enabled: bool):
        self.enabled = bool(enabled)

    def __enter__(self):
        self.prev = _state.no_branches
        _state.no_branches = not self.enabled
        return self

    def __exit__(self, *exc):
        _state.no_branches = self.prev
        return False


def _aux_stream(dev, k: int = 0) -> "torch.cuda.Stream":
    """THE auxiliary stream of ``dev`` (``k`` names the sub-graph for the reader: every spawn() shares one stream since
    round 6 -- a second highest-priority stream is a second hardware queue, see _HW_QUEUE_BUDGET; same box, single
    process: bf16 2279 / fp32 387.5 chips/s with one stream against 2285 / 385.8 with two)."""
    if _OVERLAP_WGRAD:
        _side_state(dev)  # HIP deals streams to hardware queues in creation order: the weight-gradient stream first
    lst = _aux_streams.setdefault(dev, [])
    if not lst:
        # HIGHEST priority, through the C ABI like the weight-gradient stream: a priority is a property of the hardware
        # queue, so this stream can never be dealt the queue of the compute stream, of the (lowest-priority)
        # weight-gradient stream or of RCCL's streams -- with torch.cuda.Stream() (normal priority) a live process group
        # put an auxiliary stream on a queue shared with the compute stream: 2115 -> 1255 chips/s (bf16), 377 -> 241 (fp32).
        lst.append(_priority_stream(dev, lowest=False))
    return lst[0]


# ---- the engine's allocator -----------------------------------------------------------------------------------------
# Every per-step buffer of the engine (activations, gradients, statistics rows, masks, scratch) comes from _alloc().
# torch's caching allocator only knows the compute stream, while launches carry explicit stream handles: whoever needs
# buffers to outlive a host-side free -- the branches of spawn() until they are joined, a launch plan while it is being
# recorded -- registers a list as an allocation SINK of the calling thread (``holding_allocations``), and _alloc() files
# every tensor it hands out there. Nothing in ``torch``'s namespace is touched (rounds 3-5 wrapped
# torch.empty / zeros / full process-wide instead).
def _alloc(shape, dtype: torch.dtype, device) -> torch.Tensor:
    t = torch.empty(shape, dtype=dtype, device=device)
    sinks = _state.alloc_sinks
    if sinks:
        for sink in sinks:
            sink.append(t)
    return t


def _alloc_like(t: torch.Tensor) -> torch.Tensor:
    return _alloc(tuple(t.shape), t.dtype, t.device)


def alloc(shape, dtype: torch.dtype, device) -> torch.Tensor:
    """Public form of the engine allocator for the host mirror (unet_parts / lightning): a buffer whose lifetime follows
    the calling thread's open branches / plan recording."""
    return _alloc(shape, dtype, device)


def _new(shape, like: torch.Tensor) -> torch.Tensor:
    if like.dtype == torch.bfloat16 and len(shape) == 4:
        B, C, H, W = shape
        return _alloc((B, H, W, C), torch.bfloat16, like.device).permute(0, 3, 1, 2)
    return _alloc(shape, torch.float32, like.device)


def new_buffer(shape, like: torch.Tensor) -> torch.Tensor:
    """An activation buffer of logical shape [B,C,H,W] in ``like``'s precision / layout (fp32 NCHW or bf16 NHWC)."""
    return _new(tuple(shape), like)


class holding_allocations:
    """Context manager: every buffer _alloc() hands out on this thread is also appended to ``sink`` (kept alive by it)."""

    def __init__(self, sink: T.List[T.Any]):
        self.sink = sink

    def __enter__(self):
        sinks = _state.alloc_sinks
        if sinks is None:
            sinks = _state.alloc_sinks = []
        sinks.append(self.sink)
        return self.sink

    def __exit__(self, *exc):
        sinks = _state.alloc_sinks
        for i in range(len(sinks) - 1, -1, -1):
            if sinks[i] is self.sink:
                del sinks[i]
                break
        return False


class _KeepAlive:
    """Frees are deferred while any branch is open. torch's caching allocator only knows the compute stream (launches
    go through the C ABI with explicit stream handles): a block freed on the host while an auxiliary stream's kernel
    still uses it could be handed to a compute-stream allocation at once. Reference-counted per thread: buffers the
    engine allocates (``keep`` is an allocation sink of _alloc while depth > 0), finished backward closures and incoming
    gradients are held until the thread's last open branch has been joined."""

    def __init__(self):
        self.depth = 0
        self.keep: T.List[T.Any] = []
        self._hold: T.Optional[holding_allocations] = None

    def acquire(self) -> None:
        self.depth += 1
        if self.depth == 1:
            self._hold = holding_allocations(self.keep)
            self._hold.__enter__()

    def release(self, force: bool = False) -> None:
        if self.depth == 0:
            return
        self.depth = 0 if force else self.depth - 1
        if self.depth == 0:
            if self._hold is not None:
                self._hold.__exit__(None, None, None)
                self._hold = None
            self.keep = []


def _keepalive() -> _KeepAlive:
    ka = _state.keepalive
    if ka is None:
        ka = _state.keepalive = _KeepAlive()
    return ka
