"""Tape layer of the engine: ``Var``, the reverse-mode ``Tape``, gradient-buffer plumbing, and the spawn() / join()
branches that run small sub-graphs of the tape on the auxiliary stream.

Layer order runtime -> params -> scratch -> tape -> engine: this module imports from the three above it; the ops of
``engine`` are built on it.
"""
from __future__ import annotations

import contextlib
import typing as T

import torch

from . import _lib, runtime
from .params import _bind_conv_workspace, current_store
from .runtime import (_aux_stream, _keepalive, _main_stream, _new, _py_op, _rows, _state, _stream, branch_streams_allowed,
                      bstride, is16, join_side_stream, ld)
from .scratch import deferring_slice_sums


class Var:
    """A device buffer and (during training) its gradient buffer."""

    __slots__ = ("t", "grad", "req", "parent", "stats", "bnfin")

    def __init__(self, t: torch.Tensor, req: bool = False):
        self.t = t
        self.grad: T.Optional[torch.Tensor] = None
        self.req = req
        self.parent: T.Optional[T.Tuple["Var", int, int]] = None  # channel slice [c0, c1) of another Var
        self.stats: T.Optional[torch.Tensor] = None  # bf16 conv outputs: per-channel {sum, sumsq} from the epilogue
        self.bnfin = None  # (bn module, mean, rstd): BatchNorm statistics already finished by the producing conv launch

    @property
    def shape(self):
        return self.t.shape


def _tr(p: T.Optional[torch.Tensor]) -> bool:
    """Does parameter ``p`` get a gradient (exists and ``requires_grad``)? Frozen parameters get none."""
    return p is not None and p.requires_grad


def _req(tape: "Tape", vs: T.Sequence[T.Optional[Var]] = (), params: T.Sequence[T.Optional[torch.Tensor]] = ()) -> bool:
    """Does an op's output need a gradient: the tape is on and an input or one of the op's own parameters needs one.
    An op whose output needs none records no tape node."""
    if not tape.enabled:
        return False
    return any(v is not None and v.req for v in vs) or any(p is not None and p.requires_grad for p in params)


class Tape:
    def __init__(self, enabled: bool):
        self.enabled = enabled
        self.nodes: T.List[T.Callable[[], None]] = []
        self.marks: T.Dict[int, int] = {}  # flat offset of a parameter -> index of the node that uses it

    def add(self, fn: T.Callable[[], None], params: T.Sequence[T.Optional[torch.Tensor]] = ()) -> None:
        if self.enabled:
            br = _state.branch
            if br is not None:  # recorded inside spawn(): its backward runs on the branch's stream
                fn = br.wrap(fn)
            self.nodes.append(fn)
            if params:
                base = current_store()._base
                idx = len(self.nodes) - 1
                for p in params:
                    # frozen parameters get no gradient: only trainable offsets are marked (the bucket plan relies on it)
                    if p is not None and p.requires_grad:  # a gradient is final once backward has passed the FIRST node that used it
                        k = (p.data_ptr() - base) // 4
                        self.marks[k] = min(self.marks.get(k, idx), idx)

    def backward(self) -> None:
        nodes, self.nodes = self.nodes, []
        hold = begin_branch_backward(self)
        store = _state.store
        try:
            with deferring_slice_sums(store) if store is not None else contextlib.nullcontext():
                while nodes:
                    fn = nodes.pop()
                    fn()
                    if hold is not None:
                        hold.append(fn)
        finally:
            release_branches()
        join_side_stream()


def current_tape() -> Tape:
    tp = _state.tape
    if tp is None:
        tp = Tape(False)
        _state.tape = tp
    return tp


class recording:
    """Context manager: run forward ops under a fresh tape (enabled or not)."""

    def __init__(self, enabled: bool = True):
        self.tape = Tape(enabled)

    def __enter__(self) -> Tape:
        self.prev = _state.tape
        _state.tape = self.tape
        return self.tape

    def __exit__(self, *exc):
        _state.tape = self.prev
        return False


# ---------------------------------------------------------------------------
# gradient plumbing
# ---------------------------------------------------------------------------

def grad_buffer(v: Var) -> T.Tuple[torch.Tensor, int]:
    """(buffer, accumulate flag) to write/accumulate v's gradient into."""
    if v.grad is None:
        if v.parent is not None:
            # a channel slice writes straight into its parent's gradient (zero-filled once, then accumulated)
            pv, c0, c1 = v.parent
            if pv.grad is None:
                pv.grad = _new(tuple(pv.t.shape), pv.t)
                if is16(pv.t):
                    _lib.call("cn_zero_bf16", pv.grad.data_ptr(), ld(pv.grad), _rows(pv.grad), pv.grad.shape[1], _stream())
                else:
                    _lib.call("cn_fill_f32", pv.grad.data_ptr(), pv.grad.numel(), 0.0, _stream())
            v.grad = pv.grad[:, c0:c1]
            return v.grad, 1
        v.grad = _new(tuple(v.t.shape), v.t)
        return v.grad, 0
    return v.grad, 1


def give_grad(v: Var, g: torch.Tensor) -> None:
    """v.grad (+)= g where the op is the identity on the gradient: alias when first, else add in place."""
    if not v.req:
        return
    if v.grad is None and v.parent is None:
        v.grad = g
        return
    if v.grad is None:
        grad_buffer(v)
    if is16(g):
        _lib.call("cn_copy_bf16", g.data_ptr(), ld(g), v.grad.data_ptr(), ld(v.grad), _rows(g), g.shape[1], 1, _stream())
        return
    B = g.shape[0]
    n = g[0].numel()
    _lib.call("cn_copy_f32", g.data_ptr(), bstride(g), v.grad.data_ptr(), bstride(v.grad), B, n, 1, _stream())


# ---------------------------------------------------------------------------
# small sub-graphs beside the big kernels: spawn() / join()
# ---------------------------------------------------------------------------
# final_c and final_b (TowerUNetFinal, nunet.py:197-202 of the reference) are chains of ~15 small launches forward and
# ~25 backward on 9- / 3- / 1-channel tensors. They depend only on x_tower_c / x_tower_b, which exist long before the
# forward reaches the heads, and in backward nothing needs their result until tower_b / tower_c run. spawn() puts such
# a chain on an auxiliary stream the moment its input exists, so that it executes BESIDE the MFMA-bound tower
# convolutions of the compute stream (the regime in which overlap pays on this chip: a bandwidth- / latency-bound kernel
# next to a matrix-pipe-bound one); its tape nodes run on the same stream in backward. ``branch_streams(False)``: off.

def begin_branch_backward(tape) -> T.Optional[T.List[T.Any]]:
    """A tape with spawned branches: NOTHING is freed during its backward (returns the list that holds the finished
    nodes' closures; the engine's allocations are filed there by _alloc). Between a branch's start and its fork the compute stream
    runs arbitrary nodes of its own; a block one of them frees on the host while its kernel is still queued must not be
    handed to an allocation whose kernel runs on an auxiliary stream."""
    if not getattr(tape, "has_branches", False):
        return None
    ka = _keepalive()
    ka.acquire()
    return ka.keep


def release_branches() -> None:
    """After a backward pass (also one that raised): nothing may be left holding tensors or torch wrappers."""
    _keepalive().release(force=True)
    _state.open_branches = []


def aux_stream_events() -> T.List["torch.cuda.Event"]:
    """Events recorded now on the auxiliary streams with backward work of open branches (for the RCCL bucket stream,
    like side_stream_event())."""
    out = []
    for br in _state.open_branches or ():
        ev = torch.cuda.Event()
        ev.record(br.stream)
        out.append(ev)
    return out


class _Branch:
    def __init__(self, stream: "torch.cuda.Stream", main: "torch.cuda.Stream", inputs, aliases):
        self.stream, self.main = stream, main
        self.inputs, self.aliases = inputs, aliases
        self.fork_ev, self.done_ev = torch.cuda.Event(), torch.cuda.Event()
        self.left = 0
        self.result = None

    def enter(self):
        prev = (_state.stream_override, _state.stream_obj_override)
        _state.stream_override, _state.stream_obj_override = self.stream.cuda_stream, self.stream
        _bind_conv_workspace(self.main.device)
        return prev

    @staticmethod
    def leave(prev) -> None:
        _state.stream_override, _state.stream_obj_override = prev

    def wrap(self, fn: T.Callable[[], None]) -> T.Callable[[], None]:
        self.left += 1

        def node():
            prev = self.enter()
            try:
                fn()
            finally:
                self.leave(prev)
            _keepalive().keep.append(fn)  # its closure (saved activations) lives until the branches are joined
            self.left -= 1
            if self.left == 0:
                _py_op(self.done_ev.record, self.stream)

        return node

    def bwd_fork(self) -> None:
        """In backward this runs AFTER the branch's nodes (it was recorded before them): the compute stream waits for
        the branch, takes over the gradients of its inputs, and the deferred frees of this branch are released."""
        _py_op(self.main.wait_event, self.done_ev)
        for x, xa in zip(self.inputs, self.aliases):
            if xa.grad is not None:
                give_grad(x, xa.grad)
                xa.grad = None
        ob = _state.open_branches
        if ob and self in ob:
            ob.remove(self)
        _keepalive().release()


def spawn(fn: T.Callable[..., T.Any], inputs: T.Sequence[Var], k: int) -> T.Tuple[T.Optional[_Branch], T.Any]:
    """Run ``fn(*aliases of inputs)`` -- engine ops that read nothing but ``inputs`` and the parameters -- on auxiliary
    stream k, concurrently with whatever the compute stream does next. Returns (branch, result); join([branch, ...])
    must be called before the result is used. The branch sees ALIASES of its inputs (same tensors, own gradient slots):
    two streams never accumulate into one gradient buffer; the compute stream adds the alias gradients in bwd_fork."""
    tape = current_tape()
    if (not runtime._OVERLAP_WGRAD or not torch.cuda.is_available() or _state.stream_override is not None
            or _state.branch is not None or not branch_streams_allowed()):
        return None, fn(*inputs)
    main = _main_stream()
    aliases = [Var(x.t, x.req) for x in inputs]
    br = _Branch(_aux_stream(main.device, k), main, list(inputs), aliases)
    if tape.enabled:
        tape.has_branches = True
        tape.add(br.bwd_fork)
    _keepalive().acquire()
    _py_op(br.fork_ev.record, main)
    _py_op(br.stream.wait_event, br.fork_ev)
    prev = br.enter()
    _state.branch = br
    try:
        br.result = fn(*aliases)
    finally:
        _state.branch = None
        br.leave(prev)
    _py_op(br.done_ev.record, br.stream)
    return br, br.result


def join(branches: T.Sequence[T.Optional[_Branch]]) -> None:
    """The compute stream waits for the spawned branches (forward); in backward this is where they may start."""
    brs = [b for b in branches if b is not None]
    if not brs:
        return
    tape = current_tape()
    for br in brs:
        _py_op(br.main.wait_event, br.done_ev)
        _keepalive().release()
    if not tape.enabled:
        return

    def bwd_join():
        ka = _keepalive()
        ob = _state.open_branches
        if ob is None:
            ob = _state.open_branches = []
        ev = torch.cuda.Event()
        for br in brs:
            ka.acquire()
            ob.append(br)
            r = br.result
            for v in (r if isinstance(r, (tuple, list)) else (r,)):
                if isinstance(v, Var) and v.grad is not None:
                    ka.keep.append(v.grad)  # allocated before the deferral began, freed inside the branch
        _py_op(ev.record, brs[0].main)
        for br in brs:
            _py_op(br.stream.wait_event, ev)
            if br.left == 0:  # no backward nodes: nothing to wait for at the fork
                _py_op(br.done_ev.record, br.stream)

    tape.add(bwd_join)
