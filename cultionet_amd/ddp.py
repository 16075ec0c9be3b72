"""Data-parallel gradient exchange: bucketed all-reduce of the flat gradient, overlapped with backward.

The reference's only multi-GPU strategy is Lightning ``strategy="ddp"`` (torch DDP over NCCL;
/root/reference/src/cultionet/model.py:101,168-186). Here one process drives one MI355X; the only exchange
step of the hot path is the sum of the flat fp32 gradient buffer across ranks (RCCL over xGMI;
``torch.distributed`` backend "nccl" IS RCCL on ROCm). BatchNorm statistics stay per rank (the reference
does not enable sync_batchnorm) and the loss is logged per rank.

Mechanics: parameters are registered in forward order inside ONE flat buffer and the tape runs backward,
so gradients complete from the END of the buffer towards its start. The buffer is cut into contiguous
buckets (default 8 MiB: a handful of launches per step -- each ring all-reduce is bound by one
~153 GB/s xGMI link, so fewer, larger messages beat torch's 25 MB/param-list bucketing of 270 tensors);
a bucket is launched on a side stream as soon as the tape has passed the first forward node that used any
of its parameters, and the compute stream only waits for the collectives before the optimizer step.
The 1/world_size averaging is folded into the fused AdamW kernel (grad_scale).
"""
from __future__ import annotations

import typing as T

import torch
import torch.distributed as dist

from . import engine as _engine


def plan_buckets(offsets: T.Sequence[int], sizes: T.Sequence[int], ready_node: T.Sequence[int], total: int,
                 bucket_elems: int, trainable: T.Optional[T.Sequence[bool]] = None) -> T.List[T.Tuple[int, int, int]]:
    """Cut [0, total) into contiguous buckets walking parameters from last to first.

    Returns [(lo, hi, ready)] where ``ready`` is the tape node index after which the whole bucket is final
    (the minimum forward node index over its parameters; backward visits nodes in decreasing order).
    ``trainable`` (one flag per parameter): frozen parameters have no gradient and are never communicated -- the
    buckets then cover the runs of adjacent trainable parameters only (each run from its first parameter's offset to
    the padded end of its last), cut the same way.
    """
    order = sorted(range(len(offsets)), key=lambda i: offsets[i], reverse=True)
    if trainable is None or all(trainable):
        runs = [(0, total, order)]
    else:
        runs = []  # (lo, hi, parameters from last to first) of every run of adjacent trainable parameters
        for n, i in enumerate(order):
            if not trainable[i]:
                continue
            if n > 0 and trainable[order[n - 1]]:  # continues the run of the parameter after it
                runs[-1][2].append(i)
            else:  # a run ends where the next parameter's slice begins
                runs.append((0, offsets[order[n - 1]] if n > 0 else total, [i]))
        runs = [(offsets[ps[-1]], hi, ps) for _, hi, ps in runs]
    buckets: T.List[T.Tuple[int, int, int]] = []
    for run_lo, hi, ps in runs:
        cur_ready = None
        for n, i in enumerate(ps):
            r = ready_node[i]
            cur_ready = r if cur_ready is None else min(cur_ready, r)
            lo = offsets[i]
            last = n == len(ps) - 1
            if hi - lo >= bucket_elems or last:
                if last:
                    lo = run_lo
                buckets.append((lo, hi, cur_ready))
                hi = lo
                cur_ready = None
    return buckets


def broadcast_module_state(store, module=None, group=None, src: int = 0) -> None:
    """What torch DDP does at construction (the reference's strategy="ddp"): every rank starts from rank ``src``'s
    parameters and buffers. One broadcast of the flat parameter buffer + one per floating-point buffer (BatchNorm
    running statistics); integer buffers (num_batches_tracked) are identical by construction."""
    dist.broadcast(store.flat, src=src, group=group)
    if module is not None:
        for b in module.buffers():
            if b.is_floating_point():
                dist.broadcast(b, src=src, group=group)
    store.bump()


class GradientAllReduce:
    def __init__(self, world_size: T.Optional[int] = None, bucket_mb: float = 8.0, group=None):
        self.group = group
        self.world_size = world_size if world_size is not None else dist.get_world_size(group)
        self.rank = dist.get_rank(group) if dist.is_available() and dist.is_initialized() else 0
        self.bucket_elems = int(bucket_mb * (1 << 20) / 4)
        self.comm_stream = None
        self._plan = None
        self._plan_key = None
        # diagnostics (bench.py): with ``measure`` on, every backward appends an event pair bracketing the compute
        # stream's wait for the collectives to ``exposed`` (elapsed = communication time NOT hidden behind backward)
        self.measure = False
        self.exposed: T.List[T.Tuple[T.Any, T.Any]] = []
        self.buckets_last_step = 0

    def sync_initial_state(self, store, module=None) -> None:
        """Replicas must start identical (init_conv_weights is random per process): broadcast rank 0's state."""
        if self.world_size > 1:
            broadcast_module_state(store, module, group=self.group, src=0)

    def _get_plan(self, tape, store):
        tm = getattr(store, "trainable_mask", None)  # (None: a store without frozen parameters)
        mask = tm() if tm is not None else None
        key = (len(tape.nodes), store.numel, mask)
        if self._plan is None or self._plan_key != key:
            sizes = [p.numel() for p in store.params]
            ready = [tape.marks.get(o, 0) for o in store.offsets]
            self._plan = plan_buckets(store.offsets, sizes, ready, store.numel, self.bucket_elems, mask)
            self._plan_key = key
        return self._plan

    def backward(self, tape, store) -> None:
        """Run ``tape`` backward, all-reducing (SUM) each bucket of ``store.flat_grad`` as soon as it is final."""
        plan = self._get_plan(tape, store)
        by_node: T.Dict[int, T.List[T.Tuple[int, int]]] = {}
        for lo, hi, r in plan:
            by_node.setdefault(r, []).append((lo, hi))
        flat = store.flat_grad
        on_gpu = flat.is_cuda
        works = []
        if on_gpu and self.comm_stream is None:
            self.comm_stream = torch.cuda.Stream(device=flat.device)
        nodes, tape.nodes = tape.nodes, []
        hold = _engine.begin_branch_backward(tape)
        try:
            with _engine.deferring_slice_sums(store):
                for k in range(len(nodes) - 1, -1, -1):
                    nodes[k]()
                    if hold is not None:
                        hold.append(nodes[k])
                    nodes[k] = None
                    ready = by_node.get(k, ())
                    if ready and on_gpu:
                        # the weight-gradient slice sums deferred so far: ONE launch, in front of the bucket's event
                        _engine.flush_slice_sums()
                    # weight gradients run on the engine's side stream: the bucket stream waits for them, the compute
                    # stream does not (joining it here five times per step would serialise the two streams at every bucket)
                    side_ev = _engine.side_stream_event() if (ready and on_gpu) else None
                    for lo, hi in ready:
                        works.append(self._launch(flat[lo:hi], on_gpu, side_ev))
        finally:
            _engine.release_branches()
        if on_gpu:
            _engine.join_side_stream()
        for lo, hi, r in plan:  # buckets whose ready index lies outside the tape (no nodes recorded)
            if r >= len(nodes) or r < 0:
                works.append(self._launch(flat[lo:hi], on_gpu, None))
        self.buckets_last_step = len(works)
        ev0 = None
        if on_gpu and self.measure:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record(torch.cuda.current_stream())
        for w in works:
            w.wait()  # NCCL: makes the current (compute) stream wait for the collective; gloo: blocks
        if ev0 is not None:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record(torch.cuda.current_stream())
            self.exposed.append((ev0, ev1))

    def reduce(self, store) -> None:
        """All-reduce (SUM) ``store.flat_grad`` outside a backward pass, in one collective: a trailing group of
        accumulated micro-batches whose last backward ran without communication."""
        flat = store.flat_grad
        if flat.is_cuda and self.comm_stream is None:
            self.comm_stream = torch.cuda.Stream(device=flat.device)
        self._launch(flat, flat.is_cuda).wait()
        self.buckets_last_step = 1

    def _launch(self, chunk: torch.Tensor, on_gpu: bool, side_ev=None):
        if not on_gpu:
            return dist.all_reduce(chunk, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.comm_stream):
            self.comm_stream.wait_event(ev)
            if side_ev is not None:
                self.comm_stream.wait_event(side_ev)
            for ev in _engine.aux_stream_events():  # head branches still running their backward on auxiliary streams
                self.comm_stream.wait_event(ev)
            return dist.all_reduce(chunk, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
