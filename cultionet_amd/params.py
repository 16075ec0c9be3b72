"""Parameter layer of the engine: the flat fp32 parameter / gradient store (``ParamStore``), the packed weight copies
of the implicit-GEMM kernels with their registry, the split-K workspace binding and the workspace epoch.

Layer order runtime -> params -> scratch -> tape -> engine: this module imports from ``runtime`` only. ``_ws_epoch`` is
rebound here alone; everyone else calls ``workspace_epoch()`` / ``_bump_ws_epoch()``.
"""
from __future__ import annotations

import bisect
import os
import struct
import typing as T

import torch

from . import _lib
from .runtime import _alloc, _state, _stream


# ---------------------------------------------------------------------------
# flat parameter store
# ---------------------------------------------------------------------------

class PackFormat(T.NamedTuple):
    """One layout of the implicit-GEMM weight copies: the single-pack and the batched entry point, the element count
    of a copy of (T, K, N), its element type, and (wptr, dst ptr, T, K, N, sk, sn, st) -> the bytes of one record of
    the batched entry point's descriptor table."""
    pack: str
    batched: str
    elems: T.Callable[[int, int, int], int]
    dtype: torch.dtype
    record: T.Callable[..., bytes]


def _pack_record_f32(wptr: int, dst: int, T_: int, K: int, N: int, sk: int, sn: int, st: int) -> bytes:
    """CnPackDesc (csrc/cn_conv.hip), 64 bytes."""
    kp, np_ = _lib.query("cn_conv_kpad", K), _lib.query("cn_conv_npad", N)
    return struct.pack("<QQiiiiiiqqq", wptr, dst, T_, K, N, kp, np_, 0, sk, sn, st)


def _pack_record_bf16(wptr: int, dst: int, T_: int, K: int, N: int, sk: int, sn: int, st: int) -> bytes:
    """CnBPackDesc (csrc/cn_bconv.hip), 72 bytes (nscale = NULL)."""
    return struct.pack("<QQiiiiiiqqqQ", wptr, dst, T_, K, N, (K + 15) // 16, (N + 31) // 32, 0, sk, sn, st, 0)


PACK_F32 = PackFormat(  # [tap][Kpad][Npad] fp32
    "cn_pack_weights_f32", "cn_pack_weights_batched_f32",
    lambda T_, K, N: T_ * _lib.query("cn_conv_kpad", K) * _lib.query("cn_conv_npad", N),
    torch.float32, _pack_record_f32)
PACK_BF16 = PackFormat(  # bf16 MFMA fragments (mixed-precision path)
    "cn_pack_weights_bf16", "cn_pack_weights_batched_bf16",
    lambda T_, K, N: _lib.query("cn_bconv_packed_elems", T_, K, N),
    torch.bfloat16, _pack_record_bf16)


def select_packs(offsets: T.Sequence[int], spans: T.Sequence[T.Tuple[int, int]],
                 dirty: T.Optional[T.AbstractSet[int]]) -> T.List[int]:
    """Indices of the pack records to refresh: all of them (``dirty`` None), else those whose source -- elements
    [lo, hi) of the flat buffer: a dense weight tensor, or adjacent ones (a declared group) -- overlaps a parameter in
    ``dirty`` (parameter i starts at ``offsets[i]``, ascending)."""
    if dirty is None:
        return list(range(len(spans)))
    out = []
    for r, (lo, hi) in enumerate(spans):
        i = max(bisect.bisect_right(offsets, lo) - 1, 0)
        while i < len(offsets) and offsets[i] < hi:
            if i in dirty:
                out.append(r)
                break
            i += 1
    return out


_SUB_TABLES_KEPT = 8  # pack tables (ParamStore.repack_all) cached per set of changed parameters ("any" is one of them)


class ParamStore:
    """All parameters of a module in one flat fp32 buffer; gradients likewise.

    ``param.data`` becomes a view of ``flat`` (checkpoints / state_dict keep working); gradients are
    accumulated by the kernels into ``flat_grad``, on which the fused AdamW step and the RCCL
    all-reduce operate directly (``attach_grads`` exposes them as ``param.grad`` views).
    """

    _serial = __import__("itertools").count(1)

    def __init__(self, module: torch.nn.Module):
        params = [p for p in module.parameters()]
        if not params:
            raise ValueError("module has no parameters")
        params = self._with_contiguous_groups(module, params)
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError("ParamStore needs the module on the GPU (call .to('cuda') first)")
        self.params = params
        offs, n = [], 0
        for p in params:
            offs.append(n)
            n += (p.numel() + 3) // 4 * 4  # 16-byte aligned slices
        self.numel = n
        self.offsets = offs
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(params, offs):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        self.version = 0  # bumped whenever parameter values change (invalidates packed weights)
        # process-unique serial: caches key their validity on it (CPython may hand a rebuilt store the id() of a dead one,
        # and a cached VIEW of the old flat buffer would then be used silently -- ADVICE r4)
        self.uid = next(ParamStore._serial)
        self._sig = self._signature()
        self._base = self.flat.data_ptr()
        self._packs: T.List[T.Tuple] = []  # (PackFormat, dst tensor, w ptr, T, K, N, sk, sn, st): every registered copy
        self.packed_version = self.version  # the parameter values the registered copies hold (repack_all)
        # parameters written since the last repack: None = any of them (a full repack), else a set of indices (the
        # optimizer step of a model with frozen parameters writes the trainable ones only)
        self._dirty: T.Optional[T.FrozenSet[int]] = None
        # dirty set -> [(batched entry point, device table, records)] of its repack, most recently used last
        self._tables: T.Dict[T.Optional[T.FrozenSet[int]], T.List[T.Tuple[str, torch.Tensor, int]]] = {}

    @staticmethod
    def _with_contiguous_groups(module: torch.nn.Module, params: T.List[torch.nn.Parameter]) -> T.List[torch.nn.Parameter]:
        """Registration order with the members of every declared group made adjacent (at the place of the group's first
        member). A submodule declares groups through ``cn_contiguous_params()`` -> lists of parameters that one kernel
        reads / writes as ONE tensor (the three 128 -> 3 head convolutions of a tower: one 128 -> 9 convolution on the
        views, no concatenated copies of weights or gradients). Members must be multiples of 4 elements (the store pads
        every slice to 16 bytes: a padded member would break adjacency)."""
        first_of, member = {}, set()
        for m in module.modules():
            fn = getattr(m, "cn_contiguous_params", None)
            if fn is None:
                continue
            for grp in fn():
                grp = list(grp)
                if len(grp) < 2 or any(q.numel() % 4 for q in grp) or any(id(q) in member for q in grp):
                    continue
                first_of[id(grp[0])] = grp
                member.update(id(q) for q in grp)
        if not first_of:
            return params
        out = []
        for q in params:
            if id(q) in first_of:
                out.extend(first_of[id(q)])
            elif id(q) not in member:
                out.append(q)
        assert len(out) == len(params)
        return out

    def owns(self, module: torch.nn.Module) -> bool:
        lo, hi = self._base, self._base + self.numel * 4
        first, last = self.params[0], self.params[-1]
        return lo <= first.data_ptr() < hi and lo <= last.data_ptr() < hi

    def grad_of(self, p: torch.Tensor) -> torch.Tensor:
        """Gradient slice matching a parameter (or any dense view of one) inside the flat buffer."""
        o = (p.data_ptr() - self._base) // 4
        if o < 0 or o + p.numel() > self.numel:
            raise RuntimeError("tensor is not part of this ParamStore (was the module moved or re-created?)")
        return self.flat_grad[o:o + p.numel()].view(p.shape)

    def attach_grads(self) -> None:
        """Point every ``param.grad`` at its slice of the flat gradient (for torch optimizers driving the NATIVE step).
        Not for drop-in mode: autograd_bridge hands the flat buffer itself to autograd at every backward (p.grad then
        IS a view of that step's buffer) and gives the store a fresh one, so views attached here would go stale."""
        for p, o in zip(self.params, self.offsets):
            p.grad = self.flat_grad[o:o + p.numel()].view(p.shape)

    def zero_grad(self) -> None:
        _lib.call("cn_fill_f32", self.flat_grad.data_ptr(), self.numel, 0.0, _stream())

    def bump(self, changed: T.Optional[T.Sequence[bool]] = None) -> None:
        """The parameter values changed. ``changed``: mask (one flag per parameter, store order) of the parameters
        that did; None = any may have. Packed copies of the others are not refreshed."""
        self.version += 1
        if changed is None:
            self._dirty = None
        elif self._dirty is not None:
            self._dirty = self._dirty | frozenset(i for i, c in enumerate(changed) if c)

    def trainable_mask(self) -> T.Tuple[bool, ...]:
        """``requires_grad`` of every parameter in store order: the trainable set (frozen parameters get no gradient)."""
        return tuple(p.requires_grad for p in self.params)

    def _signature(self) -> int:
        """Sum of the parameters' torch version counters: moves whenever anything outside the engine writes a
        parameter in place (torch optimizers in drop-in mode, ``load_state_dict`` / ``load_from_checkpoint`` through
        nn.Module's recursion, ``param.data.copy_``). The engine's own kernels (fused AdamW) do not touch it and call
        ``bump()`` themselves."""
        return sum(p._version for p in self.params)

    def refresh(self) -> None:
        """Invalidate the packed weight copies if the parameters were modified behind the engine's back."""
        sig = self._signature()
        if sig != self._sig:
            self._sig = sig
            self.bump()

    def register_pack(self, fmt: PackFormat, dst: torch.Tensor, w: torch.Tensor, T_: int, K: int, N: int, sk: int,
                      sn: int, st: int) -> None:
        self._packs.append((fmt, dst, w.data_ptr(), T_, K, N, sk, sn, st))
        self._tables.clear()  # (they list the copies registered so far)

    def _build_tables(self, dirty: T.Optional[T.FrozenSet[int]]) -> T.List[T.Tuple[str, torch.Tensor, int]]:
        """The descriptor tables that refresh the copies of the parameters in ``dirty``: bf16 first, then fp32 (the
        order recorded plans hold), none for a precision without records."""
        spans = []
        for (_fmt, _dst, wptr, T_, K, N, *_strides) in self._packs:
            lo = (wptr - self._base) // 4
            spans.append((lo, lo + T_ * K * N))
        chosen = [self._packs[i] for i in select_packs(self.offsets, spans, dirty)]
        tables = []
        for fmt in (PACK_BF16, PACK_F32):
            recs = [fmt.record(wptr, dst.data_ptr(), *dims) for (f, dst, wptr, *dims) in chosen if f is fmt]
            if recs:
                table = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8).clone().to(self.flat.device)
                tables.append((fmt.batched, table, len(recs)))
        return tables

    def repack_all(self) -> None:
        """Refresh the registered packed weight copies with ONE launch per precision (after the parameters changed):
        every copy, or -- when only known parameters changed (bump with a mask) -- the copies of those."""
        dirty = self._dirty
        self._dirty = frozenset()
        self.packed_version = self.version
        tables = self._tables.pop(dirty, None)
        if tables is None:
            tables = self._build_tables(dirty)
        self._tables[dirty] = tables  # most recently used last; a few trainable sets are kept (gradual unfreezing)
        while len(self._tables) > _SUB_TABLES_KEPT:
            self._tables.pop(next(iter(self._tables)))
        for sink in _state.alloc_sinks or ():  # a plan being recorded bakes the table pointers in:
            sink.extend(t for (_name, t, _n) in tables)          # it keeps the tables alive past their eviction
        for (name, t, n) in tables:
            _lib.call(name, t.data_ptr(), n, _stream())


SEG_CHUNK = 4096  # elements per chunk of the segmented optimizer kernels (CN_SEG_CHUNK in csrc/cn_optim.hip)


def trainable_segments(offsets: T.Sequence[int], sizes: T.Sequence[int], trainable: T.Sequence[bool],
                       steps: T.Sequence[int]) -> T.List[T.Tuple[int, int, int]]:
    """The runs of trainable parameters in the flat buffer as [(offset, length, step)]: adjacent trainable parameters
    with equal AdamW step counts merge (across the 16-byte padding between their slices, which is zero in every
    buffer); a frozen parameter or a different step count starts a new run."""
    segs: T.List[T.List[int]] = []
    end = None  # padded end of the previous parameter, when it is trainable
    for i in sorted(range(len(offsets)), key=lambda k: offsets[k]):
        o, n = int(offsets[i]), int(sizes[i])
        if not trainable[i] or n <= 0:
            end = None
            continue
        if end is not None and end == o and segs[-1][2] == int(steps[i]):
            segs[-1][1] = o + n - segs[-1][0]
        else:
            segs.append([o, n, int(steps[i])])
        end = o + (n + 3) // 4 * 4
    return [tuple(x) for x in segs]


def segment_table(segs: T.Sequence[T.Tuple[int, int, int]]) -> T.Tuple[bytes, int]:
    """The 24-byte CnSeg records of ``segs`` for cn_*_seg_f32 and the total chunk count."""
    buf, chunk = bytearray(), 0
    for o, n, st in segs:
        buf += struct.pack("<qqii", o, n, st, chunk)
        chunk += (n + SEG_CHUNK - 1) // SEG_CHUNK
    return bytes(buf), chunk


# Launch plans (cultionet_amd/replay.py) bake the raw pointers of the process-wide scratch buffers below into their
# recorded arguments. Every (re)allocation of one of them bumps this epoch; the plans' keys hold it, so a plan recorded
# against an older buffer is never replayed (it is re-recorded against the current one).
_ws_epoch = 0


def workspace_epoch() -> int:
    return _ws_epoch


def _bump_ws_epoch() -> None:
    global _ws_epoch
    _ws_epoch += 1


_CONV_WS_FLOATS = 16 << 20  # split-K partial slices of the implicit-GEMM launches (64 MB, one per process)
_conv_ws: T.Dict[T.Tuple[str, int], torch.Tensor] = {}


def _bind_conv_workspace(dev: torch.device) -> None:
    """Register a split-K scratch buffer for the CURRENT stream (the library keys its scratch by stream, so model
    instances running on different streams / autograd worker threads never share one)."""
    s = _stream()
    key = (str(dev), s)
    if key in _conv_ws:
        return
    ws = torch.empty(_CONV_WS_FLOATS, dtype=torch.float32, device=dev)
    _conv_ws[key] = ws
    _bump_ws_epoch()
    _lib.call("cn_conv_set_workspace", s, ws.data_ptr(), ws.numel())
    # CN_AUTOTUNE=1: measure the (tile, K split) candidates per conv shape during the first steps instead of
    # trusting the launch-cost model (+0.5 % at batch 8; off by default so that runs are reproducible)
    _lib.call("cn_conv_set_autotune", 1 if os.environ.get("CN_AUTOTUNE", "0") == "1" else 0)


def current_store() -> ParamStore:
    st = _state.store
    if st is None:
        raise RuntimeError("no active ParamStore (ops on parameters must run inside a model forward)")
    return st


class using_store:
    def __init__(self, store: ParamStore):
        self.store = store

    def __enter__(self):
        self.prev = _state.store
        _state.store = self.store
        self.prev_stream = (_state.main_stream, _state.main_handle)
        if self.store.flat.is_cuda:
            ms = torch.cuda.current_stream()
            _state.main_stream, _state.main_handle = ms, ms.cuda_stream
        _bind_conv_workspace(self.store.flat.device)
        return self.store

    def __exit__(self, *exc):
        _state.store = self.prev
        _state.main_stream, _state.main_handle = self.prev_stream
        return False


def pgrad(p: torch.nn.Parameter) -> torch.Tensor:
    return current_store().grad_of(p)


# ---------------------------------------------------------------------------
# packed weights cache (re-packed when the store version changes)
# ---------------------------------------------------------------------------

class PackedWeight:
    """Packed copies of one weight tensor for the implicit-GEMM kernels (forward / bwd-data)."""

    __slots__ = ("fwd", "bwd", "fwd16", "bwd16", "version", "store_id")

    def __init__(self):
        self.fwd = None
        self.bwd = None
        self.fwd16 = None  # bf16 MFMA-fragment copies (mixed-precision path)
        self.bwd16 = None
        self.version = -1
        self.store_id = 0


def _pack(fmt: PackFormat, w: torch.Tensor, T_: int, K: int, N: int, sk: int, sn: int, st: int) -> torch.Tensor:
    """Pack now (first use) into a persistent buffer and register it for the batched per-step repack."""
    out = _alloc(fmt.elems(T_, K, N), fmt.dtype, w.device)
    _lib.call(fmt.pack, w.data_ptr(), out.data_ptr(), T_, K, N, sk, sn, st, _stream())
    current_store().register_pack(fmt, out, w, T_, K, N, sk, sn, st)
    return out


def _bwd_data_dims(T_: int, K: int, N: int, sk: int, sn: int, st: int) -> T.Tuple[int, int, int, int, int, int]:
    """The backward-data copy of a weight is the forward copy (T, K, N, sk, sn, st) with K and N exchanged."""
    return (T_, N, K, sn, sk, st)


def _pack_copies(fmt: PackFormat, w: torch.Tensor, fwd: T.Optional[torch.Tensor], bwd: T.Optional[torch.Tensor],
                 need_bwd: bool, *dims: int) -> T.Tuple[torch.Tensor, T.Optional[torch.Tensor]]:
    """(forward, backward-data) copies of ``w`` in one format: those given, the missing ones packed from the forward
    ``dims`` (the backward-data copy only when asked for)."""
    if fwd is None:
        fwd = _pack(fmt, w, *dims)
    if need_bwd and bwd is None:
        bwd = _pack(fmt, w, *_bwd_data_dims(*dims))
    return fwd, bwd


def _sync_packs(pw: "PackedWeight") -> None:
    """Bring all registered packed weights up to date if the parameters changed since the last pack."""
    st = current_store()
    if pw.store_id != st.uid:  # parameters were re-flattened into a new store: drop copies of the old one
        pw.fwd = pw.bwd = pw.fwd16 = pw.bwd16 = None
        pw.store_id = st.uid
    if st.packed_version != st.version:
        st.repack_all()


def _holder(mod) -> PackedWeight:
    """The module's PackedWeight (created at first use), its registered copies current."""
    pw = mod.__dict__.get("_cn_packed")
    if pw is None:
        pw = PackedWeight()
        mod.__dict__["_cn_packed"] = pw
    _sync_packs(pw)
    return pw


def _fill(pw: PackedWeight, w: torch.Tensor, need_bwd: bool, bf16: bool, *dims: int) -> PackedWeight:
    """The holder with the copies of one precision that a caller needs (forward ``dims``)."""
    if bf16:
        pw.fwd16, pw.bwd16 = _pack_copies(PACK_BF16, w, pw.fwd16, pw.bwd16, need_bwd, *dims)
    else:
        pw.fwd, pw.bwd = _pack_copies(PACK_F32, w, pw.fwd, pw.bwd, need_bwd, *dims)
    return pw


def packed_conv(mod, need_bwd: bool, bf16: bool = False) -> PackedWeight:
    """Packed weights of an nn.Conv2d / nn.Linear-like module (weight [Cout][Cin][KH][KW])."""
    w = mod.weight
    cout, cin = w.shape[0], w.shape[1]
    taps = int(w[0, 0].numel()) if w.dim() > 2 else 1
    return _fill(_holder(mod), w, need_bwd, bf16, taps, cin, cout, taps, cin * taps, 1)


def packed_convT(mod, need_bwd: bool, bf16: bool = False, taps_as_channels: bool = False) -> PackedWeight:
    """Packed weights of an nn.ConvTranspose2d (weight [Cin][Cout][KH][KW]). ``taps_as_channels`` (fp32, stride >=
    kernel size, _conv_transpose2d_taps): the tensor as the [Cin][Cout*KH*KW] matrix of a 1x1 transposed convolution."""
    w = mod.weight
    cin, cout = w.shape[0], w.shape[1]
    taps = int(w[0, 0].numel())
    if taps_as_channels and not bf16:
        n = cout * taps
        return _fill(_holder(mod), w, need_bwd, False, 1, cin, n, n, 1, 0)
    return _fill(_holder(mod), w, need_bwd, bf16, taps, cin, cout, cout * taps, taps, 1)
