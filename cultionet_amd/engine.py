"""Execution engine of cultionet_amd: a reverse-mode tape whose every node is a HIP kernel launch.

PyTorch is used for device memory (caching allocator), streams and parameter containers only;
all arithmetic runs in libcultionet_hip.so through the C ABI (cultionet_amd._lib). There is no
CPU path: calling any op without the HIP library or with CPU tensors raises.

Design (MI355X-first, not torch.autograd):
  * ``Var`` = a device buffer (+ its gradient buffer). Buffers are NCHW fp32; a Var may be a channel
    slice of a bigger buffer (batch stride != C*H*W), which every kernel supports natively.
  * forward ops append a closure to the tape; ``Tape.backward()`` walks it in reverse. Gradient
    buffers are written with beta=0 by the first producer and accumulated in-kernel (beta=1) by
    later ones, or aliased when an op is the identity on its gradient (residual adds, concat
    slices): no separate add/copy kernels.
  * parameters live in ONE flat fp32 buffer and so do their gradients (``ParamStore``): the optimizer
    is one fused launch and data-parallel all-reduce buckets are plain slices of the flat gradient.

This module holds the ops of both precisions. What they stand on lives in four modules, each importing only from those
before it: ``runtime`` (thread state, streams, allocator), ``params`` (ParamStore, weight packs), ``scratch`` (deferred
slice sums, scratch pools), ``tape`` (Var, Tape, spawn / join). Their names are re-bound here: ``engine`` is the name
the rest of the package uses.
"""
from __future__ import annotations

import contextlib
import ctypes
import struct
import typing as T

import torch

from . import _lib, runtime
# The infrastructure the ops stand on, bottom layer first; each module imports only from those above it. Their names are
# re-bound here so that ``engine.<name>`` keeps resolving for the rest of the package, the tools and the tests.
from .runtime import (  # noqa: F401
    _alloc, alloc, _alloc_like, _aux_stream, _aux_streams, bf16_enabled, branch_streams, branch_streams_allowed,
    bstride, _check, _dense16, _dense_inner, holding_allocations, _HW_QUEUE_BUDGET, _hw_queue_cap, is16,
    join_side_stream, _KeepAlive, _keepalive, ld, _main_stream, mixed_precision, _new, new_buffer,
    overlap_wgrad, _priority_stream, _py_op, _rows, _side_state, side_stream, side_stream_event, _side_streams,
    _state, _stream)
from .params import (  # noqa: F401
    _bind_conv_workspace, _bump_ws_epoch, _bwd_data_dims, _conv_ws, _CONV_WS_FLOATS, current_store, _fill,
    _holder, _pack, PACK_BF16, _pack_copies, PACK_F32, _pack_record_bf16, _pack_record_f32, packed_conv,
    packed_convT, PackedWeight, PackFormat, ParamStore, pgrad, SEG_CHUNK, segment_table, select_packs,
    _SUB_TABLES_KEPT, _sync_packs, trainable_segments, using_store, workspace_epoch)
from .scratch import (  # noqa: F401
    _bn_group_ws16, _bn_ws16, _bng_ws, deferring_slice_sums, flush_slice_sums, _grown, _pad_ws, _pretime_ws,
    _pt_ws, _SliceSums, _SS_BLOCK, _SS_CAP, _SS_FLUSH_FLOATS, _ss_state, _sum_stream, _ws16, _WS16_MAX_FLOATS,
    _WS_FLOATS, _zeroed_scratch)
from .tape import (  # noqa: F401
    aux_stream_events, begin_branch_backward, _Branch, current_tape, give_grad, grad_buffer, join, recording,
    release_branches, _req, spawn, Tape, _tr, Var)


def __getattr__(name: str):
    """``_OVERLAP_WGRAD`` and ``_recorder`` are rebound at run time and live in ``runtime``: a copy bound here at import
    would go stale, so reads of ``engine.<flag>`` are forwarded (PEP 562)."""
    if name in ("_OVERLAP_WGRAD", "_recorder"):
        return getattr(runtime, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ---------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------

def conv2d(x: Var, mod, stride: int = 1, padding: int = 0, dilation: int = 1, out: T.Optional[torch.Tensor] = None,
           want_stats: bool = False, bn=None) -> Var:
    """nn.Conv2d forward (+ tape node for bwd-data, bwd-weight, bias grad). ``bn``: the BatchNorm2d that follows (training
    mode, mixed precision): the conv launch finishes its batch statistics when it can (see _bnstats_launch)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt):
        return _conv2d_bf16(x, mod, stride, padding, dilation, out, want_stats, bn)
    B, Cin, H, W = xt.shape
    w = mod.weight
    Cout = w.shape[0]
    KH, KW = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    Ho = (H + 2 * padding - dilation * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * padding - dilation * (KW - 1) - 1) // stride + 1
    pw = packed_conv(mod, tape.enabled and x.req)
    y = out if out is not None else _new((B, Cout, Ho, Wo), xt)
    bias = mod.bias
    _lib.call("cn_conv2d_fwd_f32", xt.data_ptr(), bstride(xt), pw.fwd.data_ptr(),
              bias.data_ptr() if bias is not None else None, y.data_ptr(), bstride(y), B, Cin, H, W, Cout, KH, KW,
              stride, padding, dilation, 0, _stream())
    yv = Var(y, _req(tape, (x,), (w, bias)))
    if yv.req:
        store = current_store()
        gw, gb = _tr(w), _tr(bias)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            if gw or gb:
                with side_stream(xt, dy):
                    s = _stream()
                    if gw:
                        wsp, wsn = _pad_ws(xt, dy)
                        _lib.call("cn_conv2d_bwd_weight_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(), bstride(dy),
                                  store.grad_of(w).data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, padding, dilation,
                                  wsp, wsn, s)
                    if gb:
                        _lib.call("cn_channel_sum_f32", dy.data_ptr(), bstride(dy), B, Cout, Ho * Wo,
                                  store.grad_of(bias).data_ptr(), 1, s)
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv2d_bwd_data_f32", dy.data_ptr(), bstride(dy), pw.bwd.data_ptr(), dx.data_ptr(),
                          bstride(dx), B, Cin, H, W, Cout, KH, KW, stride, padding, dilation, acc, _stream())
            yv.grad = None

        tape.add(bwd, (w, bias))
    return yv


def conv2d_group(xs: T.Sequence[Var], mods: T.Sequence, paddings: T.Sequence[int], dilations: T.Sequence[int],
                 stride: int = 1, bns: T.Optional[T.Sequence] = None) -> T.List[Var]:
    """G (<= 4) nn.Conv2d of identical shapes (per-conv padding / dilation) in ONE implicit-GEMM launch -- the
    dilation branches of ResidualAConv. ``xs`` may repeat one Var (branches sharing their input: backward sums the
    G input gradients in the same launch). Weight gradients stay one launch per conv."""
    tape = current_tape()
    G = len(mods)
    xts = [_check(x.t) for x in xs]
    if is16(xts[0]):  # mixed precision: one grouped launch, each conv with BatchNorm statistics rows from its epilogue
        return _conv2d_group_bf16(xs, mods, paddings, dilations, stride, bns)
    B, Cin, H, W = xts[0].shape
    w0 = mods[0].weight
    Cout, KH, KW = w0.shape[0], w0.shape[2], w0.shape[3]
    for xt, m in zip(xts, mods):
        if tuple(xt.shape) != (B, Cin, H, W) or tuple(m.weight.shape) != tuple(w0.shape) or bstride(xt) != bstride(xts[0]):
            raise ValueError("conv2d_group: all inputs / weights must have the same shape")
    Ho = (H + 2 * paddings[0] - dilations[0] * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * paddings[0] - dilations[0] * (KW - 1) - 1) // stride + 1
    shared_in = all(x is xs[0] for x in xs)
    need_bwd = tape.enabled and any(x.req for x in xs)
    pws = [packed_conv(m, need_bwd) for m in mods]
    ys = [_new((B, Cout, Ho, Wo), xts[0]) for _ in range(G)]
    biases = [m.bias for m in mods]
    has_bias = biases[0] is not None
    tab = lambda ptrs: (ctypes.c_void_p * G)(*ptrs)
    pads_c = (ctypes.c_int * G)(*paddings)
    dils_c = (ctypes.c_int * G)(*dilations)
    _lib.call("cn_conv2d_fwd_grouped_f32", G, tab([t.data_ptr() for t in xts]), bstride(xts[0]),
              tab([p.fwd.data_ptr() for p in pws]), tab([b.data_ptr() for b in biases]) if has_bias else None,
              tab([y.data_ptr() for y in ys]), bstride(ys[0]), B, Cin, H, W, Cout, KH, KW, stride, pads_c, dils_c, 0,
              _stream())
    req = _req(tape, xs, [m.weight for m in mods] + biases)
    yvs = [Var(y, req) for y in ys]
    if req:
        store = current_store()
        # one flag for the group (the grouped weight-gradient launch writes every member; a frozen member's slice is
        # written and never read)
        gw = any(_tr(m.weight) for m in mods) or any(_tr(b) for b in biases)

        def bwd():
            live = [i for i in range(G) if yvs[i].grad is not None]
            grouped_w = (len(live) == G and len(set(paddings)) == 1 and len(set(dilations)) == 1
                         and len({bstride(yvs[i].grad) for i in live}) == 1)
            with side_stream(*(list(xts) + [yvs[i].grad for i in live])) if gw else contextlib.nullcontext():
                s = _stream()
                if grouped_w and gw:  # one launch for the G weight gradients
                    wsp, wsn = _pad_ws(*([xts[i] for i in range(G)] + [yvs[i].grad for i in range(G)]))
                    _lib.call("cn_conv2d_bwd_weight_grouped_f32", G, tab([t.data_ptr() for t in xts]), bstride(xts[0]),
                              tab([yvs[i].grad.data_ptr() for i in range(G)]), bstride(yvs[0].grad),
                              tab([store.grad_of(m.weight).data_ptr() for m in mods]), B, Cin, H, W, Cout, KH, KW,
                              stride, paddings[0], dilations[0], wsp, wsn, s)
                for i in (live if gw else ()):
                    dy, m, xt = yvs[i].grad, mods[i], xts[i]
                    if grouped_w:
                        if has_bias:
                            _lib.call("cn_channel_sum_f32", dy.data_ptr(), bstride(dy), B, Cout, Ho * Wo,
                                      store.grad_of(m.bias).data_ptr(), 1, s)
                        continue
                    wsp, wsn = _pad_ws(xt, dy)
                    _lib.call("cn_conv2d_bwd_weight_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(), bstride(dy),
                              store.grad_of(m.weight).data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, paddings[i],
                              dilations[i], wsp, wsn, s)
                    if has_bias:
                        _lib.call("cn_channel_sum_f32", dy.data_ptr(), bstride(dy), B, Cout, Ho * Wo,
                                  store.grad_of(m.bias).data_ptr(), 1, s)
            s = _stream()
            todo = [i for i in live if xs[i].req]
            if todo:
                bufs = []
                if shared_in:
                    dx, acc = grad_buffer(xs[0])
                    bufs = [(dx, acc)] * len(todo)
                else:
                    bufs = [grad_buffer(xs[i]) for i in todo]
                accs = {a for _, a in bufs}
                dybs = {bstride(yvs[i].grad) for i in todo}
                dxbs = {bstride(d) for d, _ in bufs}
                if len(todo) == G and len(accs) == 1 and len(dybs) == 1 and len(dxbs) == 1:
                    dyp = [yvs[i].grad.data_ptr() for i in todo]
                    wpp = [p.bwd.data_ptr() for p in pws]
                    dxp = [d.data_ptr() for d, _ in bufs]
                    khs, kws, pds, dls = [KH] * G, [KW] * G, list(paddings), list(dilations)
                    n = len(dyp)
                    ptab = lambda ptrs: (ctypes.c_void_p * n)(*ptrs)
                    itab = lambda v: (ctypes.c_int * n)(*v)
                    _lib.call("cn_conv2d_bwd_data_grouped_f32", n, ptab(dyp), dybs.pop(), ptab(wpp), ptab(dxp),
                              dxbs.pop(), B, Cin, H, W, Cout, itab(khs), itab(kws), stride, itab(pds), itab(dls),
                              accs.pop(), s)
                else:  # mixed accumulate flags / strides: conv by conv
                    first = True
                    for i, (d, a) in zip(todo, bufs):
                        dy = yvs[i].grad
                        _lib.call("cn_conv2d_bwd_data_f32", dy.data_ptr(), bstride(dy), pws[i].bwd.data_ptr(),
                                  d.data_ptr(), bstride(d), B, Cin, H, W, Cout, KH, KW, stride, paddings[i],
                                  dilations[i], a if (first or not shared_in) else 1, s)
                        first = False
            for v in yvs:
                v.grad = None

        tape.add(bwd, tuple(m.weight for m in mods) + tuple(b for b in biases if b is not None))
    return yvs


def _conv_transpose2d_taps(x: Var, mod, stride: int, padding: int, size, out: T.Optional[torch.Tensor]) -> Var:
    """nn.ConvTranspose2d(k, stride s >= k, padding) FOLLOWED BY check_upsample to ``size`` (None: no resize), fp32: no
    two taps of an input pixel meet, so the contraction is a dense 1x1 GEMM on the small grid into
    P [B, Cout*k*k, H, W] (the weight tensor viewed as [Cin][Cout*k*k]) and one pointwise pass writes
    resize(bias + scatter(P)); backward: dP = gather(resize^T(dz)) in one pass, then the 1x1 data / weight gradients (the
    weight gradient lands in the parameter's own [Cin][Cout][k][k] layout). Returns the RESIZED tensor (csrc/cn_pointwise.hip,
    cn_convt_taps_*; convolution.py:45-68 + unet_parts.py:227-309 of the reference)."""
    tape = current_tape()
    xt = x.t
    B, Cin, H, W = xt.shape
    w = mod.weight
    Cout, K = w.shape[1], w.shape[2]
    KK = K * K
    Hy = (H - 1) * stride - 2 * padding + K
    Wy = (W - 1) * stride - 2 * padding + K
    Ho, Wo = (int(size[0]), int(size[1])) if size is not None else (Hy, Wy)
    pw = packed_convT(mod, tape.enabled and x.req, taps_as_channels=True)
    P = _new((B, Cout * KK, H, W), xt)
    _lib.call("cn_conv_transpose2d_fwd_f32", xt.data_ptr(), bstride(xt), pw.fwd.data_ptr(), None, P.data_ptr(),
              bstride(P), B, Cin, H, W, Cout * KK, 1, 1, 1, 0, 0, 0, _stream())
    z = out if (out is not None and tuple(out.shape) == (B, Cout, Ho, Wo)) else _new((B, Cout, Ho, Wo), xt)
    bias = mod.bias
    _lib.call("cn_convt_taps_fwd_f32", P.data_ptr(), bstride(P), bias.data_ptr() if bias is not None else None,
              z.data_ptr(), bstride(z), B, Cout, H, W, K, stride, padding, Ho, Wo, _stream())
    del P  # (not needed by the backward pass)
    zv = Var(z, _req(tape, (x,), (w, bias)))
    if zv.req:
        store = current_store()
        gw, gb = _tr(w), _tr(bias)

        def bwd():
            dz = zv.grad
            if dz is None:
                return
            if gw or x.req:  # (a bias gradient alone needs only dz)
                dP = _new((B, Cout * KK, H, W), xt)
                _lib.call("cn_convt_taps_bwd_f32", dz.data_ptr(), bstride(dz), dP.data_ptr(), bstride(dP), B, Cout, H,
                          W, K, stride, padding, Ho, Wo, _stream())
            if gw or gb:
                with side_stream(xt, dP, dz) if gw else side_stream(xt, dz):
                    s = _stream()
                    if gw:
                        wsp, wsn = _pad_ws(xt, dP)
                        _lib.call("cn_conv_transpose2d_bwd_weight_f32", xt.data_ptr(), bstride(xt), dP.data_ptr(),
                                  bstride(dP), store.grad_of(w).data_ptr(), B, Cin, H, W, Cout * KK, 1, 1, 1, 0, 0, wsp,
                                  wsn, s)
                    if gb:  # the resize weights of every output pixel sum to one: sum of dz
                        _lib.call("cn_channel_sum_f32", dz.data_ptr(), bstride(dz), B, Cout, Ho * Wo,
                                  store.grad_of(bias).data_ptr(), 1, s)
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv_transpose2d_bwd_data_f32", dP.data_ptr(), bstride(dP), pw.bwd.data_ptr(),
                          dx.data_ptr(), bstride(dx), B, Cin, H, W, Cout * KK, 1, 1, 1, 0, 0, acc, _stream())
            zv.grad = None

        tape.add(bwd, (w, bias))
    return zv


def conv_transpose2d(x: Var, mod, stride: int, padding: int, size: T.Optional[T.Tuple[int, int]] = None,
                     out: T.Optional[torch.Tensor] = None) -> Var:
    """nn.ConvTranspose2d forward (k x k, stride s, padding p, with bias), then check_upsample (convolution.py:45-68):
    with ``size`` given the result is the tensor at ``size``, bilinearly resized (into ``out`` when given) unless the
    natural output already has that size -- then it is returned as computed, and a caller that passed ``out`` copies.

    When ``size`` exceeds the natural (2n-1)-style output by less than the stride on both axes (every site of
    TowerUNet), the fp32 transposed convolution is computed on THAT grid -- output_padding = size - natural, whose
    top-left natural-size block is exactly the reference's tensor -- and the resize reads the image inside it in place:
    planes of 100 x 100 / 50 x 50 are 16-byte aligned where 99 x 99 / 49 x 49 / 97 x 97 are not, so the weight gradient
    needs no aligned copy of dy (cn_pad_planes) and the data gradient stages 16 bytes per lane instead of 4. A stride
    >= kernel size (final_c's 3 x 3, stride 4) takes _conv_transpose2d_taps, which resizes in its own pointwise pass."""
    xt = _check(x.t)
    B, Cin, H, W = xt.shape
    w = mod.weight
    Cout, KH, KW = w.shape[1], w.shape[2], w.shape[3]
    Ho = (H - 1) * stride - 2 * padding + KH
    Wo = (W - 1) * stride - 2 * padding + KW
    if is16(xt):
        y = _conv_transpose2d_bf16(x, mod, stride, padding)
    elif KH == KW and stride >= KH and 0 <= padding < stride and \
            (size is None or (2 * Ho > int(size[0]) and 2 * Wo > int(size[1]))):
        return _conv_transpose2d_taps(x, mod, stride, padding, size, out)
    else:
        op = 0
        if size is not None and stride > 1:
            dh, dw_ = int(size[0]) - Ho, int(size[1]) - Wo
            if dh == dw_ and 0 < dh < stride:
                op = dh
        y = _conv_transpose2d_f32(x, mod, stride, padding, op)
    if size is None or (Ho, Wo) == (int(size[0]), int(size[1])):
        return y
    return _resize_bilinear(y, (Ho, Wo), (int(size[0]), int(size[1])), out)


def _conv_transpose2d_f32(x: Var, mod, stride: int, padding: int, op: int) -> Var:
    """The fp32 transposed convolution with output_padding ``op``: the natural output plus ``op`` rows and columns."""
    tape = current_tape()
    xt = x.t
    B, Cin, H, W = xt.shape
    w = mod.weight
    Cout, KH, KW = w.shape[1], w.shape[2], w.shape[3]
    Hs = (H - 1) * stride - 2 * padding + KH + op  # the stored grid
    Ws = (W - 1) * stride - 2 * padding + KW + op
    pw = packed_convT(mod, tape.enabled and x.req)
    y = _new((B, Cout, Hs, Ws), xt)
    bias = mod.bias
    _lib.call("cn_conv_transpose2d_fwd_f32", xt.data_ptr(), bstride(xt), pw.fwd.data_ptr(),
              bias.data_ptr() if bias is not None else None, y.data_ptr(), bstride(y), B, Cin, H, W, Cout, KH, KW,
              stride, padding, op, 0, _stream())
    yv = Var(y, _req(tape, (x,), (w, bias)))
    if yv.req:
        store = current_store()
        gw, gb = _tr(w), _tr(bias)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            if gw or gb:
                with side_stream(xt, dy):
                    s = _stream()
                    if gw:
                        wsp, wsn = _pad_ws(xt, dy)
                        _lib.call("cn_conv_transpose2d_bwd_weight_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(),
                                  bstride(dy), store.grad_of(w).data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, padding,
                                  op, wsp, wsn, s)
                    if gb:  # (the padding of dy is zero: the resize adjoint writes it)
                        _lib.call("cn_channel_sum_f32", dy.data_ptr(), bstride(dy), B, Cout, Hs * Ws,
                                  store.grad_of(bias).data_ptr(), 1, s)
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv_transpose2d_bwd_data_f32", dy.data_ptr(), bstride(dy), pw.bwd.data_ptr(),
                          dx.data_ptr(), bstride(dx), B, Cin, H, W, Cout, KH, KW, stride, padding, op, acc, _stream())
            yv.grad = None

        tape.add(bwd, (w, bias))
    return yv


def time_conv(x: Var, mod, tin: int) -> Var:
    """nn.Conv3d(kernel (k,1,1), bias=False) on x viewed as [B, Cin*Tin, H, W] -> [B, Cout*Tout, H, W]."""
    tape = current_tape()
    xt = _check(x.t)
    B, CT, H, W = xt.shape
    w = mod.weight  # [Cout, Cin, k, 1, 1]
    Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]
    assert CT == Cin * tin
    tout = tin - k + 1
    ver = current_store().version
    pw = mod.__dict__.get("_cn_packed")
    if pw is None or pw.version != ver or pw.store_id != current_store().uid:
        pw = PackedWeight()
        pw.version = ver
        pw.store_id = current_store().uid
        mod.__dict__["_cn_packed"] = pw
    if pw.fwd is None:
        n = _lib.query("cn_conv_kpad", Cin * tin) * _lib.query("cn_conv_npad", Cout * tout)
        pw.fwd = _new((n,), xt)
        _lib.call("cn_pack_timeconv_f32", w.data_ptr(), pw.fwd.data_ptr(), Cout, Cin, tin, k, 0, _stream())
    if tape.enabled and x.req and pw.bwd is None:
        n = _lib.query("cn_conv_kpad", Cout * tout) * _lib.query("cn_conv_npad", Cin * tin)
        pw.bwd = _new((n,), xt)
        _lib.call("cn_pack_timeconv_f32", w.data_ptr(), pw.bwd.data_ptr(), Cout, Cin, tin, k, 1, _stream())
    y = _new((B, Cout * tout, H, W), xt)
    _lib.call("cn_conv2d_fwd_f32", xt.data_ptr(), bstride(xt), pw.fwd.data_ptr(), None, y.data_ptr(), bstride(y), B,
              CT, H, W, Cout * tout, 1, 1, 1, 0, 1, 0, _stream())
    yv = Var(y, _req(tape, (x,), (w,)))
    if yv.req:
        store = current_store()
        gw = _tr(w)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            if gw:
                with side_stream(xt, dy):
                    s = _stream()
                    dwexp = _alloc(Cout * tout * CT, torch.float32, xt.device)
                    _lib.call("cn_fill_f32", dwexp.data_ptr(), dwexp.numel(), 0.0, s)
                    _lib.call("cn_conv2d_bwd_weight_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(), bstride(dy),
                              dwexp.data_ptr(), B, CT, H, W, Cout * tout, 1, 1, 1, 0, 1, None, 0, s)
                    _lib.call("cn_fold_timeconv_grad_f32", dwexp.data_ptr(), store.grad_of(w).data_ptr(), Cout, Cin,
                              tin, k, s)
                    if runtime._OVERLAP_WGRAD:
                        dwexp.record_stream(_side_state(xt.device)["stream"])
            s = _stream()
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv2d_bwd_data_f32", dy.data_ptr(), bstride(dy), pw.bwd.data_ptr(), dx.data_ptr(),
                          bstride(dx), B, CT, H, W, Cout * tout, 1, 1, 1, 0, 1, acc, s)
            yv.grad = None

        tape.add(bwd, (w,))
    return yv


# The fused PreTimeReduction family (csrc/cn_pretime.hip) serves training and inference (forward 3
# launches / 1 in eval mode instead of ~20, backward 3 instead of ~20; same-box A/B in round 4 against the op-by-op
# path: bf16 batch 32 at parity, fp32 batch 8 +1 %, 32 / 29 launches fewer per step).


def pretime_reduction(x: Var, pre, in_channels: int, in_time: int) -> T.Optional[Var]:
    """PreTimeReduction (models/nunet.py:60-105) through the fused kernel family cn_pretime_*: both Conv3d stacks, their
    BatchNorm3d / BatchNorm2d, the branch sum and the LayerNorm, recomputed from x in every pass (3 launches forward in
    training, 1 in inference, 3 backward on the compute stream: the stage has parameter gradients only).
    Writes fp32 NCHW, or bf16 NHWC directly when the mixed-precision region is on. Returns None for shapes / settings the
    fused kernels do not cover (the caller keeps the generic op-by-op path)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt) or x.req or not xt.is_contiguous():
        return None
    B, CT, H, W = xt.shape
    C, Tn = in_channels, in_time
    br = (pre.conv3, pre.conv5)
    ln = pre.layer_norm[1]
    Cout = ln.weight.shape[0]
    HW = H * W
    training = bool(pre.training)
    bn3 = [b.seq[1] for b in br]
    bn2 = [b.seq[5] for b in br]
    if CT != C * Tn or any(b.momentum is None for b in bn3 + bn2) or \
            bn3[0].eps != bn3[1].eps or bn2[0].eps != bn2[1].eps or bn3[0].momentum != bn3[1].momentum or \
            bn2[0].momentum != bn2[1].momentum or any(b.running_mean is None for b in bn3 + bn2) or \
            any(b.training != training for b in bn3 + bn2):
        return None
    glist = []
    for b, b3, b2 in zip(br, bn3, bn2):
        glist += [b.seq[0].weight, b.seq[3].weight, b3.weight, b3.bias, b2.weight, b2.bias]
    glist += [ln.weight, ln.bias]
    req = _req(tape, (), glist)  # (the stage has parameter gradients only; a frozen one records nothing)
    with_bwd = 1 if req else 0
    need = int(_lib.query("cn_pretime_workspace_floats", B, C, Tn, HW, Cout, with_bwd))
    if need < 0:
        return None
    dev = xt.device
    bf16 = bf16_enabled()
    if bf16:
        y = _alloc((B, H, W, Cout), torch.bfloat16, dev).permute(0, 3, 1, 2)
        ystride, kind = Cout, 1
    else:
        y = _alloc((B, Cout, H, W), torch.float32, dev)
        ystride, kind = Cout * HW, 0
    plist = []
    for b, b3, b2 in zip(br, bn3, bn2):
        plist += [b.seq[0].weight, b.seq[3].weight, b3.weight, b3.bias, b3.running_mean, b3.running_var, b2.weight,
                  b2.bias, b2.running_mean, b2.running_var]
    plist += [ln.weight, ln.bias]
    params = (ctypes.c_void_p * 22)(*[t.data_ptr() for t in plist])
    stats_t = _alloc(2 * (2 * C + 2 * Cout), torch.float32, dev)
    offs, o = [], 0
    for _ in range(2):
        for n in (C, C, Cout, Cout):
            offs.append(o)
            o += n
    stats = (ctypes.c_void_p * 8)(*[stats_t[i:].data_ptr() for i in offs])
    bnc = (ctypes.c_float * 4)(float(bn3[0].eps), float(bn3[0].momentum), float(bn2[0].eps), float(bn2[0].momentum))
    _note_bn_update(training)
    ws = _pretime_ws(need, dev)
    _lib.call("cn_pretime_fwd_f32", xt.data_ptr(), bstride(xt), params, stats, y.data_ptr(), ystride, kind, B, C, Tn, HW,
              Cout, 1 if training else 0, bnc, float(ln.eps), ws.data_ptr(), ws.numel(), _stream())
    yv = Var(y, req)
    if req:
        store = current_store()

        def bwd(stats_t=stats_t):  # (``stats`` points into stats_t: held until the backward has run)
            dy = yv.grad
            if dy is None:
                return
            if bf16:
                dstride = ld(dy)
                if not _dense16(dy):
                    raise RuntimeError("pretime_reduction: the output gradient must be a dense NHWC buffer")
            else:
                if not _dense_inner(dy):  # (a channel slice of a concat gradient: batch stride > Cout * HW is fine)
                    raise RuntimeError("pretime_reduction: the output gradient must be NCHW with dense planes")
                dstride = bstride(dy)
            grads = (ctypes.c_void_p * 14)(*[store.grad_of(p).data_ptr() for p in glist])
            # parameter gradients only, and the LAST node of the backward. On the compute stream: the weight-gradient
            # stream still holds the encoder's 100 x 100 weight gradients at this point, behind which these three
            # launches would queue (measured 1 % slower end to end; that variant was removed)
            wsb = _pretime_ws(need, dev)
            _lib.call("cn_pretime_bwd_f32", xt.data_ptr(), bstride(xt), params, stats, dy.data_ptr(), dstride, kind,
                      grads, B, C, Tn, HW, Cout, 1 if training else 0, bnc, float(ln.eps), wsb.data_ptr(), wsb.numel(),
                      _stream())
            yv.grad = None

        tape.add(bwd, tuple(glist))
    return yv


ACT_NONE, ACT_SILU = 0, 1

# bumped by every train-mode BatchNorm forward (the kernels update running_mean / running_var in place, which torch's
# version counters do not see): invalidates the eval-mode folded weights below
_bn_stats_epoch = 0


def _note_bn_update(training: bool) -> None:
    global _bn_stats_epoch
    if training:
        _bn_stats_epoch += 1


def _bn_momentum(bn) -> float:
    """torch's momentum=None means a cumulative moving average (factor 1/num_batches_tracked, a device counter);
    the reference never configures it and the fused kernel takes a host scalar: refuse instead of guessing."""
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm(momentum=None) (cumulative average) has no HIP kernel; the reference "
                                  "uses the default momentum=0.1 everywhere")
    return float(bn.momentum)


def bn_act(x: Var, bn, act: int, residual: T.Optional[Var] = None, channels: T.Optional[int] = None,
           training: bool = True, out: T.Optional[torch.Tensor] = None) -> Var:
    """y = act(batch_norm(x)) (+ residual). x viewed as [B][C][L] with C = ``channels`` (BatchNorm3d: L = T*H*W)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt):
        if channels is not None and channels != xt.shape[1]:
            raise NotImplementedError("BatchNorm3d views are fp32-only (PreTimeReduction runs in fp32)")
        return _bn_act_bf16(x, bn, act, residual, training, out)
    B = xt.shape[0]
    C = channels if channels is not None else xt.shape[1]
    L = int(xt[0].numel()) // C
    dev = xt.device
    y = out if out is not None else _new(xt.shape, xt)
    mean = _new((C,), xt)
    rstd = _new((C,), xt)
    ws = _alloc(_lib.query("cn_bn_workspace_doubles", C), torch.float64, dev)
    rt = residual.t if residual is not None else None
    mom = _bn_momentum(bn)
    use_batch = training or (bn.running_mean is None)
    _note_bn_update(training)
    _lib.call("cn_bn_act_fwd_f32", xt.data_ptr(), bstride(xt), bn.weight.data_ptr(), bn.bias.data_ptr(),
              bn.running_mean.data_ptr() if bn.running_mean is not None else None,
              bn.running_var.data_ptr() if bn.running_var is not None else None,
              rt.data_ptr() if rt is not None else None, bstride(rt) if rt is not None else 0, y.data_ptr(),
              bstride(y), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), B, C, L, 1 if use_batch else 0, float(mom),
              float(bn.eps), act, _stream())
    gamma, beta = bn.weight, bn.bias
    # frozen gamma / beta with a live input: the fused kernel still writes their slices (never read)
    yv = Var(y, _req(tape, (x, residual), (gamma, beta)))
    if yv.req:
        store = current_store()

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            s = _stream()
            if residual is not None:
                give_grad(residual, dy)
            if x.req:
                dx, acc = grad_buffer(x)
                dxp, dxbs = dx.data_ptr(), bstride(dx)
            else:
                dxp, dxbs, acc = None, 0, 0
            _lib.call("cn_bn_act_bwd_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(), bstride(dy), mean.data_ptr(),
                      rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dxp, dxbs, store.grad_of(gamma).data_ptr(),
                      store.grad_of(beta).data_ptr(), None, ws.data_ptr(), B, C, L, 1 if use_batch else 0,
                      act, acc, 1, s)
            yv.grad = None

        tape.add(bwd, (gamma, beta))
    return yv


def _bn_group_uniform(bns: T.Sequence) -> bool:
    """Can one grouped launch serve these layers? It takes a single eps and momentum, and running statistics for
    every layer or for none."""
    return 1 <= len(bns) <= 4 and all(bn.momentum == bns[0].momentum and bn.eps == bns[0].eps for bn in bns) \
        and all((bn.running_mean is None) == (bns[0].running_mean is None) for bn in bns)


def bn_act_group(xs: T.Sequence[Var], bns: T.Sequence, act: int, residual: T.Optional[Var] = None,
                 sum_outputs: bool = False, training: bool = True,
                 outs: T.Optional[T.Sequence[torch.Tensor]] = None) -> T.Union[Var, T.List[Var]]:
    """G BatchNorm2d(+act) over G same-shaped tensors in one launch pair. ``sum_outputs``: returns the single Var
    ``residual + sum_g act(bn_g(x_g))`` (the ResUNet-a sum, accumulated in the order of the sequential form);
    otherwise the list of G activations."""
    tape = current_tape()
    G = len(xs)
    xts = [_check(x.t) for x in xs]
    if residual is not None and not sum_outputs:
        raise ValueError("bn_act_group: a residual needs sum_outputs=True")
    bf16 = is16(xts[0])
    if not _bn_group_uniform(bns) or \
            (bf16 and not all(tuple(t.shape) == tuple(xts[0].shape) and ld(t) == ld(xts[0]) and _dense16(t) for t in xts)):
        # the grouped kernels take ONE eps / momentum and running statistics for all layers or none (the bf16 ones also
        # dense NHWC inputs of one shape and pixel stride): other groups run one bn_act each; the summed form chains
        # the residual in the order of the fused sum
        if outs is not None and len(outs) != (1 if sum_outputs else G):
            raise ValueError("bn_act_group: outs must hold one tensor per output")
        if not sum_outputs:
            return [bn_act(x, bn, act, training=training, out=outs[i] if outs is not None else None)
                    for i, (x, bn) in enumerate(zip(xs, bns))]
        acc = residual
        for i, (x, bn) in enumerate(zip(xs, bns)):
            last = i == G - 1
            acc = bn_act(x, bn, act, residual=acc, training=training, out=outs[0] if outs is not None and last else None)
        return acc
    if bf16:  # mixed precision: the G branches in one launch per pass (cn_bn_act_group_*_bf16)
        return _bn_act_group_bf16(xs, bns, act, residual, sum_outputs, training, outs)
    B, C = xts[0].shape[0], xts[0].shape[1]
    L = int(xts[0][0].numel()) // C
    for t in xts:
        if tuple(t.shape) != tuple(xts[0].shape) or bstride(t) != bstride(xts[0]):
            raise ValueError("bn_act_group: inputs must have the same shape and strides")
    dev = xts[0].device
    use_batch = training or bns[0].running_mean is None
    _note_bn_update(training)
    tab = lambda ptrs: (ctypes.c_void_p * G)(*ptrs)
    if outs is not None:  # caller-provided outputs (e.g. channel slices of one buffer, all with the same strides)
        ys = list(outs)
        if len(ys) != (1 if sum_outputs else G) or any(bstride(y) != bstride(ys[0]) for y in ys):
            raise ValueError("bn_act_group: outs must match the outputs and share their batch stride")
    else:
        ys = [_new(xts[0].shape, xts[0])] if sum_outputs else [_new(xts[0].shape, xts[0]) for _ in range(G)]
    means = [_new((C,), xts[0]) for _ in range(G)]
    rstds = [_new((C,), xts[0]) for _ in range(G)]
    ws = _alloc(G * _lib.query("cn_bn_workspace_doubles", C), torch.float64, dev)
    rt = residual.t if residual is not None else None
    mom = _bn_momentum(bns[0])
    has_running = bns[0].running_mean is not None
    _lib.call("cn_bn_act_group_fwd_f32", G, tab([t.data_ptr() for t in xts]), bstride(xts[0]),
              tab([bn.weight.data_ptr() for bn in bns]), tab([bn.bias.data_ptr() for bn in bns]),
              tab([bn.running_mean.data_ptr() for bn in bns]) if has_running else None,
              tab([bn.running_var.data_ptr() for bn in bns]) if has_running else None,
              rt.data_ptr() if rt is not None else None, bstride(rt) if rt is not None else 0,
              (ctypes.c_void_p * len(ys))(*[y.data_ptr() for y in ys]) if not sum_outputs else tab([ys[0].data_ptr()] * G),
              bstride(ys[0]), tab([m.data_ptr() for m in means]), tab([r.data_ptr() for r in rstds]), ws.data_ptr(),
              B, C, L, 1 if use_batch else 0, float(mom), float(bns[0].eps), act, 1 if sum_outputs else 0, _stream())
    req = _req(tape, list(xs) + [residual], [bn.weight for bn in bns] + [bn.bias for bn in bns])
    yvs = [Var(y, req) for y in ys]
    if req:
        store = current_store()

        def bwd():
            s = _stream()
            if sum_outputs:
                dy = yvs[0].grad
                if dy is None:
                    return
                if residual is not None:
                    give_grad(residual, dy)
                dys = [dy] * G
            else:
                dys = [v.grad for v in yvs]
                if any(d is None for d in dys):
                    raise RuntimeError("bn_act_group: every output needs a gradient")
            bufs = [grad_buffer(x) if x.req else (None, 0) for x in xs]
            dxbs = {bstride(d) for d, _ in bufs if d is not None}
            dybs = {bstride(d) for d in dys}
            if len(dxbs) > 1 or len(dybs) > 1:
                raise RuntimeError("bn_act_group: gradient buffers must share their strides")
            _lib.call("cn_bn_act_group_bwd_f32", G, tab([t.data_ptr() for t in xts]), bstride(xts[0]),
                      tab([d.data_ptr() for d in dys]), dybs.pop(), tab([m.data_ptr() for m in means]),
                      tab([r.data_ptr() for r in rstds]), tab([bn.weight.data_ptr() for bn in bns]),
                      tab([bn.bias.data_ptr() for bn in bns]),
                      tab([d.data_ptr() if d is not None else None for d, _ in bufs]), dxbs.pop() if dxbs else 0,
                      (ctypes.c_int * G)(*[a for _, a in bufs]),
                      tab([store.grad_of(bn.weight).data_ptr() for bn in bns]),
                      tab([store.grad_of(bn.bias).data_ptr() for bn in bns]), ws.data_ptr(), B, C, L,
                      1 if use_batch else 0, act, 1, s)
            for v in yvs:
                v.grad = None

        tape.add(bwd, tuple(bn.weight for bn in bns) + tuple(bn.bias for bn in bns))
    return yvs[0] if sum_outputs else yvs


def _out_ok(out: T.Optional[torch.Tensor], like: torch.Tensor) -> bool:
    """May ``out`` (a channel slice of a concat buffer handed down by TowerUNet) receive a result shaped like ``like``?"""
    return (out is not None and tuple(out.shape) == tuple(like.shape) and out.dtype == like.dtype
            and out.device == like.device and (not is16(like) or (_dense16(out) and out.stride(1) == 1)))


LN_BWD_MAX_C = 512  # widest LayerNorm the backward kernels take (cn_ln_bwd_kernel<512> keeps C partial sums in LDS)


def layer_norm_c(x: Var, ln, residual: T.Optional[Var] = None, out: T.Optional[torch.Tensor] = None) -> Var:
    """nn.LayerNorm over the channel axis of an NCHW buffer (+ residual)."""
    tape = current_tape()
    xt = _check(x.t)
    if tape.enabled and xt.shape[1] > LN_BWD_MAX_C:
        # refused before the forward launch, not at the backward (the bf16 path falls back to this one for wide layers)
        raise NotImplementedError(f"LayerNorm backward over {xt.shape[1]} channels: cn_layernorm_c_bwd_f32 takes at "
                                  f"most {LN_BWD_MAX_C} (the forward alone, without a tape, runs at any width)")
    if is16(xt):
        return _layer_norm_c_bf16(x, ln, residual, out)
    B, C = xt.shape[0], xt.shape[1]
    L = int(xt[0, 0].numel())
    y = out if _out_ok(out, xt) and _dense_inner(out) else _new(xt.shape, xt)
    mu = _new((B, L), xt)
    rstd = _new((B, L), xt)
    rt = residual.t if residual is not None else None
    _lib.call("cn_layernorm_c_fwd_f32", xt.data_ptr(), bstride(xt), ln.weight.data_ptr(), ln.bias.data_ptr(),
              rt.data_ptr() if rt is not None else None, bstride(rt) if rt is not None else 0, y.data_ptr(),
              bstride(y), mu.data_ptr(), rstd.data_ptr(), B, C, L, float(ln.eps), _stream())
    yv = Var(y, _req(tape, (x, residual), (ln.weight, ln.bias)))
    if yv.req:
        store = current_store()

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            if residual is not None:
                give_grad(residual, dy)
            dx, acc = grad_buffer(x)
            nws = _lib.query("cn_layernorm_c_workspace_floats", B, C, L)
            ws = _alloc(max(nws, 1), torch.float32, xt.device)
            _lib.call("cn_layernorm_c_bwd_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(), bstride(dy),
                      ln.weight.data_ptr(), mu.data_ptr(), rstd.data_ptr(), dx.data_ptr(), bstride(dx),
                      store.grad_of(ln.weight).data_ptr(), store.grad_of(ln.bias).data_ptr(), B, C, L, acc,
                      ws.data_ptr(), nws, _stream())
            yv.grad = None

        tape.add(bwd, (ln.weight, ln.bias))
    return yv


def na2d(qkv: Var, heads: int, kernel_size: int, dilation: int, attn_drop: float = 0.0) -> Var:
    """Neighborhood attention core on a [B, 3C, H, W] qkv buffer -> [B, C, H, W]."""
    tape = current_tape()
    qt = _check(qkv.t)
    if is16(qt):
        return _na2d_bf16(qkv, heads, kernel_size, dilation, attn_drop)
    B, C3, H, W = qt.shape
    C = C3 // 3
    out = _new((B, C, H, W), qt)
    attn = _new((B, heads, kernel_size * kernel_size, H, W), qt)
    seed = _next_seed() if attn_drop > 0.0 else 0
    stepw = _step_word(qt.device).data_ptr() if attn_drop > 0.0 else None
    step_fwd = _rng["step"]
    _lib.call("cn_na2d_fwd_f32", qt.data_ptr(), bstride(qt), out.data_ptr(), bstride(out), attn.data_ptr(), B, C,
              heads, H, W, kernel_size, dilation, float(attn_drop), seed, stepw, _stream())
    ov = Var(out, _req(tape, (qkv,)))
    if ov.req:

        def bwd():
            do = ov.grad
            if do is None:
                return
            dattn = _alloc_like(attn)
            dq = _new(qt.shape, qt)
            _lib.call("cn_na2d_bwd_f32", qt.data_ptr(), bstride(qt), do.data_ptr(), bstride(do), attn.data_ptr(),
                      dattn.data_ptr(), dq.data_ptr(), bstride(dq), B, C, heads, H, W, kernel_size, dilation,
                      float(attn_drop), _bwd_seed(seed, step_fwd), stepw, _stream())
            if qkv.grad is None:
                qkv.grad = dq
            else:  # pragma: no cover - qkv has a single consumer in TowerUNet
                give_grad(qkv, dq)
            ov.grad = None

        tape.add(bwd)
    return ov


def spatial_channel_attention(skip: Var, out: Var, mod) -> Var:
    """out * (1 + gamma * 0.5 * (channel_attention(skip) + spatial_attention(skip))) -- SpatialChannelAttention
    (nn/modules/attention.py:89-126) applied the way ResidualAConv does (convolution.py:388-393).
    ``mod``: the host mirror with .channel_attention.fc1/.fc2 (Conv2d 1x1 pairs), .spatial_attention.conv, .gamma."""
    tape = current_tape()
    st, ot = _check(skip.t), _check(out.t)
    if is16(st):
        return _spatial_channel_attention_bf16(skip, out, mod)
    B, C, H, W = st.shape
    L = H * W
    Ch = C // 2
    dev = st.device
    fc1, fc2 = mod.channel_attention.fc1, mod.channel_attention.fc2
    w1a, w2a, w1m, w2m = fc1[0].weight, fc1[2].weight, fc2[0].weight, fc2[2].weight
    gamma = mod.gamma
    f = lambda *shape: _alloc(shape, torch.float32, dev)
    avg, mx, ca = f(B, C), f(B, C), f(B, C)
    hpre_a, hpre_m = f(B, Ch), f(B, Ch)
    idx = _alloc((B, C), torch.int32, dev)
    ccnt = _alloc((B, L), torch.int32, dev)  # channels tied at the channel maximum of every pixel
    pooled = f(B, 2, H, W)
    s = _stream()
    _lib.call("cn_sca_pool_fwd_f32", st.data_ptr(), bstride(st), B, C, L, avg.data_ptr(), mx.data_ptr(), idx.data_ptr(),
              pooled.data_ptr(), ccnt.data_ptr(), s)
    _lib.call("cn_sca_mlp_fwd_f32", avg.data_ptr(), mx.data_ptr(), w1a.data_ptr(), w2a.data_ptr(), w1m.data_ptr(),
              w2m.data_ptr(), hpre_a.data_ptr(), hpre_m.data_ptr(), ca.data_ptr(), B, C, Ch, s)
    # one flag for the whole block: its fused kernels write every parameter gradient of the block together (frozen
    # slices included, never read) whenever a gradient has to pass through it
    req = _req(tape, (skip, out), (w1a, w2a, w1m, w2m, gamma, mod.spatial_attention.conv.weight,
                                   mod.spatial_attention.conv.bias))
    pv = Var(pooled, req)
    shared = {}  # d ca handed from the apply node to the pooling node
    if req:
        store = current_store()

        def bwd_pool():  # recorded first => runs last: after the apply node and the 3x3 conv's backward
            dca = shared.pop("dca", None)
            if dca is None:
                return
            s2 = _stream()
            davg, dmx = f(B, C), f(B, C)
            _lib.call("cn_sca_mlp_bwd_f32", avg.data_ptr(), mx.data_ptr(), w1a.data_ptr(), w2a.data_ptr(),
                      w1m.data_ptr(), w2m.data_ptr(), hpre_a.data_ptr(), hpre_m.data_ptr(), ca.data_ptr(),
                      dca.data_ptr(), store.grad_of(w1a).data_ptr(), store.grad_of(w2a).data_ptr(),
                      store.grad_of(w1m).data_ptr(), store.grad_of(w2m).data_ptr(), davg.data_ptr(), dmx.data_ptr(),
                      B, C, Ch, s2)
            if skip.req:
                dpool = pv.grad
                if dpool is None:
                    dpool = _alloc_like(pooled)
                    _lib.call("cn_fill_f32", dpool.data_ptr(), dpool.numel(), 0.0, s2)
                dx, acc = grad_buffer(skip)
                _lib.call("cn_sca_pool_bwd_f32", st.data_ptr(), bstride(st), davg.data_ptr(), dmx.data_ptr(),
                          idx.data_ptr(), pooled.data_ptr(), dpool.data_ptr(), ccnt.data_ptr(), dx.data_ptr(),
                          bstride(dx), B, C, L, acc, s2)
            pv.grad = None

        tape.add(bwd_pool, (w1a, w2a, w1m, w2m))
    sconv = thin_conv3x3(pv, [mod.spatial_attention.conv], grouped=False)  # [B,1,H,W]
    y = _new(ot.shape, ot)
    _lib.call("cn_sca_apply_fwd_f32", ot.data_ptr(), bstride(ot), ca.data_ptr(), sconv.t.data_ptr(), gamma.data_ptr(),
              y.data_ptr(), bstride(y), B, C, L, s)
    yv = Var(y, req)
    if req:

        def bwd_apply():
            dy = yv.grad
            if dy is None:
                return
            s2 = _stream()
            dca, dsconv, scratch = f(B, C), f(B, 1, H, W), f(B * C)
            if out.req:
                do, acc = grad_buffer(out)
                dop, dobs = do.data_ptr(), bstride(do)
            else:
                dop, dobs, acc = None, 0, 0
            _lib.call("cn_sca_apply_bwd_f32", dy.data_ptr(), bstride(dy), ot.data_ptr(), bstride(ot), ca.data_ptr(),
                      sconv.t.data_ptr(), gamma.data_ptr(), dop, dobs, acc, dca.data_ptr(), dsconv.data_ptr(),
                      store.grad_of(gamma).data_ptr(), scratch.data_ptr(), B, C, L, s2)
            shared["dca"] = dca
            give_grad(sconv, dsconv)
            yv.grad = None

        tape.add(bwd_apply, (gamma,))
    return yv


def resize_bilinear(x: Var, size: T.Tuple[int, int], out: T.Optional[torch.Tensor] = None) -> Var:
    """F.interpolate(mode='bilinear', align_corners=True); identity when the size already matches."""
    Ho, Wo = int(size[0]), int(size[1])
    if tuple(x.shape[-2:]) == (Ho, Wo) and out is None:
        return x
    return _resize_bilinear(x, tuple(x.shape[-2:]), (Ho, Wo), out)


def _resize_bilinear(x: Var, image: T.Tuple[int, int], size: T.Tuple[int, int], out: T.Optional[torch.Tensor]) -> Var:
    """resize_bilinear of the top-left ``image`` (H, W) of x's stored grid (fp32 conv_transpose2d computes on an
    output_padding grid larger than its image)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt):
        return _resize_bilinear_bf16(x, size, out)
    B, C, Hp, Wp = xt.shape
    Hi, Wi = image
    Ho, Wo = size
    y = out if out is not None else _new((B, C, Ho, Wo), xt)
    _lib.call("cn_bilinear_fwd_f32", xt.data_ptr(), bstride(xt), y.data_ptr(), bstride(y), B, C, Hi, Wi, Ho, Wo,
              Hp, Wp, _stream())
    yv = Var(y, tape.enabled and x.req)
    if tape.enabled and x.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            dx, acc = grad_buffer(x)
            _lib.call("cn_bilinear_bwd_f32", dy.data_ptr(), bstride(dy), dx.data_ptr(), bstride(dx), B, C, Hi, Wi, Ho,
                      Wo, Hp, Wp, acc, _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


def split_channels(v: Var, sizes: T.Sequence[int]) -> T.List[Var]:
    """Channel slices of ``v`` as Vars (views, no copies); their gradients land in v's gradient buffer."""
    outs, c0 = [], 0
    for c in sizes:
        sv = Var(v.t[:, c0:c0 + c], v.req)
        sv.parent = (v, c0, c0 + c)
        outs.append(sv)
        c0 += c
    return outs


def join_channels(parts: T.Sequence[Var], buf: torch.Tensor) -> Var:
    """The parts ARE the consecutive channel slices of ``buf`` (written in place by ops with ``out=``):
    torch.cat without copies. Backward hands each part its slice of the gradient."""
    tape = current_tape()
    c0 = 0
    for p in parts:
        c = p.t.shape[1]
        if p.t.data_ptr() != buf[:, c0:c0 + c].data_ptr() or \
                (not is16(buf) and buf.shape[0] > 1 and bstride(p.t) != bstride(buf)):
            raise RuntimeError("join_channels: parts must be the channel slices of buf, in order")
        c0 += c
    yv = Var(buf, _req(tape, parts))
    if yv.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            o = 0
            for p in parts:
                c = p.t.shape[1]
                give_grad(p, dy[:, o:o + c])
                o += c
            yv.grad = None

        tape.add(bwd)
    return yv


def thin_conv3x3(x: Var, mods: T.Sequence, grouped: bool, dilation: int = 1,
                 out: T.Optional[torch.Tensor] = None) -> Var:
    """Several thin 3x3 'same' nn.Conv2d (weights [CP][Cin][3][3], padding == dilation) in one direct-kernel pass:
    ``grouped=False``: all read x; ``grouped=True``: conv g reads channels [g*Cin, (g+1)*Cin) of x.
    Output [B, len(mods)*CP, H, W] (channel = g*CP + c)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt):
        return _thin_conv3x3_bf16(x, mods, grouped, dilation, out)
    B, Cx, H, W = xt.shape
    n = len(mods)
    w0 = mods[0].weight
    CP, Cin = w0.shape[0], w0.shape[1]
    for m in mods:
        if tuple(m.weight.shape) != (CP, Cin, 3, 3):
            raise ValueError("thin_conv3x3: all weight sets must be [CP][Cin][3][3]")
    if Cx != (n * Cin if grouped else Cin):
        raise ValueError("thin_conv3x3: input channels do not match the weights")
    ws = [m.weight for m in mods]
    bs = [m.bias for m in mods]
    has_bias = bs[0] is not None
    wtab = _ptr_table([w.data_ptr() for w in ws])
    btab = _ptr_table([b.data_ptr() for b in bs]) if has_bias else None
    y = out if out is not None else _new((B, n * CP, H, W), xt)
    g = 1 if grouped else 0
    wpk = _new((Cin * 84,), xt) if (n, CP, g) == (3, 3, 0) and Cin >= 16 else None  # per-call packed weights
    _lib.call("cn_thin_conv3x3_fwd_f32", xt.data_ptr(), bstride(xt), wtab, btab, y.data_ptr(), bstride(y), B, Cin, H, W,
              n, CP, g, dilation, wpk.data_ptr() if wpk is not None else None, _stream())
    yv = Var(y, _req(tape, (x,), ws + bs))
    if yv.req:
        store = current_store()
        gw, gb = any(_tr(w) for w in ws), any(_tr(b) for b in bs)  # (one launch writes every weight set)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            with side_stream(xt, dy) if (gw or gb) else contextlib.nullcontext():
                s = _stream()
                if gw:
                    dwtab = _ptr_table([store.grad_of(w).data_ptr() for w in ws])
                    _lib.call("cn_thin_conv3x3_bwd_weight_f32", xt.data_ptr(), bstride(xt), dy.data_ptr(), bstride(dy),
                              dwtab, B, Cin, H, W, n, CP, g, dilation, s)
                if has_bias and gb:
                    for i, b in enumerate(bs):
                        dyi = dy[:, i * CP:(i + 1) * CP]
                        _lib.call("cn_channel_sum_f32", dyi.data_ptr(), bstride(dy), B, CP, H * W,
                                  store.grad_of(b).data_ptr(), 1, s)
            s = _stream()
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_thin_conv3x3_bwd_data_f32", dy.data_ptr(), bstride(dy), wtab, dx.data_ptr(), bstride(dx),
                          B, Cin, H, W, n, CP, g, dilation, acc, wpk.data_ptr() if wpk is not None else None, s)
            yv.grad = None

        tape.add(bwd, tuple(ws) + tuple(b for b in bs if b is not None))
    return yv


def cat_channels(parts: T.Sequence[Var], buf: T.Optional[torch.Tensor] = None) -> Var:
    """torch.cat(dim=1). Backward hands each input a channel-slice VIEW of the gradient (no copies).
    ``buf``: a preallocated [B, sum C, H, W] buffer; parts that were already produced in place in their slice of it
    (ops with ``out=``) are not copied."""
    tape = current_tape()
    t0 = _check(parts[0].t)
    B, H, W = t0.shape[0], t0.shape[2], t0.shape[3]
    Ctot = sum(p.t.shape[1] for p in parts)
    y = buf if buf is not None else _new((B, Ctot, H, W), t0)
    if tuple(y.shape) != (B, Ctot, H, W):
        raise ValueError("cat_channels: buffer shape does not match the parts")
    off = 0
    for p in parts:
        c = p.t.shape[1]
        dst = y[:, off:off + c]
        if is16(y):
            if p.t.data_ptr() != dst.data_ptr():
                _lib.call("cn_copy_bf16", _check(p.t).data_ptr(), ld(p.t), dst.data_ptr(), ld(y), B * H * W, c, 0,
                          _stream())
            off += c
            continue
        in_place = p.t.data_ptr() == dst.data_ptr() and (B == 1 or bstride(p.t) == bstride(y))
        if not in_place:
            _lib.call("cn_copy_f32", p.t.data_ptr(), bstride(p.t), dst.data_ptr(), bstride(y), B, c * H * W, 0,
                      _stream())
        off += c
    yv = Var(y, _req(tape, parts))
    if yv.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            o = 0
            for p in parts:
                c = p.t.shape[1]
                give_grad(p, dy[:, o:o + c])
                o += c
            yv.grad = None

        tape.add(bwd)
    return yv


def add(a: Var, b: Var) -> Var:
    tape = current_tape()
    at, bt = _check(a.t), _check(b.t)
    B = at.shape[0]
    n = int(at[0].numel())
    y = _new(at.shape, at)
    if is16(at):
        _lib.call("cn_add_bf16", at.data_ptr(), ld(at), bt.data_ptr(), ld(bt), y.data_ptr(), ld(y), _rows(at),
                  at.shape[1], _stream())
    else:
        _lib.call("cn_add_f32", at.data_ptr(), bstride(at), bt.data_ptr(), bstride(bt), y.data_ptr(), bstride(y), B, n,
                  _stream())
    yv = Var(y, _req(tape, (a, b)))
    if yv.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            give_grad(a, dy)
            if b.req:
                # never let two Vars alias one gradient buffer; a channel slice has no buffer of its own: give_grad
                # adds dy into its parent's gradient
                if b.grad is None and b.parent is None:
                    cp = _new(dy.shape, dy)
                    if is16(dy):
                        _lib.call("cn_copy_bf16", dy.data_ptr(), ld(dy), cp.data_ptr(), ld(cp), _rows(dy), dy.shape[1],
                                  0, _stream())
                    else:
                        _lib.call("cn_copy_f32", dy.data_ptr(), bstride(dy), cp.data_ptr(), bstride(cp), B, n, 0,
                                  _stream())
                    b.grad = cp
                else:
                    give_grad(b, dy)
            yv.grad = None

        tape.add(bwd)
    return yv


def _ptr_table(ptrs: T.Sequence[int]):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def final_combine(ha: Var, hb: Var, hc: Var, params: T.Sequence[torch.nn.Parameter], smooth: float) -> T.Tuple[Var, Var, Var]:
    """Fused TowerUNetFinalCombine. ``params``: 16 scalar parameters in the layout of cn_final_combine_fwd_f32."""
    tape = current_tape()
    a, b, c = _check(ha.t), _check(hb.t), _check(hc.t)
    B, _, H, W = a.shape
    HW = H * W
    for t in (a, b, c):
        if not t.is_contiguous():
            raise RuntimeError("final_combine expects dense [B,3,H,W] tower outputs")
    ptab = _ptr_table([p.data_ptr() for p in params])
    dist, edge, crop = (_new((B, 1, H, W), a) for _ in range(3))
    _lib.call("cn_final_combine_fwd_f32", a.data_ptr(), b.data_ptr(), c.data_ptr(), ptab, dist.data_ptr(),
              edge.data_ptr(), crop.data_ptr(), B, HW, float(smooth), _stream())
    req = _req(tape, (ha, hb, hc), params)
    outs = tuple(Var(t, req) for t in (dist, edge, crop))
    if req:
        store = current_store()

        def bwd():
            zeros = None
            gs = []
            for v in outs:
                if v.grad is None:
                    if zeros is None:
                        zeros = _new(dist.shape, dist)
                        _lib.call("cn_fill_f32", zeros.data_ptr(), zeros.numel(), 0.0, _stream())
                    gs.append(zeros)
                else:
                    gs.append(v.grad)
            das = []
            for v in (ha, hb, hc):
                if v.grad is not None:
                    raise RuntimeError("final_combine inputs must have a single consumer")
                v.grad = _new(v.t.shape, v.t)
                das.append(v.grad)
            dtab = _ptr_table([store.grad_of(p).data_ptr() for p in params])
            _lib.call("cn_final_combine_bwd_f32", a.data_ptr(), b.data_ptr(), c.data_ptr(), ptab, dist.data_ptr(),
                      edge.data_ptr(), crop.data_ptr(), gs[0].data_ptr(), gs[1].data_ptr(), gs[2].data_ptr(),
                      das[0].data_ptr(), das[1].data_ptr(), das[2].data_ptr(), dtab, B, HW, float(smooth), _stream())
            for v in outs:
                v.grad = None

        tape.add(bwd, tuple(params))
    return outs


# loss kinds / target modes of cn_tanimoto_*
LOSS_KINDS = {"TanimotoComplementLoss": 0, "TanimotoDistLoss": 1, "TanimotoCombined": 2}
TGT_FLOAT, TGT_EQ, TGT_RANGE, TGT_ONEHOT = 0, 1, 2, 3
MSK_NONE, MSK_LABEL, MSK_I64, MSK_F32 = 0, 1, 2, 3


def _loss_pred(pred: Var) -> torch.Tensor:
    """pred of a Tanimoto loss: fp32 [B,C,H,W] whose inner dims are dense (the kernels take a batch stride only)."""
    pt = pred.t
    if not pt.is_cuda or pt.dtype != torch.float32 or pt.dim() != 4:
        raise RuntimeError(f"Tanimoto losses need an fp32 [B,C,H,W] device tensor, got {pt.dtype} {tuple(pt.shape)}")
    if not _dense_inner(pt):
        raise RuntimeError("Tanimoto losses need pred with dense C,H,W (a batch stride is the only freedom)")
    return pt


def _loss_term_check(B: int, C: int, HW: int, kw: T.Dict[str, T.Any]) -> None:
    """The kernels index target_f as [B][C][HW] and labels / mask as [B][HW] with no bounds of their own: check every
    buffer a mode reads before anything is launched."""
    tmode, mmode = int(kw["target_mode"]), int(kw["mask_mode"])
    if tmode not in (TGT_FLOAT, TGT_EQ, TGT_RANGE, TGT_ONEHOT) or mmode not in (MSK_NONE, MSK_LABEL, MSK_I64, MSK_F32):
        raise ValueError(f"unknown target_mode {tmode} / mask_mode {mmode}")

    def dense(name, t, dtype, numel):
        if t is None:
            raise ValueError(f"{name} is required by target_mode {tmode} / mask_mode {mmode}")
        if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous {dtype} device tensor, got {t.dtype} "
                               f"(contiguous={t.is_contiguous()}, device={t.device})")
        if t.numel() != numel:
            raise ValueError(f"{name} must hold {numel} elements, got {t.numel()} {tuple(t.shape)}")

    labels, target_f, mask = kw.get("labels"), kw.get("target_f"), kw.get("mask")
    if labels is not None and labels.dtype != torch.int64:
        raise RuntimeError("labels must be int64")
    if tmode != TGT_FLOAT or mmode == MSK_LABEL:
        dense("labels", labels, torch.int64, B * HW)
    if tmode == TGT_FLOAT:
        dense("target_f", target_f, torch.float32, B * C * HW)
    if mmode == MSK_I64:
        dense("mask", mask, torch.int64, B * HW)
    elif mmode == MSK_F32:
        dense("mask", mask, torch.float32, B * HW)


def tanimoto_loss(pred: Var, *, target_f: T.Optional[torch.Tensor] = None, labels: T.Optional[torch.Tensor] = None,
                  mask: T.Optional[torch.Tensor] = None, target_mode: int, mask_mode: int, klass: int = 0,
                  loss_kind: int = 0, weight: float = 1.0, smooth: float = 1e-5, depth: int = 5,
                  total: T.Optional[torch.Tensor] = None) -> torch.Tensor:
    """Batch-mean Tanimoto loss of ``pred`` [B,C,H,W]; returns a 1-element device tensor.

    The tape node writes ``weight * dL/dpred`` into pred's gradient; ``total`` (1-element device
    tensor), when given, is incremented by ``weight * loss`` on the device.
    """
    tape = current_tape()
    pt = _loss_pred(pred)
    B, C = pt.shape[0], pt.shape[1]
    HW = int(pt[0, 0].numel())
    dev = pt.device
    _loss_term_check(B, C, HW, dict(target_f=target_f, labels=labels, mask=mask, target_mode=target_mode,
                                    mask_mode=mask_mode))
    sums = _alloc(5 * B, torch.float64, dev)
    coef = _alloc(4 * B, torch.float32, dev)
    loss = _alloc(1, torch.float32, dev)
    tf = target_f.data_ptr() if target_f is not None else None
    lb = labels.data_ptr() if labels is not None else None
    mk = mask.data_ptr() if mask is not None else None
    _lib.call("cn_tanimoto_fwd_f32", pt.data_ptr(), bstride(pt), tf, lb, mk, target_mode, mask_mode, klass, B, C, HW,
              loss_kind, smooth, depth, sums.data_ptr(), coef.data_ptr(), loss.data_ptr(), float(weight),
              total.data_ptr() if total is not None else None, _stream())
    if tape.enabled and pred.req:

        def bwd():
            dp, acc = grad_buffer(pred)
            _lib.call("cn_tanimoto_bwd_f32", pt.data_ptr(), bstride(pt), tf, lb, mk, target_mode, mask_mode, klass, B,
                      C, HW, coef.data_ptr(), float(weight), dp.data_ptr(), bstride(dp), acc, _stream())
            _keep = (target_f, labels, mask)  # noqa: F841  keep inputs alive until backward has run

        tape.add(bwd)
    return loss


def tanimoto_loss_multi(preds: T.Sequence[Var], terms: T.Sequence[T.Dict[str, T.Any]], *, loss_kind: int = 0,
                        weights: T.Optional[T.Sequence[float]] = None, smooth: float = 1e-5, depth: int = 5,
                        total: T.Optional[torch.Tensor] = None) -> torch.Tensor:
    """The n (<= 4) Tanimoto losses of calc_loss in ONE launch per pass (cn_tanimoto_multi_*_f32): ``terms[h]`` holds
    tanimoto_loss()'s keyword arguments for head h (target_f / labels / mask / target_mode / mask_mode / klass). Returns
    the n per-head batch means (device tensor); ``total`` (1 element) is WRITTEN with sum_h weights[h] * loss_h. The one
    tape node writes weights[h] * dL_h/dpred_h into every head's gradient."""
    tape = current_tape()
    n = len(preds)
    if not 1 <= n <= 4:
        raise ValueError(f"tanimoto_loss_multi: 1..4 heads, got {n}")
    if len(terms) != n or (weights is not None and len(weights) != n):
        raise ValueError("tanimoto_loss_multi: one term (and one weight) per head")
    weights = [1.0] * n if weights is None else [float(w) for w in weights]
    pts = [_loss_pred(p) for p in preds]
    B = pts[0].shape[0]
    HW = int(pts[0][0, 0].numel())
    dev = pts[0].device
    for pt, kw in zip(pts, terms):
        if pt.shape[0] != B or int(pt[0, 0].numel()) != HW:
            raise ValueError("tanimoto_loss_multi: the heads must share batch size and H*W")
        _loss_term_check(B, pt.shape[1], HW, kw)
    sums = _alloc(5 * B * n, torch.float64, dev)
    coef = _alloc(4 * B * n, torch.float32, dev)
    loss = _alloc(n, torch.float32, dev)

    def records(grads):
        buf = bytearray()
        for h, (pt, kw) in enumerate(zip(pts, terms)):
            ptr = lambda t: t.data_ptr() if t is not None else 0
            dp, dbs, acc = grads[h] if grads is not None else (0, 0, 0)
            buf += struct.pack("<QqQQQQqiiiifi", pt.data_ptr(), bstride(pt), ptr(kw.get("target_f")), ptr(kw.get("labels")),
                               ptr(kw.get("mask")), dp, dbs, int(kw["target_mode"]), int(kw["mask_mode"]),
                               int(kw.get("klass", 0)), pt.shape[1], weights[h], acc)
        return bytes(buf)

    _lib.call("cn_tanimoto_multi_fwd_f32", n, records(None), B, HW, loss_kind, smooth, depth, sums.data_ptr(),
              coef.data_ptr(), loss.data_ptr(), total.data_ptr() if total is not None else None, _stream())
    if tape.enabled and any(p.req for p in preds):

        def bwd():
            grads = []
            for p in preds:
                dp, acc = grad_buffer(p)
                grads.append((dp.data_ptr(), bstride(dp), acc))
            _lib.call("cn_tanimoto_multi_bwd_f32", n, records(grads), B, HW, coef.data_ptr(), _stream())
            _keep = terms  # noqa: F841  keep targets / labels / masks alive until backward has run

        tape.add(bwd)
    return loss


# ---------------------------------------------------------------------------
# dropout / pooling
# ---------------------------------------------------------------------------
_rng = {"seed": 0x5EED, "calls": 0, "step": 0, "words": {}}


def manual_seed(seed: int) -> None:
    """Seed of the counter-based dropout masks. A mask's seed has a HOST part -- (seed, index of the dropout call
    inside the step), a launch argument and therefore constant inside a recorded launch plan -- and a DEVICE part, the
    step word (one 64-bit word per device, bumped once per training forward by `begin_rng_step`), which the kernels add
    to it. Eager and replayed steps bump the same word the same way, so they draw identical masks."""
    _rng["seed"] = int(seed) & 0xFFFFFFFFFFFF
    _rng["calls"] = 0
    _rng["step"] = 0
    for w in _rng["words"].values():
        w.zero_()


def _step_word(dev) -> torch.Tensor:
    w = _rng["words"].get(dev)
    if w is None:
        w = _rng["words"][dev] = torch.zeros(1, dtype=torch.int64, device=dev)
    return w


def _host_step_inc() -> None:
    _rng["step"] += 1


def begin_rng_step(dev) -> None:
    """Start of a training forward with dropout: the per-step call counter restarts and the device step word advances
    (one 1-thread launch on the compute stream; part of a recorded plan like any other launch, as is the host mirror
    of the word's value)."""
    _rng["calls"] = 0
    _py_op(_host_step_inc)
    _lib.call("cn_rng_advance_u64", _step_word(dev).data_ptr(), 1, 0, _stream())


_STEP_MULT = 0xD1B54A32D192ED03  # cn_step_seed (cn_common.h)


def _bwd_seed(seed: int, step_fwd: int) -> int:
    """Seed for a backward mask launch: the kernels add the CURRENT step word; if another training forward has bumped
    it since this node's forward (two forwards before a backward in drop-in mode), compensate on the host."""
    d = step_fwd - _rng["step"]
    return seed if d == 0 else (seed + d * _STEP_MULT) & 0xFFFFFFFFFFFFFFFF


def _next_seed() -> int:
    _rng["calls"] += 1
    return ((_rng["seed"] << 16) ^ (_rng["calls"] * 0x9E3779B1)) & 0xFFFFFFFFFFFFFFFF


def dropout(x: Var, p: float, channelwise: bool, training: bool, out: T.Optional[torch.Tensor] = None) -> Var:
    """nn.Dropout2d (channelwise) / nn.Dropout; identity in eval mode or for p == 0 (``out`` is then ignored: the caller
    hands it to the producer of x instead)."""
    if not training or p <= 0.0:
        return x
    tape = current_tape()
    xt = _check(x.t)
    B, C = xt.shape[0], xt.shape[1]
    L = int(xt.shape[2] * xt.shape[3]) if is16(xt) else int(xt[0, 0].numel())
    seed = _next_seed()
    stepw = _step_word(xt.device).data_ptr()
    step_fwd = _rng["step"]
    y = out if _out_ok(out, xt) and (is16(xt) or _dense_inner(out)) else _new(xt.shape, xt)
    cw = 1 if channelwise else 0
    if is16(xt):  # mixed precision: the same counter-based masks on the NHWC buffer
        _lib.call("cn_dropout_bf16", xt.data_ptr(), ld(xt), y.data_ptr(), ld(y), B, C, L, float(p), seed, stepw, cw, 0,
                  _stream())
    else:
        _lib.call("cn_dropout_f32", xt.data_ptr(), bstride(xt), y.data_ptr(), bstride(y), B, C, L, float(p), seed, stepw,
                  cw, 0, _stream())
    yv = Var(y, tape.enabled and x.req)
    if tape.enabled and x.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            dx, acc = grad_buffer(x)
            if is16(dy):
                _lib.call("cn_dropout_bf16", dy.data_ptr(), ld(dy), dx.data_ptr(), ld(dx), B, C, L, float(p),
                          _bwd_seed(seed, step_fwd), stepw, cw, acc, _stream())
            else:
                _lib.call("cn_dropout_f32", dy.data_ptr(), bstride(dy), dx.data_ptr(), bstride(dx), B, C, L, float(p),
                          _bwd_seed(seed, step_fwd), stepw, cw, acc, _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


def adaptive_max_pool2d(x: Var, size: T.Tuple[int, int]) -> Var:
    """F.adaptive_max_pool2d(x, output_size=size)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt):
        return _adaptive_max_pool2d_bf16(x, size)
    B, C, Hi, Wi = xt.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = _new((B, C, Ho, Wo), xt)
    idx = _alloc((B, C, Ho, Wo), torch.int32, xt.device)
    _lib.call("cn_adaptive_maxpool_fwd_f32", xt.data_ptr(), bstride(xt), y.data_ptr(), bstride(y), idx.data_ptr(), B, C,
              Hi, Wi, Ho, Wo, _stream())
    yv = Var(y, tape.enabled and x.req)
    if tape.enabled and x.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            dx, acc = grad_buffer(x)
            _lib.call("cn_adaptive_maxpool_bwd_f32", dy.data_ptr(), bstride(dy), idx.data_ptr(), dx.data_ptr(),
                      bstride(dx), B, C, Hi, Wi, Ho, Wo, acc, _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


# ---------------------------------------------------------------------------
# mixed-precision (bf16 NHWC) op bodies: activations / activation gradients bf16, parameters + statistics fp32
# ---------------------------------------------------------------------------


def to_bf16(x: Var) -> Var:
    """fp32 NCHW -> bf16 NHWC at the entry of the mixed-precision region (gradient converted back)."""
    tape = current_tape()
    xt = _check(x.t)
    if is16(xt):
        return x
    B, C, H, W = xt.shape
    y = _alloc((B, H, W, C), torch.bfloat16, xt.device).permute(0, 3, 1, 2)
    if C % 8:
        raise RuntimeError("the bf16 region needs channel counts that are multiples of 8")
    _lib.call("cn_convert_f32nchw_to_bf16nhwc", xt.data_ptr(), bstride(xt), y.data_ptr(), ld(y), B, C, C, H * W,
              _stream())
    yv = Var(y, tape.enabled and x.req)
    if tape.enabled and x.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            dx, acc = grad_buffer(x)
            _lib.call("cn_convert_bf16nhwc_to_f32nchw", dy.data_ptr(), ld(dy), dx.data_ptr(), bstride(dx), B, C, H * W,
                      acc, _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


def to_f32(x: Var) -> Var:
    """bf16 NHWC -> fp32 NCHW inside the mixed-precision region: the way out for an op whose bf16 kernel does not cover a
    shape (LayerNorm over a channel count that is not 8 x a power of two, attention head dimensions outside 4..64 --
    widths like hidden 24 / 40 / 48 / 96): the op runs through its fp32 kernel and to_bf16() brings the result back."""
    tape = current_tape()
    xt = _check(x.t)
    if not is16(xt):
        return x
    B, C, H, W = xt.shape
    y = _alloc((B, C, H, W), torch.float32, xt.device)
    _lib.call("cn_convert_bf16nhwc_to_f32nchw", xt.data_ptr(), ld(xt), y.data_ptr(), bstride(y), B, C, H * W, 0, _stream())
    yv = Var(y, tape.enabled and x.req)
    if tape.enabled and x.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            dx, acc = grad_buffer(x)
            if acc:
                tmp = _new(tuple(xt.shape), xt)
                _lib.call("cn_convert_f32nchw_to_bf16nhwc", dy.data_ptr(), bstride(dy), tmp.data_ptr(), ld(tmp), B, C, C,
                          H * W, _stream())
                _lib.call("cn_copy_bf16", tmp.data_ptr(), ld(tmp), dx.data_ptr(), ld(dx), _rows(tmp), C, 1, _stream())
            else:
                _lib.call("cn_convert_f32nchw_to_bf16nhwc", dy.data_ptr(), bstride(dy), dx.data_ptr(), ld(dx), B, C, C,
                          H * W, _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


def _pow2(n: int) -> bool:
    return n >= 1 and (n & (n - 1)) == 0


def _bnstats_launch(xts, pws, ys, B, Cin, H, W, Cout, KH, KW, stride, paddings, dilations, stats, bns):
    """A training-mode ConvBlock2d convolution (bias-free, G <= 4 branches) through
    cn_conv2d_fwd_grouped_bnstats_bf16: the launch writes the per-tile statistics rows AND, for launches of <= 1008 pixel
    tiles, finishes them (mean / rstd / running statistics) by a last-block ticket -- the dependent finalize launch between
    the convolution and the BatchNorm apply disappears. Returns per-output (bn, mean, rstd) or None when the launch only
    wrote the rows."""
    G = len(xts)
    dev = xts[0].device
    tab = lambda ptrs: (ctypes.c_void_p * G)(*ptrs)
    means = _alloc((G, Cout), torch.float32, dev)
    rstds = _alloc((G, Cout), torch.float32, dev)
    has_running = bns[0].running_mean is not None
    need = int(_lib.query("cn_bn_group_workspace_floats_bf16", G, Cout))
    ws = _bn_group_ws16(G, Cout, dev)
    fin = ctypes.c_int(0)
    _lib.call("cn_conv2d_fwd_grouped_bnstats_bf16", G, tab([t.data_ptr() for t in xts]), ld(xts[0]),
              tab([p.fwd16.data_ptr() for p in pws]), tab([y.data_ptr() for y in ys]), ld(ys[0]), B, Cin, H, W, Cout, KH,
              KW, stride, (ctypes.c_int * G)(*paddings), (ctypes.c_int * G)(*dilations),
              tab([t.data_ptr() for t in stats]), tab([means[g].data_ptr() for g in range(G)]),
              tab([rstds[g].data_ptr() for g in range(G)]),
              tab([bn.running_mean.data_ptr() for bn in bns]) if has_running else None,
              tab([bn.running_var.data_ptr() for bn in bns]) if has_running else None, _bn_momentum(bns[0]),
              float(bns[0].eps), ws, max(need, 1 << 20), ctypes.byref(fin), _stream())
    if not fin.value:
        return None
    return [(bns[g], means[g], rstds[g]) for g in range(G)]


def _bnfin_ok(bns, mods) -> bool:
    return (bns is not None and len(bns) == len(mods)
            and all(m.bias is None for m in mods) and all(bn.training for bn in bns)
            and all(bn.momentum == bns[0].momentum and bn.eps == bns[0].eps for bn in bns)
            and all((bn.running_mean is None) == (bns[0].running_mean is None) for bn in bns)
            and mods[0].weight.shape[0] % 8 == 0)


def _conv2d_bf16(x: Var, mod, stride: int, padding: int, dilation: int, out: T.Optional[torch.Tensor],
                 want_stats: bool, bn=None) -> Var:
    tape = current_tape()
    xt = x.t
    B, Cin, H, W = xt.shape
    w = mod.weight
    Cout = w.shape[0]
    KH, KW = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    Ho = (H + 2 * padding - dilation * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * padding - dilation * (KW - 1) - 1) // stride + 1
    pw = packed_conv(mod, tape.enabled and x.req, bf16=True)
    y = _check(out) if out is not None else _new((B, Cout, Ho, Wo), xt)
    bias = mod.bias
    stats = None
    if want_stats:  # one row of {sum, sumsq}[Cout] per pixel tile, written by the conv epilogue (no zero-fill)
        rows = _lib.query("cn_conv2d_stats_rows_bf16", B, H, W, Cout, KH, KW, stride, padding, dilation)
        stats = _alloc((rows, 2, Cout), torch.float32, xt.device)
    bnfin = None
    if stats is not None and w.dim() == 4 and _bnfin_ok([bn] if bn is not None else None, [mod]):
        bnfin = _bnstats_launch([xt], [pw], [y], B, Cin, H, W, Cout, KH, KW, stride, [padding], [dilation], [stats], [bn])
        bnfin = bnfin[0] if bnfin is not None else False  # False: launched (rows only)
    if bnfin is None:
        _lib.call("cn_conv2d_fwd_bf16", xt.data_ptr(), ld(xt), pw.fwd16.data_ptr(),
                  bias.data_ptr() if bias is not None else None, y.data_ptr(), ld(y), 0, B, Cin, H, W, Cout, KH, KW,
                  stride, padding, dilation, 0, 0, stats.data_ptr() if stats is not None else None, _stream())
    yv = Var(y, _req(tape, (x,), (w, bias)))
    yv.stats = stats
    yv.bnfin = bnfin or None
    if yv.req:
        store = current_store()
        gw, gb = _tr(w), _tr(bias)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            with side_stream(xt, dy) if (gw or gb) else contextlib.nullcontext():
                s = _stream()
                if gw:
                    need = _lib.query("cn_bwgrad_workspace_floats", B, Cin, H, W, Cout, KH, KW, stride, padding,
                                      dilation, 0)
                    wsp, wsn = _ws16(need, xt.device)
                    _lib.call("cn_conv2d_bwd_weight_bf16", xt.data_ptr(), ld(xt), dy.data_ptr(), ld(dy),
                              store.grad_of(w).data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, padding, dilation, wsp,
                              wsn, s)
                if gb:
                    _lib.call("cn_channel_sum_bf16", dy.data_ptr(), ld(dy), B * Ho * Wo, Cout,
                              store.grad_of(bias).data_ptr(), 1, _bn_ws16(Cout, xt.device, "side"), s)
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv2d_bwd_data_bf16", dy.data_ptr(), ld(dy), pw.bwd16.data_ptr(), dx.data_ptr(), ld(dx),
                          B, Cin, H, W, Cout, KH, KW, stride, padding, dilation, acc, _stream())
            yv.grad = None

        tape.add(bwd, (w, bias))
    return yv


def _conv2d_group_bf16(xs: T.Sequence[Var], mods: T.Sequence, paddings: T.Sequence[int], dilations: T.Sequence[int],
                       stride: int, bns: T.Optional[T.Sequence] = None) -> T.List[Var]:
    """The G dilation branches of a ResidualAConv level as ONE bf16 implicit-GEMM launch (G classes of one launch:
    twice the blocks on the small planes, half the launches), every conv with its own BatchNorm statistics rows.
    Backward: weight gradients conv by conv on the side stream; data gradients in one grouped launch when the G inputs
    are distinct tensors (second level), conv by conv when they share their input (first level: the second launch
    accumulates -- a grouped launch would race on the shared dx)."""
    tape = current_tape()
    G = len(mods)
    xts = [x.t for x in xs]
    B, Cin, H, W = xts[0].shape
    w0 = mods[0].weight
    same = all(tuple(t.shape) == (B, Cin, H, W) and ld(t) == ld(xts[0]) for t in xts) and \
        all(tuple(m.weight.shape) == tuple(w0.shape) and (m.bias is None) == (mods[0].bias is None) for m in mods)
    if G < 2 or G > 4 or not same or w0.dim() != 4:
        return [_conv2d_bf16(x, m, stride, p, d, None, tape.enabled, bns[i] if bns is not None else None)
                for i, (x, m, p, d) in enumerate(zip(xs, mods, paddings, dilations))]
    Cout, KH, KW = w0.shape[0], w0.shape[2], w0.shape[3]
    Ho = (H + 2 * paddings[0] - dilations[0] * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * paddings[0] - dilations[0] * (KW - 1) - 1) // stride + 1
    need_bwd = tape.enabled and any(x.req for x in xs)
    pws = [packed_conv(m, need_bwd, bf16=True) for m in mods]
    ys = [_new((B, Cout, Ho, Wo), xts[0]) for _ in range(G)]
    biases = [m.bias for m in mods]
    has_bias = biases[0] is not None
    tab = lambda ptrs: (ctypes.c_void_p * G)(*ptrs)
    pads_c = (ctypes.c_int * G)(*paddings)
    dils_c = (ctypes.c_int * G)(*dilations)
    stats = None
    if tape.enabled:  # (training forward: the tape is on; rows of {sum, sumsq}[Cout] per pixel tile and conv)
        rows = _lib.query("cn_conv2d_stats_rows_bf16", B, H, W, Cout, KH, KW, stride, max(paddings), max(dilations))
        stats = [_alloc((rows, 2, Cout), torch.float32, xts[0].device) for _ in range(G)]
    bnfin = None
    if stats is not None and _bnfin_ok(bns, mods):
        bnfin = _bnstats_launch(xts, pws, ys, B, Cin, H, W, Cout, KH, KW, stride, list(paddings), list(dilations), stats,
                                list(bns))
        if bnfin is None:
            bnfin = False  # launched, rows only
    if bnfin is None:
        _lib.call("cn_conv2d_fwd_grouped_bf16", G, tab([t.data_ptr() for t in xts]), ld(xts[0]),
                  tab([p.fwd16.data_ptr() for p in pws]), tab([b.data_ptr() for b in biases]) if has_bias else None,
                  tab([y.data_ptr() for y in ys]), ld(ys[0]), B, Cin, H, W, Cout, KH, KW, stride, pads_c, dils_c, 0,
                  tab([t.data_ptr() for t in stats]) if stats is not None else None, _stream())
    req = _req(tape, xs, [m.weight for m in mods] + biases)
    yvs = [Var(y, req) for y in ys]
    for i, v in enumerate(yvs):
        v.stats = stats[i] if stats is not None else None
        v.bnfin = bnfin[i] if bnfin else None
    if req:
        store = current_store()
        shared_in = any(xs[i] is xs[j] for i in range(G) for j in range(i))
        gws = [_tr(m.weight) for m in mods]
        gbs = [_tr(b) for b in biases]

        def bwd():
            live = [i for i in range(G) if yvs[i].grad is not None]
            if not live:
                return
            wlive = [i for i in live if gws[i] or gbs[i]]
            with side_stream(*(list(xts) + [yvs[i].grad for i in live])) if wlive else contextlib.nullcontext():
                s = _stream()
                for i in wlive:
                    dy, m = yvs[i].grad, mods[i]
                    if not gws[i]:
                        _lib.call("cn_channel_sum_bf16", dy.data_ptr(), ld(dy), B * Ho * Wo, Cout,
                                  store.grad_of(m.bias).data_ptr(), 1, _bn_ws16(Cout, xts[i].device, "side"), s)
                        continue
                    need = _lib.query("cn_bwgrad_workspace_floats", B, Cin, H, W, Cout, KH, KW, stride, paddings[i],
                                      dilations[i], 0)
                    wsp, wsn = _ws16(need, xts[i].device)
                    _lib.call("cn_conv2d_bwd_weight_bf16", xts[i].data_ptr(), ld(xts[i]), dy.data_ptr(), ld(dy),
                              store.grad_of(m.weight).data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, paddings[i],
                              dilations[i], wsp, wsn, s)
                    if has_bias and gbs[i]:
                        _lib.call("cn_channel_sum_bf16", dy.data_ptr(), ld(dy), B * Ho * Wo, Cout,
                                  store.grad_of(m.bias).data_ptr(), 1, _bn_ws16(Cout, xts[i].device, "side"), s)
            todo = [i for i in live if xs[i].req]
            bufs = [grad_buffer(xs[i]) for i in todo] if not shared_in else None
            if todo and not shared_in and len(todo) == G and len({a for _, a in bufs}) == 1 \
                    and len({ld(d) for d, _ in bufs}) == 1 and len({ld(yvs[i].grad) for i in todo}) == 1:
                _lib.call("cn_conv2d_bwd_data_grouped_bf16", G, tab([yvs[i].grad.data_ptr() for i in todo]),
                          ld(yvs[0].grad), tab([p.bwd16.data_ptr() for p in pws]), tab([d.data_ptr() for d, _ in bufs]),
                          ld(bufs[0][0]), B, Cin, H, W, Cout, KH, KW, stride, pads_c, dils_c, bufs[0][1], _stream())
            else:
                for n, i in enumerate(todo):
                    dx, acc = bufs[n] if bufs is not None else grad_buffer(xs[i])
                    dy = yvs[i].grad
                    _lib.call("cn_conv2d_bwd_data_bf16", dy.data_ptr(), ld(dy), pws[i].bwd16.data_ptr(), dx.data_ptr(),
                              ld(dx), B, Cin, H, W, Cout, KH, KW, stride, paddings[i], dilations[i], acc, _stream())
            for v in yvs:
                v.grad = None

        tape.add(bwd, tuple(m.weight for m in mods) + tuple(b for b in biases if b is not None))
    return yvs


class _Fold16:
    """Eval-mode BatchNorm folded into the bf16 packed weights of the convolution in front of it."""

    __slots__ = ("wp", "scale", "shift", "key")

    def __init__(self):
        self.wp = self.scale = self.shift = None
        self.key = None


_EVAL_FUSION = True


def eval_fusion(enabled: bool) -> bool:
    """Switch the fused inference ConvBlock2d on / off (tests compare both forms); returns the previous setting."""
    global _EVAL_FUSION
    prev, _EVAL_FUSION = _EVAL_FUSION, bool(enabled)
    return prev


def can_fuse_eval(x: Var, bn, training: bool) -> bool:
    """ConvBlock2d as ONE launch: inference mode, mixed-precision (bf16 NHWC) input, nothing recorded for backward,
    running statistics present and a channel count the 16-byte NHWC stores cover."""
    return (_EVAL_FUSION and not training and not current_tape().enabled and is16(x.t)
            and bn.running_mean is not None and bn.weight.shape[0] % 8 == 0)


def conv_bn_act_eval(x: Var, conv, bn, act: int, stride: int, padding: int, dilation: int,
                     residual: T.Optional[Var] = None) -> Var:
    """y = residual + act(BatchNorm_eval(conv(x))) in ONE launch (cn_conv2d_fwd_fused_bf16): the running statistics
    are folded into a scaled copy of the packed weights (W' = W * gamma / sigma per cout) and a bias
    (beta - mu * gamma / sigma); the activation and the ResUNet-a running sum ride in the conv epilogue. The folded
    copy is refreshed when the parameters change (ParamStore version), when a train-mode forward has updated running
    statistics anywhere (engine epoch), or when the buffers were written through torch (their version counters)."""
    xt = x.t
    B, Cin, H, W = xt.shape
    w = conv.weight
    Cout = w.shape[0]
    KH, KW = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    taps = KH * KW
    Ho = (H + 2 * padding - dilation * (KH - 1) - 1) // stride + 1
    Wo = (W + 2 * padding - dilation * (KW - 1) - 1) // stride + 1
    store = current_store()
    fd = conv.__dict__.get("_cn_fold16")
    if fd is None:
        fd = conv.__dict__["_cn_fold16"] = _Fold16()
    key = (store.uid, store.version, _bn_stats_epoch, bn.running_mean._version, bn.running_var._version)
    s = _stream()
    if fd.key != key:
        if fd.wp is None or fd.key is None or fd.key[0] != key[0]:
            fd.wp = _alloc(_lib.query("cn_bconv_packed_elems", taps, Cin, Cout), torch.bfloat16, xt.device)
            fd.scale = _alloc(Cout, torch.float32, xt.device)
            fd.shift = _alloc(Cout, torch.float32, xt.device)
        cb = conv.bias
        _lib.call("cn_bn_fold_f32", bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                  bn.running_var.data_ptr(), cb.data_ptr() if cb is not None else None, float(bn.eps), Cout,
                  fd.scale.data_ptr(), fd.shift.data_ptr(), s)
        _lib.call("cn_pack_weights_scaled_bf16", w.data_ptr(), fd.scale.data_ptr(), fd.wp.data_ptr(), taps, Cin, Cout,
                  taps, Cin * taps, 1, s)
        fd.key = key
    y = _new((B, Cout, Ho, Wo), xt)
    rt = _check(residual.t) if residual is not None else None
    if rt is not None and tuple(rt.shape) != (B, Cout, Ho, Wo):
        raise ValueError("conv_bn_act_eval: the residual must have the output's shape")
    _lib.call("cn_conv2d_fwd_fused_bf16", xt.data_ptr(), ld(xt), fd.wp.data_ptr(), fd.shift.data_ptr(),
              rt.data_ptr() if rt is not None else None, ld(rt) if rt is not None else 0, y.data_ptr(), ld(y), B, Cin, H, W,
              Cout, KH, KW, stride, padding, dilation, 1 if act == ACT_SILU else 0, s)
    return Var(y, False)


def _conv_transpose2d_bf16(x: Var, mod, stride: int, padding: int) -> Var:
    tape = current_tape()
    xt = x.t
    B, Cin, H, W = xt.shape
    w = mod.weight
    Cout, KH, KW = w.shape[1], w.shape[2], w.shape[3]
    Ho = (H - 1) * stride - 2 * padding + KH
    Wo = (W - 1) * stride - 2 * padding + KW
    pw = packed_convT(mod, tape.enabled and x.req, bf16=True)
    y = _new((B, Cout, Ho, Wo), xt)
    bias = mod.bias
    _lib.call("cn_conv_transpose2d_fwd_bf16", xt.data_ptr(), ld(xt), pw.fwd16.data_ptr(),
              bias.data_ptr() if bias is not None else None, y.data_ptr(), ld(y), B, Cin, H, W, Cout, KH, KW, stride,
              padding, 0, _stream())
    yv = Var(y, _req(tape, (x,), (w, bias)))
    if yv.req:
        store = current_store()
        gw, gb = _tr(w), _tr(bias)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            with side_stream(xt, dy) if (gw or gb) else contextlib.nullcontext():
                s = _stream()
                if gw:
                    need = _lib.query("cn_bwgrad_workspace_floats", B, Cin, H, W, Cout, KH, KW, stride, padding, 1, 1)
                    wsp, wsn = _ws16(need, xt.device)
                    _lib.call("cn_conv_transpose2d_bwd_weight_bf16", xt.data_ptr(), ld(xt), dy.data_ptr(), ld(dy),
                              store.grad_of(w).data_ptr(), B, Cin, H, W, Cout, KH, KW, stride, padding, wsp, wsn, s)
                if gb:
                    _lib.call("cn_channel_sum_bf16", dy.data_ptr(), ld(dy), B * Ho * Wo, Cout,
                              store.grad_of(bias).data_ptr(), 1, _bn_ws16(Cout, xt.device, "side"), s)
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv_transpose2d_bwd_data_bf16", dy.data_ptr(), ld(dy), pw.bwd16.data_ptr(),
                          dx.data_ptr(), ld(dx), B, Cin, H, W, Cout, KH, KW, stride, padding, acc, _stream())
            yv.grad = None

        tape.add(bwd, (w, bias))
    return yv


def _bn_act_bf16(x: Var, bn, act: int, residual: T.Optional[Var], training: bool,
                 out: T.Optional[torch.Tensor]) -> Var:
    # every bf16 BatchNorm kernel walks P = B*H*W pixel rows at one stride: a view with gaps between rows or images (a
    # spatial crop of a larger buffer) has no kernel, and launching one on it would read / write the wrong pixels
    for what, t in (("input", x.t), ("output", out)):
        if t is not None and not _dense16(t):
            raise NotImplementedError(f"bn_act (bf16): the {what} must be one run of NHWC pixel rows (one pixel stride "
                                      "over the whole batch); a view with gaps between rows or images has no kernel")
    # G = 1 of the grouped entry point: same arithmetic, the finalize is ONE coalesced, ticketed launch
    return _bn_act_group_bf16([x], [bn], act, residual, True, training, [out] if out is not None else None)


def _bn_act_group_bf16(xs: T.Sequence[Var], bns: T.Sequence, act: int, residual: T.Optional[Var], sum_outputs: bool,
                       training: bool, outs: T.Optional[T.Sequence[torch.Tensor]]) -> T.Union[Var, T.List[Var]]:
    """bn_act_group in bf16, for layers one grouped launch serves (checked by the callers: bn_act_group, _bn_act_bf16)."""
    tape = current_tape()
    G = len(xs)
    xts = [x.t for x in xs]
    B, C, H, W = xts[0].shape
    P = B * H * W
    dev = xts[0].device
    use_batch = training or (bns[0].running_mean is None)
    has_sums = all(x.stats is not None for x in xs) and len({x.stats.shape[0] for x in xs}) == 1
    _note_bn_update(training)
    tab = lambda ptrs: (ctypes.c_void_p * G)(*ptrs)
    if outs is not None:
        ys = [_check(o) for o in outs]
        if len(ys) != (1 if sum_outputs else G) or any(ld(y) != ld(ys[0]) for y in ys):
            raise ValueError("bn_act_group: outs must match the outputs and share their pixel stride")
    else:
        ys = [_new(xts[0].shape, xts[0]) for _ in range(1 if sum_outputs else G)]
    # statistics already finished by the convolution launch that produced xs (_bnstats_launch)?
    prefin = training and all(x.bnfin is not None and x.bnfin[0] is bn for x, bn in zip(xs, bns))
    if prefin:
        means = [x.bnfin[1] for x in xs]
        rstds = [x.bnfin[2] for x in xs]
    else:
        means = _alloc((G, C), torch.float32, dev)
        rstds = _alloc((G, C), torch.float32, dev)
    rt = _check(residual.t) if residual is not None else None
    has_running = bns[0].running_mean is not None
    sums = [x.stats for x in xs] if (use_batch and has_sums and not prefin) else None
    ws = _bn_group_ws16(G, C, dev)
    gam, bet = tab([bn.weight.data_ptr() for bn in bns]), tab([bn.bias.data_ptr() for bn in bns])
    mtab, rtab = tab([means[g].data_ptr() for g in range(G)]), tab([rstds[g].data_ptr() for g in range(G)])
    _lib.call("cn_bn_act_group_fwd_bf16", G, tab([t.data_ptr() for t in xts]), ld(xts[0]), gam, bet,
              tab([bn.running_mean.data_ptr() for bn in bns]) if has_running else None,
              tab([bn.running_var.data_ptr() for bn in bns]) if has_running else None,
              rt.data_ptr() if rt is not None else None, ld(rt) if rt is not None else 0,
              tab([(ys[0] if sum_outputs else ys[g]).data_ptr() for g in range(G)]), ld(ys[0]), mtab, rtab, ws, P, C,
              1 if use_batch else 0, _bn_momentum(bns[0]), float(bns[0].eps), act, 1 if sum_outputs else 0,
              tab([t.data_ptr() for t in sums]) if sums is not None else None,
              -1 if prefin else (sums[0].shape[0] if sums is not None else 0), _stream())
    req = _req(tape, list(xs) + [residual], [bn.weight for bn in bns] + [bn.bias for bn in bns])
    yvs = [Var(y, req) for y in ys]
    if req:
        store = current_store()

        def bwd():
            if sum_outputs:
                dy = yvs[0].grad
                if dy is None:
                    return
                if residual is not None:
                    give_grad(residual, dy)
                dys = [dy] * G
            else:
                dys = [v.grad for v in yvs]
                if any(d is None for d in dys):
                    raise RuntimeError("bn_act_group: every output needs a gradient")
            bufs = [grad_buffer(x) if x.req else (None, 0) for x in xs]
            dxl = {ld(d) for d, _ in bufs if d is not None}
            dyl = {ld(d) for d in dys}
            if len(dxl) > 1 or len(dyl) > 1:
                raise RuntimeError("bn_act_group: gradient buffers must share their pixel strides")
            _lib.call("cn_bn_act_group_bwd_bf16", G, tab([t.data_ptr() for t in xts]), ld(xts[0]),
                      tab([d.data_ptr() for d in dys]), dyl.pop(), mtab, rtab, gam, bet,
                      tab([d.data_ptr() if d is not None else None for d, _ in bufs]), dxl.pop() if dxl else 0,
                      (ctypes.c_int * G)(*[a for _, a in bufs]),
                      tab([store.grad_of(bn.weight).data_ptr() for bn in bns]),
                      tab([store.grad_of(bn.bias).data_ptr() for bn in bns]), _bn_group_ws16(G, C, dev), P, C,
                      1 if use_batch else 0, act, _stream())
            _keep = (means, rstds)  # noqa: F841
            for v in yvs:
                v.grad = None

        tape.add(bwd, tuple(bn.weight for bn in bns) + tuple(bn.bias for bn in bns))
    return yvs[0] if sum_outputs else yvs


def _layer_norm_c_bf16(x: Var, ln, residual: T.Optional[Var], out: T.Optional[torch.Tensor] = None) -> Var:
    tape = current_tape()
    xt = x.t
    B, C, H, W = xt.shape
    if C % 8 or not _pow2(C >> 3) or (C >> 3) > 64:
        # the bf16 kernels reduce over C / 8 lanes with shuffles (8, 16, ... 512 channels): other widths through fp32
        r32 = to_f32(residual) if residual is not None else None
        return to_bf16(layer_norm_c(to_f32(x), ln, residual=r32))
    P = B * H * W
    y = out if _out_ok(out, xt) else _new(xt.shape, xt)
    rt = _check(residual.t) if residual is not None else None
    _lib.call("cn_layernorm_c_fwd_bf16", xt.data_ptr(), ld(xt), ln.weight.data_ptr(), ln.bias.data_ptr(),
              rt.data_ptr() if rt is not None else None, ld(rt) if rt is not None else 0, y.data_ptr(), ld(y), P, C,
              float(ln.eps), _stream())
    yv = Var(y, _req(tape, (x, residual), (ln.weight, ln.bias)))
    if yv.req:
        store = current_store()

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            if residual is not None:
                give_grad(residual, dy)
            dx, acc = grad_buffer(x)
            _lib.call("cn_layernorm_c_bwd_bf16", xt.data_ptr(), ld(xt), dy.data_ptr(), ld(dy), ln.weight.data_ptr(),
                      dx.data_ptr(), ld(dx), store.grad_of(ln.weight).data_ptr(), store.grad_of(ln.bias).data_ptr(), P, C,
                      float(ln.eps), acc, _stream())
            yv.grad = None

        tape.add(bwd, (ln.weight, ln.bias))
    return yv


def _na2d_bf16(qkv: Var, heads: int, kernel_size: int, dilation: int, attn_drop: float = 0.0) -> Var:
    tape = current_tape()
    qt = qkv.t
    B, C3, H, W = qt.shape
    C = C3 // 3
    if C % heads or (C // heads) not in (4, 8, 16, 32, 64):
        # head dimensions the bf16 kernels are not compiled for (hidden 24 / 40 / 48 / 96 ...): the fp32 kernels take any
        return to_bf16(na2d(to_f32(qkv), heads, kernel_size, dilation, attn_drop))
    seed = _next_seed() if attn_drop > 0.0 else 0
    stepw = _step_word(qkv.t.device).data_ptr() if attn_drop > 0.0 else None
    step_fwd = _rng["step"]
    out = _new((B, C, H, W), qt)
    attn = _alloc((B, heads, kernel_size * kernel_size, H, W), torch.float32, qt.device)
    _lib.call("cn_na2d_fwd_bf16", qt.data_ptr(), ld(qt), out.data_ptr(), ld(out), attn.data_ptr(), B, C, heads, H, W,
              kernel_size, dilation, float(attn_drop), seed, stepw, _stream())
    ov = Var(out, _req(tape, (qkv,)))
    if ov.req:

        def bwd():
            do = ov.grad
            if do is None:
                return
            dattn = _alloc_like(attn)
            dq = _new(qt.shape, qt)
            _lib.call("cn_na2d_bwd_bf16", qt.data_ptr(), ld(qt), do.data_ptr(), ld(do), attn.data_ptr(),
                      dattn.data_ptr(), dq.data_ptr(), ld(dq), B, C, heads, H, W, kernel_size, dilation,
                      float(attn_drop), _bwd_seed(seed, step_fwd), stepw, _stream())
            if qkv.grad is None and qkv.parent is None:
                qkv.grad = dq
            else:  # pragma: no cover - qkv has a single consumer in TowerUNet
                give_grad(qkv, dq)
            ov.grad = None

        tape.add(bwd)
    return ov


def _resize_bilinear_bf16(x: Var, size: T.Tuple[int, int], out: T.Optional[torch.Tensor]) -> Var:
    tape = current_tape()
    xt = x.t
    B, C, Hi, Wi = xt.shape
    Ho, Wo = size
    y = _check(out) if out is not None else _new((B, C, Ho, Wo), xt)
    if (Hi, Wi) == (Ho, Wo):
        _lib.call("cn_copy_bf16", xt.data_ptr(), ld(xt), y.data_ptr(), ld(y), B * Ho * Wo, C, 0, _stream())
    else:
        _lib.call("cn_bilinear_fwd_bf16", xt.data_ptr(), ld(xt), y.data_ptr(), ld(y), B, C, Hi, Wi, Ho, Wo, _stream())
    yv = Var(y, tape.enabled and x.req)
    if tape.enabled and x.req:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            if (Hi, Wi) == (Ho, Wo):
                give_grad(x, dy)
            else:
                dx, acc = grad_buffer(x)
                _lib.call("cn_bilinear_bwd_bf16", dy.data_ptr(), ld(dy), dx.data_ptr(), ld(dx), B, C, Hi, Wi, Ho, Wo, acc,
                          _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


def _spatial_channel_attention_bf16(skip: Var, out: Var, mod) -> Var:
    """spatial_channel_attention on bf16 NHWC skip / out: the pools and the gating run on the bf16 kernels; the channel
    MLPs (fp32 [B][C] in and out) and the 3x3 conv on the fp32 pooled maps [B][2][H][W] stay on their fp32 kernels.
    The tape has the fp32 structure: the pooling node is recorded first and runs last, after the apply node has handed
    d ca over and the 3x3 conv's backward has produced d pooled."""
    tape = current_tape()
    st, ot = skip.t, out.t
    B, C, H, W = st.shape
    L = H * W
    Ch = C // 2
    dev = st.device
    fc1, fc2 = mod.channel_attention.fc1, mod.channel_attention.fc2
    w1a, w2a, w1m, w2m = fc1[0].weight, fc1[2].weight, fc2[0].weight, fc2[2].weight
    gamma = mod.gamma
    f = lambda *shape: _alloc(shape, torch.float32, dev)
    avg, mx, ca = f(B, C), f(B, C), f(B, C)
    hpre_a, hpre_m = f(B, Ch), f(B, Ch)
    idx = _alloc((B, C), torch.int32, dev)
    pooled = f(B, 2, H, W)
    nws = _lib.query("cn_sca_workspace_floats_bf16", B, C, L)
    ws = f(max(nws, 1))
    s = _stream()
    _lib.call("cn_sca_pool_fwd_bf16", st.data_ptr(), ld(st), B, C, L, avg.data_ptr(), mx.data_ptr(), idx.data_ptr(),
              pooled.data_ptr(), ws.data_ptr(), nws, s)
    _lib.call("cn_sca_mlp_fwd_f32", avg.data_ptr(), mx.data_ptr(), w1a.data_ptr(), w2a.data_ptr(), w1m.data_ptr(),
              w2m.data_ptr(), hpre_a.data_ptr(), hpre_m.data_ptr(), ca.data_ptr(), B, C, Ch, s)
    # one flag for the whole block: its fused kernels write every parameter gradient of the block together (frozen
    # slices included, never read) whenever a gradient has to pass through it
    req = _req(tape, (skip, out), (w1a, w2a, w1m, w2m, gamma, mod.spatial_attention.conv.weight,
                                   mod.spatial_attention.conv.bias))
    pv = Var(pooled, req)
    shared = {}  # d ca handed from the apply node to the pooling node
    if req:
        store = current_store()

        def bwd_pool():  # recorded first => runs last: after the apply node and the 3x3 conv's backward
            dca = shared.pop("dca", None)
            if dca is None:
                return
            s2 = _stream()
            davg, dmx = f(B, C), f(B, C)
            _lib.call("cn_sca_mlp_bwd_f32", avg.data_ptr(), mx.data_ptr(), w1a.data_ptr(), w2a.data_ptr(),
                      w1m.data_ptr(), w2m.data_ptr(), hpre_a.data_ptr(), hpre_m.data_ptr(), ca.data_ptr(),
                      dca.data_ptr(), store.grad_of(w1a).data_ptr(), store.grad_of(w2a).data_ptr(),
                      store.grad_of(w1m).data_ptr(), store.grad_of(w2m).data_ptr(), davg.data_ptr(), dmx.data_ptr(),
                      B, C, Ch, s2)
            if skip.req:
                dpool = pv.grad
                if dpool is None:
                    dpool = _alloc_like(pooled)
                    _lib.call("cn_fill_f32", dpool.data_ptr(), dpool.numel(), 0.0, s2)
                dx, acc = grad_buffer(skip)
                _lib.call("cn_sca_pool_bwd_bf16", st.data_ptr(), ld(st), davg.data_ptr(), dmx.data_ptr(),
                          idx.data_ptr(), dpool.data_ptr(), dx.data_ptr(), ld(dx), B, C, L, acc, s2)
            pv.grad = None

        tape.add(bwd_pool, (w1a, w2a, w1m, w2m))
    sconv = thin_conv3x3(pv, [mod.spatial_attention.conv], grouped=False)  # fp32 [B,1,H,W], pre-sigmoid
    y = _new(ot.shape, ot)
    _lib.call("cn_sca_apply_fwd_bf16", ot.data_ptr(), ld(ot), ca.data_ptr(), sconv.t.data_ptr(), gamma.data_ptr(),
              y.data_ptr(), ld(y), B, C, L, s)
    yv = Var(y, req)
    if req:

        def bwd_apply():
            dy = yv.grad
            if dy is None:
                return
            s2 = _stream()
            dca, dsconv, scratch = f(B, C), f(B, 1, H, W), f(max(nws, 1))
            if out.req:
                do, acc = grad_buffer(out)
                dop, dold = do.data_ptr(), ld(do)
            else:
                dop, dold, acc = None, 0, 0
            _lib.call("cn_sca_apply_bwd_bf16", dy.data_ptr(), ld(dy), ot.data_ptr(), ld(ot), ca.data_ptr(),
                      sconv.t.data_ptr(), gamma.data_ptr(), dop, dold, acc, dca.data_ptr(), dsconv.data_ptr(),
                      store.grad_of(gamma).data_ptr(), scratch.data_ptr(), nws, B, C, L, s2)
            shared["dca"] = dca
            give_grad(sconv, dsconv)
            yv.grad = None

        tape.add(bwd_apply, (gamma,))
    return yv


def _adaptive_max_pool2d_bf16(x: Var, size: T.Tuple[int, int]) -> Var:
    tape = current_tape()
    xt = x.t
    B, C, Hi, Wi = xt.shape
    Ho, Wo = int(size[0]), int(size[1])
    y = _new((B, C, Ho, Wo), xt)
    need_bwd = tape.enabled and x.req
    idx = _alloc((B, Ho, Wo, C), torch.int32, xt.device) if need_bwd else None  # argmax per output (NHWC order)
    _lib.call("cn_adaptive_maxpool_fwd_bf16", xt.data_ptr(), ld(xt), y.data_ptr(), ld(y),
              idx.data_ptr() if idx is not None else None, B, C, Hi, Wi, Ho, Wo, _stream())
    yv = Var(y, need_bwd)
    if need_bwd:

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            dx, acc = grad_buffer(x)
            _lib.call("cn_adaptive_maxpool_bwd_bf16", dy.data_ptr(), ld(dy), idx.data_ptr(), dx.data_ptr(), ld(dx), B,
                      C, Hi, Wi, Ho, Wo, acc, _stream())
            yv.grad = None

        tape.add(bwd)
    return yv


class _ThinPack16:
    """Concatenated copy [n*CP][Cin][3][3] of the n thin head weights + its bf16 fragment packs (refreshed when the
    parameters change): the three head streams of a tower run as ONE 128 -> 9 convolution, one 9 -> 128 backward-data
    and one weight-gradient launch instead of three each."""

    __slots__ = ("wcat", "dwcat", "fwd16", "bwd16", "version", "store_id", "view")

    def __init__(self):
        self.wcat = self.dwcat = self.fwd16 = self.bwd16 = None
        self.version = -1
        self.store_id = 0
        self.view = False  # wcat is a VIEW of the store's flat buffer (the n weights are adjacent there)


def _thin_conv3x3_bf16(x: Var, mods: T.Sequence, grouped: bool, dilation: int, out: T.Optional[torch.Tensor]) -> Var:
    """The first head convolutions (128 -> 3, three streams) on a bf16 tower output: the MFMA kernel with an fp32
    NCHW epilogue, so everything downstream of it (9 / 3 / 1-channel head tensors) stays on the fp32 head kernels."""
    if grouped:
        raise NotImplementedError("grouped thin convolutions read the fp32 head tensors, never bf16")
    if any(m.bias is not None for m in mods):
        raise NotImplementedError("thin head convolutions on the bf16 path are bias-free (ConvBlock2d)")
    tape = current_tape()
    xt = x.t
    B, Cin, H, W = xt.shape
    n = len(mods)
    CP = mods[0].weight.shape[0]
    CPt = n * CP
    y = out if out is not None else _alloc((B, CPt, H, W), torch.float32, xt.device)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise RuntimeError("thin_conv3x3 (bf16 input) writes a dense fp32 NCHW tensor")
    HW = H * W
    store = current_store()
    store.refresh()
    tw = mods[0].__dict__.get("_cn_thin16")
    if tw is None or tw.store_id != store.uid:
        tw = _ThinPack16()
        tw.store_id = store.uid
        per = CP * Cin * 9
        w0 = mods[0].weight
        # the store keeps declared groups adjacent (ParamStore._with_contiguous_groups): the n weights ARE one
        # [n*CP][Cin][3][3] tensor, and so are their gradients -- no concatenated copies, no per-step copy / pack / zero /
        # copy-back launches (27 per step for the three towers)
        tw.view = all(m.weight.is_contiguous() and m.weight.data_ptr() == w0.data_ptr() + 4 * per * i
                      for i, m in enumerate(mods))
        if tw.view:
            o = (w0.data_ptr() - store._base) // 4
            tw.wcat = store.flat[o:o + n * per].view(CPt, Cin, 3, 3)
            tw.dwcat = None  # the flat gradient slice of the moment (the bridge swaps flat_grad): looked up at use
            tw.fwd16, tw.bwd16 = _pack_copies(PACK_BF16, tw.wcat, None, None, True, 9, Cin, CPt, 9, Cin * 9, 1)
        else:
            tw.fwd16 = _alloc(_lib.query("cn_bconv_packed_elems", 9, Cin, CPt), torch.bfloat16, xt.device)
            tw.bwd16 = _alloc(_lib.query("cn_bconv_packed_elems", 9, CPt, Cin), torch.bfloat16, xt.device)
            tw.wcat = _alloc((CPt, Cin, 3, 3), torch.float32, xt.device)
            tw.dwcat = _alloc_like(tw.wcat)
        mods[0].__dict__["_cn_thin16"] = tw
    if tw.view:  # registered with the batched per-step repack: one launch for every layer of the model
        if store.packed_version != store.version:
            store.repack_all()
    elif tw.version != store.version:
        s = _stream()
        per = CP * Cin * 9
        for i, m in enumerate(mods):
            _lib.call("cn_copy_f32", m.weight.data_ptr(), per, tw.wcat[i * CP].data_ptr(), per, 1, per, 0, s)
        _lib.call("cn_pack_weights_bf16", tw.wcat.data_ptr(), tw.fwd16.data_ptr(), 9, Cin, CPt, 9, Cin * 9, 1, s)
        _lib.call("cn_pack_weights_bf16", tw.wcat.data_ptr(), tw.bwd16.data_ptr(), 9, CPt, Cin, Cin * 9, 9, 1, s)
        tw.version = store.version
    _lib.call("cn_conv2d_fwd_bf16", xt.data_ptr(), ld(xt), tw.fwd16.data_ptr(), None, y.data_ptr(), 0, CPt * HW, B, Cin,
              H, W, CPt, 3, 3, 1, dilation, dilation, 0, 1, None, _stream())
    yv = Var(y, _req(tape, (x,), [m.weight for m in mods]))
    if yv.req:
        gw = any(_tr(m.weight) for m in mods)  # (one launch writes every weight set)

        def bwd():
            dy = yv.grad
            if dy is None:
                return
            s = _stream()
            cp8 = (CPt + 7) // 8 * 8
            d16 = _alloc((B, H, W, cp8), torch.bfloat16, xt.device)
            _lib.call("cn_convert_f32nchw_to_bf16nhwc", dy.data_ptr(), bstride(dy), d16.data_ptr(), cp8, B, CPt, cp8, HW, s)
            if gw:
                with side_stream(xt, d16):
                    ss = _stream()
                    need = _lib.query("cn_bwgrad_workspace_floats", B, Cin, H, W, CPt, 3, 3, 1, dilation, dilation, 0)
                    wsp, wsn = _ws16(need, xt.device)
                    if tw.view:  # accumulates straight into the flat gradient (zeroed once per step)
                        _lib.call("cn_conv2d_bwd_weight_bf16", xt.data_ptr(), ld(xt), d16.data_ptr(), cp8,
                                  store.grad_of(tw.wcat).data_ptr(), B, Cin, H, W, CPt, 3, 3, 1, dilation, dilation, wsp,
                                  wsn, ss)
                    else:
                        _lib.call("cn_fill_f32", tw.dwcat.data_ptr(), tw.dwcat.numel(), 0.0, ss)
                        _lib.call("cn_conv2d_bwd_weight_bf16", xt.data_ptr(), ld(xt), d16.data_ptr(), cp8,
                                  tw.dwcat.data_ptr(), B, Cin, H, W, CPt, 3, 3, 1, dilation, dilation, wsp, wsn, ss)
                        per = CP * Cin * 9
                        for i, m in enumerate(mods):
                            _lib.call("cn_copy_f32", tw.dwcat[i * CP].data_ptr(), per, store.grad_of(m.weight).data_ptr(),
                                      per, 1, per, 1, ss)
            if x.req:
                dx, acc = grad_buffer(x)
                _lib.call("cn_conv2d_bwd_data_bf16", d16.data_ptr(), cp8, tw.bwd16.data_ptr(), dx.data_ptr(), ld(dx), B,
                          Cin, H, W, CPt, 3, 3, 1, dilation, dilation, acc, s)
            yv.grad = None

        tape.add(bwd, tuple(m.weight for m in mods))
    return yv
