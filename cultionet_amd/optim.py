"""The flat optimizer state of the HIP step in torch's own optimizer format.

``NativeOptimizer`` is a ``torch.optim.Optimizer`` whose ``step()`` is the fused clip + optimizer launch pair of
csrc/cn_optim.hip over the flat parameter buffer (cultionet_amd.engine.ParamStore), for the four optimizers of the
reference (Adam, AdamW, RAdam, SGD: models/lightning.py:611-655). It serves both ways of training:

  * the Lightning route: ``lit.native_optimizer = True`` makes ``configure_optimizers`` return one, so that
    ``optimizer.step()`` is one or two launches instead of per-tensor work over 442 parameter views, torch's schedulers
    steer it through the param group, and ``torch.amp.GradScaler`` (precision "16-mixed") hands it the loss scale and
    the inf flag as device words: no unscale pass and no host synchronisation per step;
  * the native route: ``HipTrainer`` owns one and calls ``step_flat`` on ``store.flat_grad``; its ``state_dict`` /
    ``load_state_dict`` are this object's.

``exp_avg`` / ``exp_avg_sq`` (SGD: the momentum buffer alone) are two flat buffers in store order; ``self.state[p]``
holds views of them, so ``state_dict()`` is what the torch optimizer of the same kind writes and either loads the other's.
"""
from __future__ import annotations

import typing as T

import torch

from . import _lib
from . import engine as E

KINDS = {"Adam": 0, "AdamW": 0, "SGD": 1, "RAdam": 2}  # CN_OPT_* of csrc/cn_optim.hip
CLIP_NONE, CLIP_NORM, CLIP_VALUE = 0, 1, 2             # CN_CLIP_*


def launch_step(p: int, g: int, exp_avg: torch.Tensor, exp_avg_sq: T.Optional[torch.Tensor], n: int, sumsq: torch.Tensor,
                kind: int, clip: T.Optional[float], clip_algorithm: str, lr: float, beta1: float, beta2: float,
                eps: float, wd: float, step: int, scale: float, seg: T.Optional[T.Tuple[int, int, int, int]] = None,
                amp: T.Optional[T.Tuple[T.Optional[int], T.Optional[int], int]] = None) -> None:
    """Clip + optimizer over the flat buffers at ``p`` / ``g`` (device pointers, ``n`` elements): the sum of squares
    that norm clipping needs, then the update. ``seg`` = (table pointer, segments, chunks, step_add) takes the segmented
    entry points (``step`` is then unused: the table holds the counts); ``amp`` = (loss scale, found_inf, skipped) device
    pointers takes cn_optim_step_amp_f32 (which needs ``seg``) and counts the skipped step. AdamW / Adam with norm
    clipping or none keep their original pair."""
    s = E._stream()
    seg_args = () if seg is None else seg[:3]
    mode, sq, bound = CLIP_NONE, None, 0.0
    if clip is not None:
        bound = float(clip)
        if clip_algorithm == "value":
            mode = CLIP_VALUE
        else:
            mode, sq = CLIP_NORM, sumsq.data_ptr()
            _lib.call("cn_grad_sumsq_f32" if seg is None else "cn_grad_sumsq_seg_f32", g, n, *seg_args, sq, s)
    v = exp_avg_sq.data_ptr() if exp_avg_sq is not None else None
    head = (p, g, exp_avg.data_ptr(), v, n) + (() if seg is None else tuple(seg))
    hyper = (float(lr), float(beta1), beta2, eps, wd) + ((step,) if seg is None else ())
    if amp is not None:
        loss_scale, found_inf, skipped = amp
        _lib.call("cn_optim_step_amp_f32", kind, mode, *head, *hyper, scale, loss_scale, found_inf, skipped, sq, bound, s)
        if found_inf is not None:
            _lib.call("cn_amp_count_skip", found_inf, skipped, s)
    elif kind == 0 and mode != CLIP_VALUE:
        _lib.call("cn_adamw_step_f32" if seg is None else "cn_adamw_step_seg_f32", *head, *hyper, scale, sq, bound, s)
    else:
        _lib.call("cn_optim_step_f32" if seg is None else "cn_optim_step_seg_f32", kind, mode, *head, *hyper, scale, sq,
                  bound, s)


class NativeOptimizer(torch.optim.Optimizer):
    """``NativeOptimizer(params, store, kind, **hyper)``: ``params`` the model's parameters (one group), ``store`` their
    ParamStore, ``kind`` "Adam" | "AdamW" | "RAdam" | "SGD", ``hyper`` what ``torch.optim.<kind>`` takes. ``defaults`` are
    those of that torch class, so torch's schedulers (OneCycleLR cycling betas[0] / momentum included) and
    ``load_state_dict`` of either optimizer work unchanged. ``lr``, ``betas`` (or ``momentum``), ``eps`` and
    ``weight_decay`` are read from the group at every step.

    A parameter without a gradient (frozen, or ``grad is None``) is skipped for that step, as torch optimizers skip it.
    Every parameter keeps its own step count. ``set_clip`` fuses gradient clipping into the step.

    ``pruner`` (default None: the launches are the ones above): a cultionet_amd.pruning.MagnitudePruner of the same store.
    The step then zeroes the pruned entries of the gradient buffer it is about to read, in place and before the
    sum of squares (clipping sees the masked gradient), and the pruned entries of the parameters after the update.

    Under a GradScaler the host counts advance at every ``step()``; steps the scaler skipped are counted on the device
    (``skipped``) and subtracted inside the kernel, and folded into the host counts only when the trainable set changes
    and at ``state_dict()``.

    ``store=None`` builds the parameter container alone (defaults, groups, schedulers); such an object cannot step.
    """

    _step_supports_amp_scaling = True  # GradScaler.step sets .grad_scale / .found_inf (device tensors) and calls step()

    def __init__(self, params, store: T.Optional[E.ParamStore], kind: str, **hyper):
        if kind not in KINDS:
            raise NameError(f"optimizer {kind!r}: choose one of {sorted(KINDS)}")
        self.kind, self.opt_kind = kind, KINDS[kind]
        stand_in = getattr(torch.optim, kind)([torch.nn.Parameter(torch.zeros(1))], **hyper)
        super().__init__(params, dict(stand_in.defaults))
        self.clip: T.Optional[float] = None
        self.clip_algorithm = "norm"
        self.in_place = False  # did the last step() run on autograd's gradient buffer itself (no gather)?
        self.step_count = 0    # step() calls; the step count of every parameter while ``_psteps`` is None
        # per parameter (store order) once a step has run with a parameter left out; until then the unsegmented step
        self._psteps: T.Optional[T.List[int]] = None
        self._mask: T.Optional[T.Tuple[bool, ...]] = None  # the parameters of the last step (or table): store order
        self._segs = None      # (mask, anchor's count at build, [(offset, length, step)], device table, chunks, (lo, hi))
        self._amp_used = False
        # a cultionet_amd.pruning.MagnitudePruner: the step masks the gradient it reads and the parameters it wrote
        self.pruner = None
        self.store = None
        if store is not None:
            self._bind(store)

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("NativeOptimizer steps the whole flat parameter buffer with one set of hyper-parameters: "
                             "a second param group is not supported")
        super().add_param_group(param_group)

    def _bind(self, store: E.ParamStore) -> None:
        params = self.param_groups[0]["params"]
        index = {id(p): i for i, p in enumerate(store.params)}
        if len(params) != len(store.params) or any(id(p) not in index for p in params):
            raise ValueError("the parameters of the optimizer are not the parameters of the store")
        self.store = store
        self._order = [index[id(p)] for p in params]  # position in the param group -> index in the store
        dev = store.flat.device
        self.exp_avg = torch.zeros_like(store.flat)  # (SGD: the momentum buffer, its only state)
        self.exp_avg_sq = torch.zeros_like(store.flat) if self.kind != "SGD" else None
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)

    def set_clip(self, value: T.Optional[float], algorithm: T.Optional[str] = "norm") -> None:
        """lightning.Trainer(gradient_clip_val, gradient_clip_algorithm) inside the step (None or 0: no clipping)."""
        algorithm = "norm" if algorithm is None else str(getattr(algorithm, "value", algorithm))
        if algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm {algorithm!r}: choose 'norm' or 'value'")
        self.clip = float(value) if value else None
        self.clip_algorithm = algorithm

    # ---- step counts and the segment table -------------------------------------------------------------------------
    @property
    def param_steps(self) -> T.List[int]:
        """Optimizer step count of every parameter (store order), steps a scaler skipped included until folded."""
        return list(self._psteps) if self._psteps is not None else [self.step_count] * len(self.store.params)

    def _fold_skipped(self) -> None:
        """Take the skipped steps counted on the device out of the host counts of the current trainable set."""
        if not self._amp_used or self._mask is None:
            return
        k = int(self.skipped.item())
        if k == 0:
            return
        self.skipped.zero_()
        if self._psteps is None:
            self.step_count -= k
        else:
            for i, t in enumerate(self._mask):
                if t:
                    self._psteps[i] -= k

    def _set_mask(self, mask: T.Tuple[bool, ...]) -> None:
        """The trainable set changed: the skipped steps belong to the counts of the set that was trainable."""
        self._fold_skipped()
        self._mask, self._segs = mask, None
        self._publish(mask)

    def segments(self, mask: T.Tuple[bool, ...]):
        """Segment table of the trainable set ``mask`` (rebuilt when that set changes)."""
        if mask != self._mask:
            self._set_mask(mask)
        sg = self._segs
        if sg is None:
            store = self.store
            steps = self.param_steps
            segs = E.trainable_segments(store.offsets, [p.numel() for p in store.params], mask, steps)
            raw, chunks = E.segment_table(segs)
            table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(store.flat.device)
            span = (segs[0][0], segs[-1][0] + segs[-1][1])
            # the step counts of a table's parameters advance together while the set is unchanged: the kernel adds
            # the steps taken since the build (step_add)
            anchor = next(i for i, t in enumerate(mask) if t)
            sg = self._segs = (mask, steps[anchor], segs, table, chunks, span)
        return sg

    def _views(self, i: int) -> T.Tuple[torch.Tensor, T.Optional[torch.Tensor]]:
        p, o = self.store.params[i], self.store.offsets[i]
        m = self.exp_avg[o:o + p.numel()].view(p.shape)
        return m, (self.exp_avg_sq[o:o + p.numel()].view(p.shape) if self.exp_avg_sq is not None else None)

    def _publish(self, mask: T.Sequence[bool]) -> None:
        """``self.state[p]`` of the parameters in ``mask`` that have none yet (torch creates it at a parameter's first
        step): views of the flat buffers, ``step`` as torch's float scalar (refreshed at ``state_dict()``)."""
        for i, t in enumerate(mask):
            p = self.store.params[i]
            if t and p not in self.state:
                m, v = self._views(i)
                self.state[p] = {"momentum_buffer": m} if v is None else \
                    {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}

    # ---- the step ------------------------------------------------------------------------------------------------------
    def step_flat(self, grad: int, mask: T.Tuple[bool, ...], lr: float, beta1: float, beta2: float, eps: float, wd: float,
                  scale: float = 1.0, clip: T.Optional[float] = None, clip_algorithm: str = "norm",
                  amp: T.Optional[T.Tuple[T.Optional[int], T.Optional[int]]] = None) -> None:
        """One optimizer step of the parameters in ``mask`` on the flat gradient at device pointer ``grad`` (store
        layout), scaled by ``scale``. ``amp`` = (loss scale, found_inf) device pointers, either may be None."""
        store = self.store
        if mask != self._mask:
            self._set_mask(mask)
        self.step_count += 1
        segmented = self._psteps is not None or not all(mask)
        if segmented:
            if self._psteps is None:
                self._psteps = [self.step_count - 1] * len(mask)
            for i, t in enumerate(mask):
                if t:
                    self._psteps[i] += 1
        seg = None
        if segmented or amp is not None:
            _mask, step0, segs, table, chunks, _span = self.segments(mask)
            anchor = next(i for i, t in enumerate(mask) if t)
            now = self._psteps[anchor] if self._psteps is not None else self.step_count
            seg = (table.data_ptr(), len(segs), chunks, now - step0)
        if amp is not None:
            self._amp_used = True
            amp = (amp[0], amp[1], self.skipped.data_ptr())
        pruner = self.pruner
        if pruner is not None:
            if pruner.store is not store:
                raise ValueError("the pruner belongs to another ParamStore")
            pruner.mask_gradients(grad)
        launch_step(store.flat.data_ptr(), grad, self.exp_avg, self.exp_avg_sq, store.numel, self.sumsq, self.opt_kind,
                    clip, clip_algorithm, lr, beta1, beta2, eps, wd, self.step_count, scale, seg, amp)
        if pruner is not None:
            pruner.mask_parameters()
        store.bump(mask if segmented else None)  # only the stepped weights changed: only their packed copies refresh

    def _hyper(self) -> T.Tuple[float, float, float, float, float]:
        g = self.param_groups[0]
        wd = float(g["weight_decay"])
        if self.kind == "SGD":
            return float(g["lr"]), float(g["momentum"]), 0.0, 0.0, wd
        if wd != 0.0 and (self.kind == "Adam" or (self.kind == "RAdam" and not g.get("decoupled_weight_decay", False))):
            raise ValueError(f"{self.kind} with coupled (L2) weight decay has no HIP kernel: the fused step decays "
                             "the weights directly (AdamW, RAdam(decoupled_weight_decay=True))")
        return float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), wd

    def _find_grad(self) -> T.Tuple[int, T.Tuple[bool, ...]]:
        """(device pointer of the flat gradient in store layout, mask of the parameters that have a gradient). After a
        drop-in backward every ``p.grad`` is a view of ONE buffer at the store's offsets (autograd_bridge hands it over
        whole): verified here and then stepped on in place. Anything else (a DDP wrapper that replaced the gradients,
        gradients set by hand) is gathered into ``store.flat_grad`` with one foreach copy."""
        store = self.store
        grads = [p.grad if p.requires_grad else None for p in store.params]
        mask = tuple(g is not None for g in grads)
        self.in_place = False
        if not any(mask):
            return 0, mask
        first = mask.index(True)
        base = grads[first].data_ptr() - 4 * store.offsets[first]
        storage = grads[first].untyped_storage()
        if storage.data_ptr() <= base and base + 4 * store.numel <= storage.data_ptr() + storage.nbytes() and \
                all(g is None or (g.data_ptr() == base + 4 * o and g.dtype == torch.float32 and g.is_contiguous())
                    for g, o in zip(grads, store.offsets)):
            self.in_place = True
            return base, mask
        store.zero_grad()  # (the padding between the slices is read by the unsegmented step)
        flat = store.flat_grad
        dst = [flat[o:o + g.numel()].view(g.shape) for g, o in zip(grads, store.offsets) if g is not None]
        torch._foreach_copy_(dst, [g for g in grads if g is not None])
        return flat.data_ptr(), mask

    @staticmethod
    def _device_word(t: T.Optional[torch.Tensor], what: str, dev: torch.device) -> T.Optional[int]:
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or t.numel() != 1:
            raise ValueError(f"optimizer.{what} must be a one-element float32 tensor on {dev} (torch.amp.GradScaler's)")
        return t.data_ptr()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        store = self.store
        if store is None:
            raise RuntimeError("NativeOptimizer was built without a ParamStore (model not on a ROCm device): it cannot step")
        lr, beta1, beta2, eps, wd = self._hyper()
        grad, mask = self._find_grad()
        if not any(mask):
            return loss
        # torch.amp.GradScaler.step: grad_scale None = the gradients were unscaled already; found_inf alone then counts
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        amp = None
        if grad_scale is not None or found_inf is not None:
            dev = store.flat.device
            amp = (self._device_word(grad_scale, "grad_scale", dev), self._device_word(found_inf, "found_inf", dev))
        self.step_flat(grad, mask, lr, beta1, beta2, eps, wd, 1.0, self.clip, self.clip_algorithm, amp)
        store._sig = store._signature()  # the engine refreshes the packs bump() named, not every copy
        return loss

    # ---- torch's optimizer-state format ----------------------------------------------------------------------------------
    def state_dict(self):
        if self.store is not None:
            self._fold_skipped()
            steps = self.param_steps
            for p, i in zip(self.param_groups[0]["params"], self._order):
                st = self.state.get(p)
                if st is not None and "step" in st:
                    st["step"].fill_(steps[i])
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        """Accepts what this class or ``torch.optim.<kind>`` wrote: after the base class has validated and cast the
        dict, the loaded tensors are copied into the flat buffers (in place: pointers recorded in launch plans stay
        valid), ``self.state`` points at the views again and the step counts are taken."""
        super().load_state_dict(state_dict)
        if self.store is None:
            return
        n = len(self._order)
        steps, dst, src = [0] * n, [], []
        self.exp_avg.zero_()
        if self.exp_avg_sq is not None:
            self.exp_avg_sq.zero_()
        for p, i in zip(self.param_groups[0]["params"], self._order):
            st = self.state.get(p)
            if not st:
                self.state.pop(p, None)
                continue
            m, v = self._views(i)
            if v is None:
                loaded = {"momentum_buffer": st.get("momentum_buffer")}
                views = {"momentum_buffer": m}
            else:
                steps[i] = int(round(float(st["step"])))
                loaded = {"exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
                views = {"exp_avg": m, "exp_avg_sq": v}
                st["step"] = torch.tensor(float(steps[i]), dtype=torch.float32)
            for k, view in views.items():
                if loaded[k] is not None:  # (SGD before its first step: momentum_buffer None = zero here)
                    dst.append(view)
                    src.append(loaded[k])
                st[k] = view
        if dst:
            torch._foreach_copy_(dst, src)
        if len(set(steps)) == 1:
            self._psteps, self.step_count = None, steps[0]
        else:
            self._psteps, self.step_count = steps, max(steps)
        self._mask = self._segs = None
        self.skipped.zero_()
