"""Global magnitude pruning on the flat parameter buffer: ``cultionet fit --model-pruning`` natively.

Upstream the flag adds ``ModelPruning("l1_unstructured", amount)`` to the trainer's callbacks (callbacks.py:268-269),
which works through ``torch.nn.utils.prune``: every ``weight`` / ``bias`` becomes a ``*_orig`` parameter, a ``*_mask``
buffer and a forward pre-hook. Here every parameter is a view of ``ParamStore.flat``, the packed MFMA copies are refreshed
from that buffer and the fused optimizer steps it as a whole, so the same rule is kept on the buffer itself
(csrc/cn_prune.hip):

  * one byte of flags per flat element (bit 0 alive, bit 1 prunable) beside the weights;
  * a round is an exact radix selection of the ``k`` alive prunable entries of smallest ``|w|`` across all tensors
    (``torch.nn.utils.prune.global_unstructured(..., L1Unstructured, amount)``), ties by lowest flat index, no host
    synchronisation;
  * ``effective weight = orig * mask`` and ``grad(orig) = grad * mask`` are kept by holding the pruned entries of the flat
    buffer at exactly ``+0.0``: the optimizer masks the gradient it is about to step (clipping sees the masked gradient)
    and the parameters after the update (``NativeOptimizer.pruner``). Optimizer moments are left alone.

``MagnitudePruner`` is the pruner, ``NativePruning`` the callback for the Lightning loop, ``HipTrainer(pruner=...)`` /
``trainer.prune(amount)`` the native route.

Non-finite weights are not looked for (that would need a synchronisation): they order by the bit pattern of ``|w|``,
above every finite value, NaN above inf.
"""
from __future__ import annotations

import numbers
import typing as T

import torch

from . import _lib
from . import engine as E

ALIVE, PRUNABLE = 1, 2  # the bits of a flag byte (csrc/cn_prune.hip)
PRUNED_NAMES = ("weight", "bias")  # ModelPruning's default ``parameter_names``
CONTAINERS = (torch.nn.Sequential, torch.nn.ModuleList, torch.nn.ModuleDict)


def _lightning_base() -> type:
    from .lightning import _Base

    return _Base


def prunable_parameters(root: torch.nn.Module) -> T.List[T.Tuple[str, str, torch.nn.Parameter]]:
    """``(module name, parameter name, parameter)`` of what ``ModelPruning`` prunes when no ``parameters_to_prune`` is
    given: the ``weight`` and ``bias`` parameters that sit directly on a module that is not a container (Sequential,
    ModuleList, ModuleDict, the LightningModule). ``requires_grad`` does not matter; a shared parameter is listed once."""
    containers = CONTAINERS + (_lightning_base(),)
    out, seen = [], set()
    for mod_name, m in root.named_modules():
        if isinstance(m, containers):
            continue
        for name in PRUNED_NAMES:
            p = m._parameters.get(name)
            if p is not None and id(p) not in seen:
                seen.add(id(p))
                out.append((mod_name, name, p))
    return out


def prune_count(amount: T.Union[int, float], alive: int) -> int:
    """Entries one round prunes out of ``alive``: an integer ``amount`` itself, ``round(amount * alive)`` for a float
    (Python's ``round``, as torch.nn.utils.prune). ValueError: a negative amount, a float outside [0, 1], more than
    ``alive``; TypeError: anything else."""
    if isinstance(amount, bool) or not isinstance(amount, (numbers.Integral, numbers.Real)):
        raise TypeError(f"amount must be an int or a float, got {type(amount).__name__}")
    if isinstance(amount, numbers.Integral):
        k = int(amount)
        if k < 0:
            raise ValueError(f"amount={k} should be a non-negative integer")
    else:
        if not 0.0 <= float(amount) <= 1.0:
            raise ValueError(f"amount={amount} should be a float in the range [0, 1]")
        k = round(float(amount) * alive)
    if k > alive:
        raise ValueError(f"amount={amount} asks for {k} entries: only {alive} prunable entries are left")
    return k


def build_flags(params: T.Iterable[torch.nn.Parameter], store: E.ParamStore) -> torch.Tensor:
    """Host flags (uint8, one per flat element) with ``params`` alive and prunable; padding and every other parameter 0."""
    offset = {id(p): o for p, o in zip(store.params, store.offsets)}
    flags = torch.zeros(store.numel, dtype=torch.uint8)
    for p in params:
        o = offset.get(id(p))
        if o is None:
            raise ValueError("a prunable parameter is not part of the ParamStore (was the module moved or re-created?)")
        flags[o:o + p.numel()] = ALIVE | PRUNABLE
    return flags


class MagnitudePruner:
    """``MagnitudePruner(lit_or_module, store=None, lottery_ticket=False)``: the pruning state of one ParamStore.

    ``lit_or_module``: a CultionetLitModel (its ``cultionet_model`` is walked, its mask model owns the store), a model with
    ``param_store()``, or any module together with its ``store``. ``lottery_ticket``: keep a copy of ``store.flat`` as it
    is now and, after every round, write it back into the surviving prunable entries (Lightning's
    ``use_lottery_ticket_hypothesis``).

    ``alive``, ``total`` and ``sparsity()`` are host integers: a round prunes exactly ``k`` entries, so nothing is read back.
    """

    def __init__(self, lit_or_module: torch.nn.Module, store: T.Optional[E.ParamStore] = None,
                 lottery_ticket: bool = False):
        module = getattr(lit_or_module, "cultionet_model", lit_or_module)
        if store is None:
            store = getattr(module, "mask_model", module).param_store()
        if store.numel >= 1 << 31:
            raise ValueError("the selection kernels index the flat buffer with 31 bits")
        self.store = store
        host = build_flags([p for _, _, p in prunable_parameters(module)], store)
        self.total = int((host != 0).sum())
        if self.total == 0:
            raise ValueError("the module has no weight or bias parameter to prune")
        self.alive = self.total
        dev = store.flat.device
        self.flags = host.to(dev)
        self.snapshot = store.flat.clone() if lottery_ticket else None
        self._ws = torch.zeros(_lib.query("cn_prune_workspace_words", store.numel), dtype=torch.int32, device=dev)
        self._count = torch.zeros(1, dtype=torch.int32, device=dev)

    @property
    def lottery_ticket(self) -> bool:
        return self.snapshot is not None

    def sparsity(self, sync: bool = False) -> float:
        """Pruned share of the prunable entries; ``sync=True`` counts on the device (one synchronisation)."""
        alive = self.count_alive() if sync else self.alive
        return 1.0 - alive / self.total

    def count_alive(self) -> int:
        """Alive prunable entries counted from the device flags (synchronises)."""
        self._count.zero_()
        _lib.call("cn_prune_count_u32", self.flags.data_ptr(), self.store.numel, self._count.data_ptr(), E._stream())
        return int(self._count.item())

    def keep_mask(self, param: torch.Tensor) -> torch.Tensor:
        """Bool tensor shaped like ``param`` (a parameter of the store): False where it is pruned."""
        o = (param.data_ptr() - self.store.flat.data_ptr()) // 4
        if o < 0 or o + param.numel() > self.store.numel:
            raise ValueError("tensor is not part of this pruner's ParamStore")
        return ((self.flags[o:o + param.numel()] & (ALIVE | PRUNABLE)) != PRUNABLE).view(param.shape)

    def mask_gradients(self, ptr: int) -> None:
        """Zero the pruned entries of a flat gradient in store layout at device pointer ``ptr``, in place."""
        _lib.call("cn_mask_select_f32", ptr, ptr, self.flags.data_ptr(), self.store.numel, E._stream())

    def mask_parameters(self) -> None:
        """Zero the pruned entries of ``store.flat`` in place (the caller bumps the store)."""
        self.mask_gradients(self.store.flat.data_ptr())

    def prune(self, amount: T.Union[int, float]) -> int:
        """One round: prune the ``k`` (``prune_count``) alive prunable entries of smallest ``|w|``; returns ``k``."""
        k = prune_count(amount, self.alive)
        if k == 0:
            return 0
        store = self.store
        _lib.call("cn_prune_magnitude_u8", store.flat.data_ptr(), self.flags.data_ptr(), store.numel, k,
                  self._ws.data_ptr(), self._ws.numel(), E._stream())
        self.alive -= k
        if self.snapshot is not None:
            _lib.call("cn_prune_reset_f32", store.flat.data_ptr(), self.snapshot.data_ptr(), self.flags.data_ptr(),
                      store.numel, E._stream())
        else:
            self.mask_parameters()
        store.bump()
        return k

    def state_dict(self) -> T.Dict[str, T.Any]:
        return {"flags": self.flags.cpu(), "alive": self.alive, "total": self.total,
                "snapshot": None if self.snapshot is None else self.snapshot.cpu()}

    def load_state_dict(self, d: T.Mapping[str, T.Any]) -> None:
        """In place: device pointers stay valid. The prunable map must be this store's."""
        flags = d["flags"]
        if flags.numel() != self.flags.numel() or int(d["total"]) != self.total:
            raise ValueError("pruner state of another parameter layout")
        if (d["snapshot"] is None) != (self.snapshot is None):
            raise ValueError("pruner state with lottery_ticket=%s loaded into a pruner with lottery_ticket=%s"
                             % (d["snapshot"] is not None, self.snapshot is not None))
        self.flags.copy_(flags)
        self.alive = int(d["alive"])
        if self.snapshot is not None:
            self.snapshot.copy_(d["snapshot"])


try:  # Lightning's Callback when lightning is installed (it is not in the build image): the trainer calls every hook of
    # the protocol on each callback, reads ``state_key`` and checkpoints ``state_dict()``, all of which the base provides
    from lightning.pytorch.callbacks import Callback as _CallbackBase  # type: ignore
except Exception:  # pragma: no cover - exercised in the build image
    try:
        from pytorch_lightning.callbacks import Callback as _CallbackBase  # type: ignore
    except Exception:
        _CallbackBase = object


class NativePruning(_CallbackBase):
    """Callback for the Lightning loop in place of ``ModelPruning("l1_unstructured", amount)``: global unstructured
    pruning at every train-epoch end, with the lottery-ticket reset by default. A ``lightning.pytorch.Callback`` when
    lightning imports, a plain object with the same hooks otherwise (so the module imports without it). It has been
    driven hook by hook only: it was never run under a real ``lightning.Trainer``. Needs
    ``pl_module.native_optimizer = True``: the masks are applied inside the fused step. ``state_dict()`` /
    ``load_state_dict()`` carry the pruner (Lightning saves them with the checkpoint under the callback's state key).
    """

    def __init__(self, amount: T.Union[int, float], lottery_ticket: bool = True):
        super().__init__()
        prune_count(amount, 1 << 62)  # (type and range)
        self.amount = amount
        self.lottery_ticket = bool(lottery_ticket)
        self.pruner: T.Optional[MagnitudePruner] = None
        self._loaded: T.Optional[T.Mapping[str, T.Any]] = None  # a state loaded before the pruner exists

    @staticmethod
    def _check(pl_module) -> None:
        if not getattr(pl_module, "native_optimizer", False):
            raise RuntimeError("NativePruning masks gradients and parameters inside the fused optimizer step: set "
                               "lit.native_optimizer = True (a torch optimizer over the parameter views is not masked)")

    def _attach(self, trainer, pl_module) -> bool:
        """Build the pruner (once) and hand it to the trainer's NativeOptimizers; False while there is none yet."""
        from .optim import NativeOptimizer

        opts = [o for o in (getattr(trainer, "optimizers", None) or []) if isinstance(o, NativeOptimizer)]
        if not opts:
            return False
        if opts[0].store is None:
            raise RuntimeError("the NativeOptimizer was built without a ParamStore (model not on a ROCm device): "
                               "NativePruning has no flat buffer to prune")
        if self.pruner is None:
            self.pruner = MagnitudePruner(pl_module, store=opts[0].store, lottery_ticket=self.lottery_ticket)
            if self._loaded is not None:
                self.pruner.load_state_dict(self._loaded)
                self._loaded = None
        for o in opts:
            o.pruner = self.pruner
        return True

    def setup(self, trainer, pl_module, stage: T.Optional[str] = None) -> None:
        self._check(pl_module)
        self._attach(trainer, pl_module)  # (Lightning configures the optimizers later: on_fit_start attaches then)

    def on_fit_start(self, trainer, pl_module) -> None:
        self._check(pl_module)
        if not self._attach(trainer, pl_module):
            raise RuntimeError("NativePruning found no NativeOptimizer among trainer.optimizers")

    def on_train_epoch_end(self, trainer, pl_module) -> None:
        if self.pruner is None:
            raise RuntimeError("NativePruning.on_train_epoch_end before on_fit_start")
        self.pruner.prune(self.amount)

    def state_dict(self) -> T.Dict[str, T.Any]:
        return {} if self.pruner is None else {"pruner": self.pruner.state_dict()}

    def load_state_dict(self, state_dict: T.Mapping[str, T.Any]) -> None:
        """Lightning restores callbacks before ``on_fit_start``: the state is kept until the pruner is built."""
        if "pruner" in state_dict:
            if self.pruner is not None:
                self.pruner.load_state_dict(state_dict["pruner"])
            else:
                self._loaded = state_dict["pruner"]
