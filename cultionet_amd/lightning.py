"""CultionetLitModel on the HIP engine.

Host-side mirror of /root/reference/src/cultionet/models/lightning.py for the hot path: the constructor
keeps the reference's 24 keyword arguments (lightning.py:822-847), the model lives under the attribute
``f"{model_name}_{model_type}"`` (state-dict prefix ``cultionet_TowerUNet.mask_model.``), and
``forward / predict_step / get_true_labels / calc_loss / training_step / configure_optimizers`` keep their
signatures and return types, so ``cultionet.fit`` / ``predict_lightning`` can drive it unchanged.

Two ways to train:
  * **drop-in** (lightning.Trainer): ``training_step`` returns a torch scalar whose ``backward()`` replays
    the HIP tape through cultionet_amd.autograd_bridge; torch optimizers / DDP work as usual.
  * **native** (``HipTrainer``, used by bench.py): forward + Tanimoto + backward + global-norm clip + fused
    AdamW entirely in HIP kernels on flat parameter/gradient buffers, RCCL all-reduce of the flat gradient
    overlapped with the backward tape (cultionet_amd.ddp).
"""
from __future__ import annotations

import typing as T
from pathlib import Path

import torch

from . import engine as E
from .cultionet import CultioNet
from .data import Data
from .enums import (AttentionTypes, InferenceNames, LearningRateSchedulers, LossTypes, ModelTypes, ResBlockTypes,
                    ValidationNames)
from .losses import CombinedLoss, TanimotoComplementLoss, TanimotoDistLoss

try:  # the real LightningModule when lightning is installed (it is not in the build image)
    from lightning import LightningModule as _Base  # type: ignore

    if not hasattr(_Base, "load_from_checkpoint"):  # a test double left in sys.modules is not Lightning
        raise ImportError("lightning.LightningModule lacks load_from_checkpoint")
except Exception:  # pragma: no cover - exercised in the build image
    class _Base(torch.nn.Module):
        """Minimal stand-in providing the LightningModule methods this file uses."""

        def __init__(self):
            super().__init__()
            self.hparams: T.Dict[str, T.Any] = {}
            self.trainer = None

        def save_hyperparameters(self, *args, **kwargs):
            import inspect

            frame = inspect.currentframe().f_back
            av = inspect.getargvalues(frame)
            self.hparams = {k: av.locals[k] for k in av.args if k != "self"}

        def clip_gradients(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
            if gradient_clip_val is None or gradient_clip_val <= 0:
                return
            params = [p for g in optimizer.param_groups for p in g["params"]]
            if str(getattr(gradient_clip_algorithm, "value", gradient_clip_algorithm)) == "value":
                torch.nn.utils.clip_grad_value_(params, clip_value=gradient_clip_val)
            else:
                torch.nn.utils.clip_grad_norm_(params, gradient_clip_val)

        def configure_gradient_clipping(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
            self.clip_gradients(optimizer, gradient_clip_val=gradient_clip_val,
                                gradient_clip_algorithm=gradient_clip_algorithm)

        def log(self, *args, **kwargs):
            pass

        def log_dict(self, *args, **kwargs):
            pass

        @classmethod
        def load_from_checkpoint(cls, checkpoint_path, map_location=None, **kwargs):
            ckpt = torch.load(str(checkpoint_path), map_location=map_location or "cpu", weights_only=False)
            hp = dict(ckpt.get("hyper_parameters", {}))
            hp.update(kwargs)
            model = cls(**hp)
            model.load_state_dict(ckpt["state_dict"])
            return model


# lightning.py:38-92 restricted to the losses selectable from the CLI (args.yml:436-442)
LOSS_DICT = {
    LossTypes.TANIMOTO_COMPLEMENT: {
        "classification": TanimotoComplementLoss(),
        "regression": TanimotoComplementLoss(transform_logits=False, one_hot_targets=False),
    },
    LossTypes.TANIMOTO: {
        "classification": TanimotoDistLoss(),
        "regression": TanimotoDistLoss(transform_logits=False, one_hot_targets=False),
    },
    LossTypes.TANIMOTO_COMBINED: {
        "classification": CombinedLoss(losses=[TanimotoDistLoss(), TanimotoComplementLoss()]),
        "regression": CombinedLoss(losses=[TanimotoDistLoss(transform_logits=False, one_hot_targets=False),
                                           TanimotoComplementLoss(transform_logits=False, one_hot_targets=False)]),
    },
}


class LightningModuleMixin(_Base):
    def __init__(self):
        super().__init__()

    def forward(self, batch: Data, batch_idx: int = None) -> T.Dict[str, torch.Tensor]:
        """distance / edge / crop probabilities, each (B, 1, H, W); crop_type, classes_l2, classes_l3 = None."""
        return self.cultionet_model(batch)

    @property
    def cultionet_model(self) -> CultioNet:
        return getattr(self, self.model_attr)

    @property
    def hip_precision(self) -> T.Optional[str]:
        """Explicit precision of the drop-in forward ("32-true" | "bf16-mixed" | "16-mixed"), or None (default): follow
        the torch.autocast region lightning.Trainer(precision=...) opens (model.py:168-186)."""
        return self.cultionet_model.mask_model.precision

    @hip_precision.setter
    def hip_precision(self, value: T.Optional[str]) -> None:
        if value not in (None, "32-true", "32", "bf16-mixed", "16-mixed"):
            raise ValueError(f"unsupported precision {value!r}")
        self.cultionet_model.mask_model.precision = value

    # ---- device-side input prologue ----------------------------------------------------------
    def set_norm_values(self, mean: T.Optional[torch.Tensor], std: T.Optional[torch.Tensor],
                        log_transform: bool = False) -> None:
        """Per-channel z-score statistics (NormValues, utils/normalize.py:63-82) applied by the device prologue.
        ``log_transform``: the datasets' ``log_transform`` switch (data/datasets.py:481-484), passed where the statistics
        are, as upstream passes both to EdgeDataset: the prologue then takes log(x * 50 + 1) floored at 1e-9 before the
        z-score, and mean / std are statistics of the transformed values."""
        self._norm_mean, self._norm_std = mean, std
        self._log_transform = bool(log_transform)

    def set_augmenter(self, augmenter) -> None:
        """A cultionet_amd.augment.DeviceAugmenter (or None): raw labelled batches are augmented by the device prologue
        while the module is in training mode. Validation, test and predict batches never are: the reference sets
        augment_prob = 0 on every dataset but the training split (data/datasets.py:410-411)."""
        self._augmenter = augmenter

    def on_after_batch_transfer(self, batch: Data, dataloader_idx: int = 0) -> Data:
        """Lightning hook, called once the batch is on the GPU. A batch whose ``x`` is still RAW (integer
        reflectances, as stored by the reference's .pt files) is scaled / clipped / z-scored here by one HIP pass
        (cn_prepare_chips_f32) instead of per sample on the CPU in EdgeDataset.get (data/datasets.py:443-446):
        collate the raw samples with cultionet_amd.data.collate_fn and let the device do the arithmetic. Float
        batches (already prepared upstream) pass through untouched."""
        x = getattr(batch, "x", None)
        if x is None or not x.is_cuda or x.dtype == torch.float32:
            return batch
        from .edges import SCALE_FACTOR, prepare_chips

        aug = getattr(self, "_augmenter", None)
        log = getattr(self, "_log_transform", False)
        if aug is not None and self.training and getattr(batch, "y", None) is not None:
            return aug.apply(batch, getattr(self, "_norm_mean", None), getattr(self, "_norm_std", None), log_transform=log)
        batch.x = prepare_chips(x, getattr(self, "_norm_mean", None), getattr(self, "_norm_std", None), log_transform=log)
        bd = getattr(batch, "bdist", None)
        if bd is not None and bd.dtype != torch.float32:
            B = bd.shape[0]
            batch.bdist = prepare_chips(bd.reshape(B, 1, 1, *bd.shape[1:])).reshape(bd.shape)
        return batch

    def predict_step(self, batch: Data, batch_idx: int = None) -> T.Dict[str, torch.Tensor]:
        return self.forward(batch, batch_idx=batch_idx)

    @torch.no_grad()
    def get_true_labels(self, batch: Data, crop_type: torch.Tensor = None) -> T.Dict[str, T.Optional[torch.Tensor]]:
        """lightning.py:161-207. Kept for API compatibility (validation code reads these tensors); the training
        loss does not call it: the HIP loss kernel derives edge / crop / mask from ``batch.y`` on the fly."""
        y = batch.y
        ec = self.edge_class
        true_edge = (y == ec).long()
        true_crop = ((y > 0) & (y < ec)).long()
        mask = None
        if y.min() == -1:
            mask = (y != -1).long().unsqueeze(1)
        return {
            ValidationNames.TRUE_EDGE: true_edge,
            ValidationNames.TRUE_CROP: true_crop,
            ValidationNames.TRUE_CROP_AND_EDGE: (y > 0).long(),
            ValidationNames.TRUE_CROP_OR_EDGE: torch.where((y > 0) & (y < ec), 1, torch.where(y == ec, 2, 0)).long(),
            ValidationNames.TRUE_CROP_TYPE: torch.where(y == ec, 0, y).long() if crop_type is not None else None,
            ValidationNames.MASK: mask,
        }

    def _loss_terms(self, batch: Data):
        """(prediction key, kernel kwargs) of the three main losses of calc_loss (lightning.py:307-339).

        The weak-supervision mask ``y != -1`` is always applied in-kernel: when no -1 is present it is the
        identity, which removes the reference's device->host sync (``batch.y.min() == -1``, lightning.py:194).
        """
        y = batch.y
        if y.dtype != torch.int64:
            y = y.long()
        y = y.contiguous()
        ec = int(self.edge_class)
        return (
            (InferenceNames.DISTANCE, dict(target_f=batch.bdist.contiguous(), labels=y, target_mode=E.TGT_FLOAT,
                                           mask_mode=E.MSK_LABEL)),
            (InferenceNames.EDGE, dict(labels=y, target_mode=E.TGT_EQ, mask_mode=E.MSK_LABEL, klass=ec)),
            (InferenceNames.CROP, dict(labels=y, target_mode=E.TGT_RANGE, mask_mode=E.MSK_LABEL, klass=ec)),
        )

    def calc_loss(self, batch: T.Union[Data, T.List], predictions: T.Dict[str, torch.Tensor]):
        """lightning.py:209-354: (dist + edge + crop) / 3 and the report dict {dloss, eloss, closs}."""
        from .autograd_bridge import tanimoto_autograd

        kind = E.LOSS_KINDS[str(self.loss_name)]
        terms = []
        for key, kw in self._loss_terms(batch):
            terms.append(tanimoto_autograd(predictions[key], loss_kind=kind, **kw))
        loss = (terms[0] + terms[1] + terms[2]) / 3.0
        return loss, {"dloss": terms[0], "eloss": terms[1], "closs": terms[2]}

    def training_step(self, batch: Data, batch_idx: int = None):
        predictions = self(batch)
        loss, _ = self.calc_loss(batch, predictions)
        self.log("loss", loss, on_step=False, on_epoch=True, prog_bar=True, batch_size=batch.num_samples)
        return loss

    def probas_to_labels(self, x: torch.Tensor, thresh: float = 0.5) -> torch.Tensor:
        """lightning.py:126-136."""
        if x.shape[1] == 1:
            return x.gt(thresh).squeeze(dim=1).long()
        return x.argmax(dim=1).long()

    def _shared_eval_step(self, batch: Data, batch_idx: int = None) -> dict:
        """lightning.py:374-481: loss + the torchmetrics scores, computed on the device by ONE fused kernel
        (masked MAE / MSE, two 2x2 confusion matrices, micro F-beta = accuracy, MCC, checkpoint score): no
        torchmetrics round trips, no masked_select copies, no host sync."""
        from . import _lib

        with torch.no_grad():
            predictions = self(batch)
            loss, loss_report = self.calc_loss(batch, predictions)
            dist = predictions[InferenceNames.DISTANCE].float().contiguous()
            edge = predictions[InferenceNames.EDGE].float().contiguous()
            crop = predictions[InferenceNames.CROP].float().contiguous()
            if edge.shape[1] != 1 or crop.shape[1] != 1:
                raise NotImplementedError("the fused metrics kernel covers single-channel edge / crop maps")
            y = batch.y if batch.y.dtype == torch.int64 else batch.y.long()
            y = y.contiguous()
            bdist = batch.bdist.float().contiguous()
            dev = dist.device
            counts = E.alloc(11, torch.float64, dev)
            out = E.alloc(7, torch.float32, dev)
            lossd = loss.detach().float().reshape(1).contiguous()
            _lib.call("cn_eval_metrics_f32", dist.data_ptr(), edge.data_ptr(), crop.data_ptr(), bdist.data_ptr(),
                      y.data_ptr(), int(self.edge_class), 0.5, y.numel(), lossd.data_ptr(), counts.data_ptr(),
                      out.data_ptr(), E._stream())
        metrics = {
            "loss": loss,
            "dist_mae": out[0],
            "dist_mse": out[1],
            "edge_f1": out[2],
            "crop_f1": out[3],
            "edge_mcc": out[4],
            "crop_mcc": out[5],
            "score": out[6],
        }
        metrics.update(loss_report)
        return metrics

    def validation_step(self, batch: Data, batch_idx: int = None) -> dict:
        """lightning.py:483-508 (``val_score`` is what callbacks.py:246 checkpoints on)."""
        eval_metrics = self._shared_eval_step(batch, batch_idx)
        metrics = {
            "vef1": eval_metrics["edge_f1"],
            "vcf1": eval_metrics["crop_f1"],
            "vmae": eval_metrics["dist_mae"],
            "val_score": eval_metrics["score"],
            "val_loss": eval_metrics["loss"],
            "val_dloss": eval_metrics["dloss"],
            "val_eloss": eval_metrics["eloss"],
            "val_closs": eval_metrics["closs"],
        }
        self.log_dict(metrics, on_step=False, on_epoch=True, prog_bar=True, batch_size=batch.num_samples)
        if self.save_batch_val_metrics:
            self._save_batch_metrics(metrics, getattr(self, "current_epoch", 0), batch)
        return metrics

    def _save_batch_metrics(self, metrics: T.Dict[str, torch.Tensor], epoch: int, batch: Data) -> None:
        """lightning.py:510-533: appends the batch metrics to <logger.save_dir>/batch_metrics.parquet."""
        import pandas as pd

        trainer = getattr(self, "trainer", None)
        if trainer is not None and getattr(trainer, "sanity_checking", False):
            return
        logger = getattr(self, "logger", None)
        save_dir = getattr(logger, "save_dir", None) if logger is not None else None
        if save_dir is None:
            return
        ids = list(getattr(batch, "train_id", []) or [])
        write_metrics = {"epoch": [epoch] * len(ids), "train_ids": ids}
        for k, v in metrics.items():
            write_metrics[k] = [float(v)] * len(ids)
        metrics_file = Path(save_dir) / "batch_metrics.parquet"
        df = pd.DataFrame(write_metrics)
        if metrics_file.is_file():
            df = pd.concat((pd.read_parquet(metrics_file), df), axis=0)
        df.to_parquet(metrics_file)

    def test_step(self, batch: Data, batch_idx: int = None) -> dict:
        """lightning.py:535-560. Upstream also reads ``edge_dice`` / ``crop_dice`` / ``edge_jaccard`` / ``crop_jaccard``
        there, keys its _shared_eval_step never produces (a KeyError in the reference): the keys that exist are
        logged."""
        eval_metrics = self._shared_eval_step(batch, batch_idx)
        metrics = {
            "test_loss": eval_metrics["loss"],
            "tmae": eval_metrics["dist_mae"],
            "tmse": eval_metrics["dist_mse"],
            "tef1": eval_metrics["edge_f1"],
            "tcf1": eval_metrics["crop_f1"],
            "temcc": eval_metrics["edge_mcc"],
            "tcmcc": eval_metrics["crop_mcc"],
            "test_score": eval_metrics["score"],
        }
        self.log_dict(metrics, on_step=False, on_epoch=True, prog_bar=True)
        return metrics

    def configure_scorer(self):
        """lightning.py:562-577. The four torchmetrics scorers (MAE, MSE, micro F-beta(2), MCC) are evaluated by the
        fused HIP metrics kernel in _shared_eval_step; the attributes are kept (torchmetrics objects when that package
        is installed) for code that reaches for them."""
        try:
            import torchmetrics  # type: ignore

            self.mae_scorer = torchmetrics.MeanAbsoluteError()
            self.mse_scorer = torchmetrics.MeanSquaredError()
            self.f_beta_scorer = torchmetrics.FBetaScore(task="multiclass", num_classes=2, beta=2.0)
            self.mcc_scorer = torchmetrics.MatthewsCorrCoef(task="multiclass", num_classes=2)
        except Exception:
            self.mae_scorer = self.mse_scorer = self.f_beta_scorer = self.mcc_scorer = None

    def configure_loss(self):
        """lightning.py:589-609."""
        if str(self.loss_name) not in [str(k) for k in LOSS_DICT]:
            raise NameError(f"loss {self.loss_name!r} has no HIP kernel; choose one of {[str(k) for k in LOSS_DICT]}")
        entry = {str(k): v for k, v in LOSS_DICT.items()}[str(self.loss_name)]
        self.reg_loss = entry.get("regression")
        self.cls_loss = entry.get("classification")

    # The reference's optimizer / scheduler choices as data (lightning.py:611-683): name -> (torch class, which of the
    # module's hyper-parameters it takes, fixed keyword arguments). HipTrainer reads this table too: its fused kernels
    # implement all four natively.
    _OPTIMIZERS = {
        "Adam": ("Adam", ("lr", "eps"), {}),
        "AdamW": ("AdamW", ("lr", "weight_decay", "eps"), {"betas": (0.9, 0.98)}),
        "RAdam": ("RAdam", ("lr", "weight_decay", "eps"), {"betas": (0.9, 0.99), "decoupled_weight_decay": True}),
        "SGD": ("SGD", ("lr", "weight_decay"), {"momentum": 0.9}),
    }

    def _make_scheduler(self, optimizer):
        """(scheduler, stepping interval) for ``self.lr_scheduler``; OneCycleLR alone steps per batch."""
        from torch.optim import lr_scheduler as sched

        name = str(self.lr_scheduler)
        if name == str(LearningRateSchedulers.ONE_CYCLE_LR):
            tr = self.trainer
            return sched.OneCycleLR(optimizer, max_lr=self.learning_rate, epochs=tr.max_epochs,
                                    steps_per_epoch=tr.estimated_stepping_batches), "step"
        per_epoch = {
            str(LearningRateSchedulers.COSINE_ANNEALING_LR): lambda: sched.CosineAnnealingLR(optimizer, T_max=20, eta_min=1e-5,
                                                                                             last_epoch=-1),
            str(LearningRateSchedulers.EXPONENTIAL_LR): lambda: sched.ExponentialLR(optimizer, gamma=0.5),
            str(LearningRateSchedulers.STEP_LR): lambda: sched.StepLR(optimizer, step_size=self.steplr_step_size, gamma=0.5),
        }
        if name not in per_epoch:
            raise NameError("The learning rate scheduler is not implemented in Cultionet.")
        return per_epoch[name](), "epoch"

    #: True: ``configure_optimizers`` returns a cultionet_amd.optim.NativeOptimizer (clip + optimizer as one or two HIP
    #: launches over the flat parameter buffer, GradScaler without a host synchronisation) instead of the torch object
    native_optimizer = False

    def configure_optimizers(self):
        """Lightning hook, same choices and error behaviour as the reference (lightning.py:611-683): a torch optimizer over
        the model's parameters + one scheduler monitored on ``val_score``. With ``native_optimizer`` set the optimizer is
        the NativeOptimizer of the same kind and hyper-parameters; the scheduler entry is the same. (The native path --
        HipTrainer -- reads the same recipe table and runs clip + optimizer in cn_optim.hip, the schedule on the host.)"""
        recipe = self._OPTIMIZERS.get(str(self.optimizer))
        if recipe is None:
            raise NameError("Choose either 'AdamW' or 'SGD'.")
        cls_name, takes, fixed = recipe
        hyper = {"lr": self.learning_rate, "weight_decay": self.weight_decay, "eps": self.eps}
        params = list(self.cultionet_model.parameters())
        if self.native_optimizer:
            from .optim import NativeOptimizer

            if params[0].device.type != "cuda" or torch.version.hip is None:
                raise RuntimeError("native_optimizer needs the model on a ROCm device (its step is a HIP kernel)")
            optimizer = NativeOptimizer(params, self.cultionet_model.mask_model.param_store(), cls_name,
                                        **{k: hyper[k] for k in takes}, **fixed)
        else:
            optimizer = getattr(torch.optim, cls_name)(params, **{k: hyper[k] for k in takes}, **fixed)
        scheduler, interval = self._make_scheduler(optimizer)
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": scheduler, "name": "lr_sch", "monitor": "val_score", "interval": interval,
                                 "frequency": 1}}

    def configure_gradient_clipping(self, optimizer, gradient_clip_val=None, gradient_clip_algorithm=None):
        """Lightning hook. A NativeOptimizer clips inside its step (and under "16-mixed" it unscales there too, which is
        why Lightning's AMP plugin would refuse ``clip_gradients`` for it): the values are handed over and no gradient is
        touched. Any other optimizer: the base class's behaviour."""
        from .optim import NativeOptimizer

        if isinstance(optimizer, NativeOptimizer):
            optimizer.set_clip(gradient_clip_val, gradient_clip_algorithm)
            return
        super().configure_gradient_clipping(optimizer, gradient_clip_val, gradient_clip_algorithm)


class CultionetLitTransferModel(LightningModuleMixin):
    """lightning.py:686-818: transfer learning on a pretrained CultionetLitModel checkpoint.

    ``finetune``: "all" trains everything; "fc" freezes the network and unfreezes the ``mask_model.final_*`` heads;
    anything else (the default None) freezes the network and REPLACES final_a / final_b / final_c / final_combine by
    freshly initialised, trainable heads. Frozen parameters keep ``requires_grad=False``: torch optimizers skip them,
    and the HIP tape records no backward for the frozen tower in front of the heads (only the heads' backward runs).
    (A frozen layer a gradient must pass through still launches its data gradient; a fused kernel there writes the
    layer's frozen gradient slices too, which nothing reads.)
    HipTrainer trains the model natively (segmented clip + AdamW over the trainable parameters).
    """

    def __init__(
        self,
        pretrained_ckpt_file: T.Union[Path, str],
        in_channels: int,
        in_time: int,
        hidden_channels: int = 64,
        model_type: str = ModelTypes.TOWERUNET,
        dropout: float = 0.2,
        activation_type: str = "SiLU",
        dilations: T.Union[int, T.Sequence[int]] = None,
        res_block_type: str = ResBlockTypes.RESA,
        attention_weights: str = AttentionTypes.NATTEN,
        optimizer: str = "AdamW",
        loss_name: str = LossTypes.TANIMOTO_COMPLEMENT,
        learning_rate: float = 0.01,
        lr_scheduler: str = LearningRateSchedulers.ONE_CYCLE_LR,
        steplr_step_size: int = 5,
        weight_decay: float = 1e-3,
        eps: float = 1e-4,
        ckpt_name: str = "last_transfer",
        model_name: str = "cultionet_transfer",
        pool_by_max: bool = False,
        batchnorm_first: bool = False,
        class_counts: T.Optional[torch.Tensor] = None,
        edge_class: T.Optional[int] = None,
        scale_pos_weight: bool = False,
        save_batch_val_metrics: bool = False,
        finetune: T.Optional[str] = None,
    ):
        super().__init__()
        self.save_hyperparameters()
        from .nunet import init_conv_weights
        from .unet_parts import TowerUNetFinal, TowerUNetFinalCombine

        self.optimizer = optimizer
        self.loss_name = loss_name
        self.learning_rate = learning_rate
        self.lr_scheduler = lr_scheduler
        self.steplr_step_size = steplr_step_size
        self.weight_decay = weight_decay
        self.eps = eps
        self.ckpt_name = ckpt_name
        self.model_name = model_name
        self.in_time = in_time
        self.class_counts = class_counts
        self.scale_pos_weight = scale_pos_weight
        self.save_batch_val_metrics = save_batch_val_metrics
        self.finetune = finetune
        self.edge_class = edge_class if edge_class is not None else 2

        cultionet_model = CultionetLitModel.load_from_checkpoint(
            checkpoint_path=str(pretrained_ckpt_file)).cultionet_model
        if self.finetune != "all":
            self.freeze(cultionet_model)
            if self.finetune == "fc":
                for name, param in cultionet_model.named_parameters():
                    if name.startswith("mask_model.final_"):
                        param.requires_grad = True
            else:
                mm = cultionet_model.mask_model
                for attr, factor in (("final_a", 0), ("final_b", 2), ("final_c", 4)):
                    old = getattr(mm, attr)
                    new = TowerUNetFinal(in_channels=old.in_channels, num_classes=old.num_classes,
                                         activation_type=activation_type, resample_factor=factor)
                    new.apply(init_conv_weights)
                    setattr(mm, attr, new)
                fc = mm.final_combine
                new_fc = TowerUNetFinalCombine(num_classes=fc.num_classes, edge_activation=fc.edge_activation,
                                               mask_activation=fc.mask_activation)
                new_fc.apply(init_conv_weights)
                mm.final_combine = new_fc
                mm.__dict__["_cn_store"] = None  # modules were replaced: re-flatten the parameters on next use
        self.model_attr = f"{model_name}_{model_type}"
        setattr(self, self.model_attr, cultionet_model)
        # Upstream ALSO assigns ``self.cultionet_model = ...`` (lightning.py:742-744), which nn.Module.__setattr__ files
        # under _modules: its transfer checkpoints carry every tensor twice, as ``cultionet_model.*`` and as
        # ``cultionet_transfer_TowerUNet.*``. Registered under both names here too, so those checkpoints load strictly
        # and checkpoints written here hold the keys upstream expects (parameters() de-duplicates the shared module).
        self._modules["cultionet_model"] = cultionet_model
        self.configure_loss()
        self.configure_scorer()

    @property
    def is_transfer_model(self) -> bool:
        return True

    def freeze(self, layer):
        for param in layer.parameters():
            param.requires_grad = False

    def unfreeze(self, layer):
        for param in layer.parameters():
            param.requires_grad = True
        return layer


class CultionetLitModel(LightningModuleMixin):
    def __init__(
        self,
        in_channels: int,
        in_time: int,
        hidden_channels: int = 64,
        model_type: str = ModelTypes.TOWERUNET,
        dropout: float = 0.2,
        activation_type: str = "SiLU",
        dilations: T.Union[int, T.Sequence[int]] = None,
        res_block_type: str = ResBlockTypes.RESA,
        attention_weights: str = AttentionTypes.NATTEN,
        optimizer: str = "AdamW",
        loss_name: str = LossTypes.TANIMOTO_COMPLEMENT,
        learning_rate: float = 0.01,
        lr_scheduler: str = LearningRateSchedulers.ONE_CYCLE_LR,
        steplr_step_size: int = 5,
        weight_decay: float = 1e-3,
        eps: float = 1e-4,
        ckpt_name: str = "last",
        model_name: str = "cultionet",
        pool_by_max: bool = False,
        batchnorm_first: bool = False,
        class_counts: T.Optional[torch.Tensor] = None,
        edge_class: T.Optional[int] = None,
        scale_pos_weight: bool = False,
        save_batch_val_metrics: bool = False,
    ):
        super().__init__()
        self.save_hyperparameters()
        self.optimizer = optimizer
        self.loss_name = loss_name
        self.learning_rate = learning_rate
        self.lr_scheduler = lr_scheduler
        self.steplr_step_size = steplr_step_size
        self.weight_decay = weight_decay
        self.eps = eps
        self.ckpt_name = ckpt_name
        self.model_name = model_name
        self.in_time = in_time
        self.class_counts = class_counts
        self.scale_pos_weight = scale_pos_weight
        self.save_batch_val_metrics = save_batch_val_metrics
        self.edge_class = edge_class if edge_class is not None else 2
        self.model_attr = f"{model_name}_{model_type}"
        setattr(self, self.model_attr, CultioNet(
            in_channels=in_channels, in_time=in_time, hidden_channels=hidden_channels, model_type=model_type,
            dropout=dropout, activation_type=activation_type, dilations=dilations, res_block_type=res_block_type,
            attention_weights=attention_weights, pool_by_max=pool_by_max, batchnorm_first=batchnorm_first))
        self.configure_loss()
        self.configure_scorer()

    @property
    def is_transfer_model(self) -> bool:
        return False


class _PlanSlot:
    """Replay state of one phase of a step (HipTrainer): the recorded plan, the key the eager warm-up steps were counted
    under, and that count."""

    __slots__ = ("plan", "key", "eager_steps")

    def __init__(self):
        self.plan, self.key, self.eager_steps = None, None, 0


class HipTrainer:
    """Native training step: every FLOP and byte of forward + loss + backward + clip + optimizer in HIP kernels.

    Semantics of lightning.Trainer(gradient_clip_val=1.0, gradient_clip_algorithm=..., accumulate_grad_batches=...) +
    the optimizer ``lit.optimizer`` names, from the same recipe table as ``configure_optimizers`` (Adam, AdamW, RAdam,
    SGD with the reference's fixed arguments: model.py:84,168-186; lightning.py:611-655). The default -- AdamW, norm
    clipping, no accumulation -- is two launches (cn_grad_sumsq_f32 + cn_adamw_step_f32); Adam takes the same pair;
    SGD, RAdam and value clipping run in cn_optim_step_f32, value clipping without the reduction launch.

    Learning-rate schedule: ``lr_fn(step) -> lr`` (or ``-> (lr, beta1)``) when given; else ``total_steps`` => the
    reference's default OneCycleLR stepped per optimizer step (lightning.py:657-664; it also cycles the first-moment
    coefficient -- beta1, or SGD's momentum -- see cultionet_amd.schedules); else ``steps_per_epoch`` (optimizer steps
    per epoch) => the per-epoch scheduler ``lit.lr_scheduler`` names (CosineAnnealingLR, ExponentialLR, StepLR); else
    constant. With ``world_size > 1`` the flat gradient is all-reduced over RCCL in buckets overlapped with the
    backward tape (see cultionet_amd.ddp).

    ``accumulate_grad_batches=k``: every ``training_step`` is one micro-batch and returns its own loss; gradients add up
    in the flat buffer (zeroed before the first micro-batch of a group only) and clip + optimizer run after the k-th,
    on the sum divided by k. Step counts and the schedule advance per optimizer step. ``flush_accumulated()`` steps a
    trailing incomplete group (still dividing by k, as Lightning does on the last batch of an epoch). Under a
    communicator only the last micro-batch of a group all-reduces (Lightning's ``no_sync``): pass ``last=True`` to
    ``training_step`` for the last batch of an epoch.

    Frozen parameters (``requires_grad=False``: CultionetLitTransferModel, or any frozen set of submodules) get no
    update and no gradient is read for them (fused backward kernels may still write their slices), as torch optimizers skip parameters without ``.grad``; clipping sees the trainable
    gradients only, and every parameter keeps its own step count (bias corrections, RAdam's rectification). The
    trainable set is read at every step; it must not change inside a group of accumulated micro-batches.

    The optimizer state and the launches of a step are a cultionet_amd.optim.NativeOptimizer (``trainer.opt``):
    ``state_dict()`` / ``load_state_dict()`` stop and resume a run, or continue one from the optimizer state of a Lightning
    checkpoint and hand it back.

    ``pruner``: a cultionet_amd.pruning.MagnitudePruner of this model (``--model-pruning``): every step masks the
    gradient before clipping and the parameters after the update, ``prune(amount)`` runs a round between steps.
    """

    _KINDS = {"Adam": 0, "AdamW": 0, "SGD": 1, "RAdam": 2}  # CN_OPT_* of csrc/cn_optim.hip

    def __init__(self, lit: CultionetLitModel, gradient_clip_val: T.Optional[float] = 1.0,
                 lr_fn: T.Optional[T.Callable[[int], T.Union[float, T.Tuple[float, float]]]] = None, comm=None,
                 total_steps: T.Optional[int] = None, precision: str = "32-true", replay: bool = False,
                 gradient_clip_algorithm: str = "norm", accumulate_grad_batches: int = 1,
                 steps_per_epoch: T.Optional[int] = None, pruner=None):
        from .optim import NativeOptimizer

        self.lit = lit
        # replay=True: forward + loss + backward run from a recorded launch plan after the first steps
        # (cultionet_amd/replay.py): the Python of a step drops from ~8-10 ms to ~1.5 ms, which is what bounds the step at
        # the reference's default batch of 4 in mixed precision. Dropout replays too (the per-step part of the mask
        # seeds is a device word the plan's first launch bumps); a communicator keeps the step eager.
        # One plan per phase: a micro-step that zeroes the gradient and repacks the weights (the first of a group; every
        # step without accumulation) and one that does neither (the later micro-batches of a group).
        self.replay = bool(replay)
        self._slots = {False: _PlanSlot(), True: _PlanSlot()}  # key: does the micro-step accumulate?
        recipe = lit._OPTIMIZERS.get(str(lit.optimizer))
        if recipe is None:
            raise NameError("Choose either 'AdamW' or 'SGD'.")
        cls_name, takes, fixed = recipe
        self.opt_kind = self._KINDS[cls_name]
        betas = fixed.get("betas", (0.9, 0.999))  # (torch's default for Adam)
        self._beta1 = float(fixed.get("momentum", betas[0]))
        self._beta2 = float(betas[1])
        self._wd = float(lit.weight_decay) if "weight_decay" in takes else 0.0
        self._eps = float(lit.eps) if "eps" in takes else 0.0
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: choose 'norm' or 'value'")
        self.clip_algorithm = gradient_clip_algorithm
        if int(accumulate_grad_batches) != accumulate_grad_batches or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches must be a positive integer, got {accumulate_grad_batches!r}")
        self.accumulate = int(accumulate_grad_batches)
        self._micro = 0  # micro-batches in flat_grad since the last optimizer step
        self._reduced = True  # under a communicator: has flat_grad been all-reduced since the last micro-batch?
        self.model = lit.cultionet_model.mask_model
        self.store = self.model.param_store()
        dev = self.store.flat.device
        # the optimizer state (exp_avg, exp_avg_sq, every parameter's step count, the segment table of the trainable set)
        # and the launches of a step live in the NativeOptimizer, in torch's optimizer-state format: state_dict()
        hyper = {"lr": lit.learning_rate, "weight_decay": lit.weight_decay, "eps": lit.eps}
        self.opt = NativeOptimizer(list(lit.cultionet_model.parameters()), self.store, cls_name,
                                   **{k: hyper[k] for k in takes}, **fixed)
        # global magnitude pruning (cultionet_amd.pruning.MagnitudePruner): the step keeps pruned entries at zero
        if pruner is not None and pruner.store is not self.store:
            raise ValueError("the pruner belongs to another ParamStore than this model's")
        self.pruner = self.opt.pruner = pruner
        self.total = torch.zeros(1, dtype=torch.float32, device=dev)
        self.clip = gradient_clip_val
        if lr_fn is None:
            lr_fn = self._schedule(lit, total_steps, steps_per_epoch)
        self.lr_fn = lr_fn
        self.comm = comm
        # lightning.Trainer(precision=...) of the reference (model.py:168-186; default "16-mixed"): on MI355X the
        # mixed mode is bf16 activations + fp32 master weights / statistics / accumulation (no loss scaling needed)
        if precision not in ("32-true", "32", "bf16-mixed", "16-mixed"):
            raise ValueError(f"unsupported precision {precision!r}")
        self.bf16 = precision in ("bf16-mixed", "16-mixed")
        if self.bf16 and not getattr(self.model, "mixed_precision_ok", True):
            import warnings

            warnings.warn("cultionet_amd: the mixed-precision path needs channel counts that are multiples of 8 "
                          "(hidden_channels % 8 == 0); this trainer runs in fp32", stacklevel=2)
            self.bf16 = False
        # frozen parameters (requires_grad=False; CultionetLitTransferModel, partial training): the backward computes no
        # gradient for them and the optimizer step skips them, as torch optimizers do for parameters without .grad.
        # Every parameter keeps its own step count: ``_psteps`` (per parameter, store order) once a step has run
        # with frozen parameters; until then all share ``step_count`` and the step is the unsegmented one.
        self._mask = self._trainable_mask()
        if comm is not None:
            # torch DDP (the reference's strategy="ddp", model.py:101,184) broadcasts rank 0's parameters and buffers
            # at construction; dropout masks must differ per rank (each rank draws its own torch RNG stream upstream)
            comm.sync_initial_state(self.store, self.model)
            E.manual_seed(E._rng["seed"] + 0x9E37 * comm.rank)

    def _schedule(self, lit, total_steps: T.Optional[int], steps_per_epoch: T.Optional[int]):
        """``lr_fn`` for ``lit.lr_scheduler`` (the choices of LightningModuleMixin._make_scheduler)."""
        from . import schedules as S

        name = str(lit.lr_scheduler)
        if total_steps is None and steps_per_epoch is None:
            return S.ConstantLR(lit.learning_rate, self._beta1)
        if name == str(LearningRateSchedulers.ONE_CYCLE_LR):
            if total_steps is None:
                raise ValueError("OneCycleLR is stepped per optimizer step: pass total_steps (steps_per_epoch alone "
                                 "does not say how long the cycle is)")
            return S.OneCycleLR(lit.learning_rate, total_steps)
        per_epoch = {
            str(LearningRateSchedulers.COSINE_ANNEALING_LR): lambda: S.CosineAnnealingLR(lit.learning_rate),
            str(LearningRateSchedulers.EXPONENTIAL_LR): lambda: S.ExponentialLR(lit.learning_rate),
            str(LearningRateSchedulers.STEP_LR): lambda: S.StepLR(lit.learning_rate, lit.steplr_step_size),
        }
        if name not in per_epoch:
            raise NameError("The learning rate scheduler is not implemented in Cultionet.")
        if steps_per_epoch is None:
            raise ValueError(f"{name} is stepped per epoch: pass steps_per_epoch (optimizer steps per epoch); "
                             "total_steps alone does not say where an epoch ends")
        return S.PerEpoch(per_epoch[name](), steps_per_epoch, self._beta1)

    # the replay state of the zeroing phase under its historical names (the only phase without accumulation)
    @property
    def _plan(self):
        return self._slots[False].plan

    @_plan.setter
    def _plan(self, plan):
        self._slots[False].plan = plan

    @property
    def _plan_acc(self):
        """The recorded plan of an accumulating micro-step (no gradient zero-fill, no weight repack)."""
        return self._slots[True].plan

    @property
    def _accumulating(self) -> bool:
        """Does the next micro-batch add to gradients already in flat_grad?"""
        return self.accumulate > 1 and self._micro > 0

    def _trainable_mask(self) -> T.Tuple[bool, ...]:
        mask = self.store.trainable_mask()
        if not any(mask):
            # (upstream fails here too: loss.backward() on a graph without any parameter that requires a gradient)
            raise ValueError("every parameter of the model is frozen (requires_grad=False): nothing to train")
        return mask

    # the optimizer state under the names it had while it lived here
    @property
    def exp_avg(self) -> torch.Tensor:
        return self.opt.exp_avg

    @property
    def exp_avg_sq(self) -> T.Optional[torch.Tensor]:
        return self.opt.exp_avg_sq

    @property
    def sumsq(self) -> torch.Tensor:
        return self.opt.sumsq

    @property
    def step_count(self) -> int:
        """Optimizer steps taken (the schedule's clock; every parameter's step count until one is frozen)."""
        return self.opt.step_count

    @step_count.setter
    def step_count(self, value: int) -> None:
        self.opt.step_count = int(value)

    @property
    def _psteps(self) -> T.Optional[T.List[int]]:
        return self.opt._psteps

    @property
    def param_steps(self) -> T.List[int]:
        """Optimizer step count of every parameter (store order)."""
        return self.opt.param_steps

    def _segments(self):
        """Segment table of the current trainable set (rebuilt when that set changes)."""
        return self.opt.segments(self._mask)

    def forward_backward(self, batch: Data, last: bool = False) -> torch.Tensor:
        """Forward + loss + backward; adds d(loss)/d(params) of this micro-batch to store.flat_grad (the trainable slices
        when parameters are frozen), zeroed first unless the micro-batch continues a group. Returns the loss (1-elem
        tensor). ``last``: the group ends here (matters under a communicator, which all-reduces on a group's last
        micro-batch only)."""
        mask = self._trainable_mask()
        acc = self._accumulating
        if acc and mask != self._mask:
            raise RuntimeError("requires_grad changed inside a group of accumulated micro-batches: the gradients "
                               "already summed belong to another trainable set (change it after an optimizer step)")
        self._mask = mask
        if not acc:
            self._micro = 0
        self._sync = self.comm is not None and (last or self._micro + 1 >= self.accumulate)
        try:
            return self._forward_backward(batch, acc)
        finally:
            self._micro += 1
            self._reduced = self._sync

    def _forward_backward(self, batch: Data, acc: bool) -> torch.Tensor:
        if self.replay and self.comm is None and self.model.training:
            from . import replay as R

            slot = self._slots[acc]
            key = R.step_key(self, batch)
            if slot.plan is not None and slot.plan.key == key and not all(self._mask) and \
                    self.store._signature() != self.store._sig:
                # parameters were written outside the engine: the plan refreshes the trainable packs only
                self.store.refresh()
                slot.plan = None
            if slot.plan is not None and slot.plan.key == key:
                R.replay_step(slot.plan, batch)
                self.last_outputs = slot.plan.outputs
                return self.total
            if slot.key != key:  # new shapes / stream: two eager steps first (workspaces grow, packs are built)
                slot.key, slot.eager_steps, slot.plan = key, 0, None
            if slot.eager_steps >= 2:  # everything lazily created exists by now: record this step
                plan = R.record_step(self, batch, self._forward_backward_eager)
                slot.plan = plan if plan.key is not None else None  # (None: a scratch buffer moved while recording)
                return self.total
            slot.eager_steps += 1
        return self._forward_backward_eager(batch)

    def _forward_backward_eager(self, batch: Data) -> torch.Tensor:
        from . import _lib

        lit, store = self.lit, self.store
        kind = E.LOSS_KINDS[str(lit.loss_name)]
        with E.using_store(store), E.recording(True) as tape, E.mixed_precision(self.bf16):
            outs = self.model.forward_vars(self.model.input_var(batch.x))
            self.last_outputs = {k: v.t for k, v in outs.items()}  # distance / edge / crop of this step (no copies)
            # the three losses in one launch per pass; self.total = (dist + edge + crop) / 3 is written by the kernel
            terms = lit._loss_terms(batch)
            self.last_losses = E.tanimoto_loss_multi([outs[key] for key, _ in terms], [kw for _, kw in terms],
                                                     loss_kind=kind, weights=[1.0 / 3.0] * len(terms), total=self.total)
            if self._accumulating:  # every producer of a parameter gradient adds into flat_grad
                pass
            elif all(self._mask):
                store.zero_grad()
            else:  # the span of the trainable runs (frozen slices get no gradient and are never read)
                lo, hi = self._segments()[5]
                _lib.call("cn_fill_f32", store.flat_grad[lo:].data_ptr(), hi - lo, 0.0, E._stream())
            if self.comm is not None and self._sync:
                self.comm.backward(tape, store)
            else:  # (under a communicator: Lightning's no_sync for all but a group's last micro-batch)
                tape.backward()
        return self.total

    def optimizer_step(self) -> None:
        """Clip + optimizer over what flat_grad holds: the sum of the micro-batches since the last step, divided by
        ``accumulate_grad_batches`` (and by the world size)."""
        store = self.store
        if self.accumulate > 1 and self._micro == 0:
            raise RuntimeError("optimizer_step without a micro-batch since the last step: nothing accumulated")
        if self.comm is not None and not self._reduced:
            self.comm.reduce(store)  # a trailing group flushed without a ``last=True`` micro-batch
            self._reduced = True
        self._micro = 0
        scale = 1.0 / ((self.comm.world_size if self.comm is not None else 1) * self.accumulate)
        sched = self.lr_fn(self.opt.step_count + 1)
        lr, beta1 = sched if isinstance(sched, tuple) else (sched, self._beta1)
        # unsegmented while no parameter has ever been frozen, else over the trainable runs only, each with its own
        # step count (cultionet_amd.optim.launch_step)
        self.opt.step_flat(store.flat_grad.data_ptr(), self._mask, lr, beta1, self._beta2, self._eps, self._wd, scale,
                           self.clip, self.clip_algorithm)

    def prune(self, amount: T.Union[int, float]) -> int:
        """One round of global magnitude pruning (``MagnitudePruner.prune``) between optimizer steps; returns the
        number of entries pruned."""
        if self.pruner is None:
            raise RuntimeError("HipTrainer was built without a pruner")
        if self._micro != 0:
            raise RuntimeError("prune inside a group of accumulated micro-batches: the gradients summed so far were "
                               "taken with the weights about to be pruned (prune after an optimizer step)")
        return self.pruner.prune(amount)

    def state_dict(self) -> T.Dict[str, T.Any]:
        """What a resumed run needs besides the module's own state_dict: ``optimizer`` in torch's optimizer-state format
        (what ``torch.optim.<kind>.state_dict()`` holds after the same steps: it can go into ``optimizer_states[0]`` of a
        Lightning checkpoint), the schedule's clock and the accumulation phase, and ``pruner`` when one is attached.
        A copy: later steps do not change it."""
        import copy

        d = {"optimizer": copy.deepcopy(self.opt.state_dict()), "step_count": self.step_count, "micro": self._micro,
             "param_steps": self.param_steps}
        if self.pruner is not None:
            d["pruner"] = self.pruner.state_dict()
        return d

    def load_state_dict(self, d: T.Mapping[str, T.Any]) -> None:
        """Resume from ``state_dict()``. ``d["optimizer"]`` may equally be ``optimizer_states[0]`` of a Lightning
        checkpoint written with the torch optimizer or the NativeOptimizer; without ``step_count`` the schedule resumes
        from the largest step count in it. The state buffers are written in place: recorded replay plans stay valid."""
        if self._micro != 0 or int(d.get("micro", 0)) != 0:
            raise RuntimeError("load_state_dict inside a group of accumulated micro-batches: the gradients summed so far "
                               "belong to another state (load after an optimizer step, save after one)")
        self.opt.load_state_dict(d["optimizer"])
        steps = d.get("param_steps")
        if steps is not None and len(set(steps)) > 1:
            self.opt._psteps = [int(t) for t in steps]
        if "step_count" in d:
            self.opt.step_count = int(d["step_count"])
        if "pruner" in d:
            if self.pruner is None:
                raise RuntimeError("the state holds a pruner: build the trainer with pruner=MagnitudePruner(...)")
            self.pruner.load_state_dict(d["pruner"])

    def training_step(self, batch: Data, last: bool = False) -> torch.Tensor:
        """One micro-batch; the optimizer steps once ``accumulate_grad_batches`` of them are summed, or at once with
        ``last=True`` (Lightning steps on the last batch of an epoch whatever the group holds)."""
        loss = self.forward_backward(batch, last=last)
        if last or self._micro >= self.accumulate:
            self.optimizer_step()
        return loss

    def flush_accumulated(self) -> bool:
        """Step a trailing incomplete group of micro-batches (the sum is still divided by ``accumulate_grad_batches``).
        Returns whether there was one."""
        if self.accumulate == 1 or self._micro == 0:
            return False
        self.optimizer_step()
        return True
