"""Sliding-window scene prediction on the device (BASELINE configs[4]).

The reference predicts a scene by (a) cutting it into ``window_size`` chunks grown by ``padding`` on every side with
zero fill at the scene border and zero-filled to ``window_size + 2*padding`` squares
(/root/reference/src/cultionet/data/create.py:176-212, data/store.py:69-100), one ``.pt`` file per window; (b)
``EdgeDataset.get`` scaling each window (x/10000, clip(1e-9, 1), optional z-score; data/datasets.py:443-488,
utils/normalize.py:63-82); (c) ``predict_step``; (d) ``LightningGTiffWriter.write_on_batch_end`` slicing the padding
off, x10000, clip, and writing the window into the GeoTIFF (callbacks.py:176-227), one window at a time through
Python, numpy and a file lock.

Here the raw scene stays resident in HBM in its stored integer type; every batch of windows is cut + scaled + z-scored
by ONE kernel (cn_window_chips_f32), run through the HIP eval forward, and stitched into the uint16 [3, H, W] mosaic
by ONE kernel (cn_stitch_predictions_u16). File IO (GeoTIFF) stays with the caller.
"""
from __future__ import annotations

import typing as T

import torch

from . import _lib
from .edges import _DTYPES, LOG_FLOOR, LOG_GAIN, SCALE_FACTOR
from .engine import _stream


def window_origins(height: int, width: int, window_size: int) -> T.List[T.Tuple[int, int]]:
    """Row-major window origins (row_off, col_off): the chunk grid of data/create.py:176-182."""
    return [(r, c) for r in range(0, height, window_size) for c in range(0, width, window_size)]


class SlidingWindowPredictor:
    """``predict_scene(scene)``: raw [C, T, H, W] scene (f32 / i32 / i16 / u16, on the GPU) -> uint16 [3, H, W]
    (distance, edge, crop) x 10000, exactly the bands LightningGTiffWriter writes."""

    def __init__(self, lit, window_size: int = 100, padding: int = 5, batch_size: int = 8,
                 mean: T.Optional[torch.Tensor] = None, std: T.Optional[torch.Tensor] = None,
                 scale: float = 1.0 / SCALE_FACTOR, lo: float = 1e-9, hi: float = 1.0, precision: str = "32-true",
                 replay: bool = True, pixels_per_launch: T.Optional[int] = 400_000, log_transform: bool = False):
        if window_size <= 0 or padding < 0 or batch_size <= 0:
            raise ValueError("window_size, batch_size must be positive and padding non-negative")
        if pixels_per_launch is not None and pixels_per_launch < 0:
            raise ValueError("pixels_per_launch must be non-negative (None / 0: launch batch_size windows as given)")
        if precision not in ("32-true", "32", "bf16-mixed", "16-mixed"):
            raise ValueError(f"unsupported precision {precision!r}")
        # lightning.Trainer(precision=...) of the reference's predict entry (model.py:168-186): the mixed modes run the
        # TowerUNet body in bf16 NHWC on the MFMA bf16 path (fp32 parameters / running statistics / heads)
        self.bf16 = precision in ("bf16-mixed", "16-mixed")
        self.lit = lit
        self.ws, self.pad, self.bs = int(window_size), int(padding), int(batch_size)
        self.mean, self.std = mean, std
        self.scale, self.lo, self.hi = float(scale), float(lo), float(hi)
        # the predict dataset's log_transform (scripts/cultionet.py:171; data/datasets.py:481-484): log(v * 50 + 1) floored at
        # 1e-9 before the z-score, in the window kernel (cn_window_chips_log_f32). For a model trained with --log-transform.
        self.log_transform = bool(log_transform)
        # every full window batch has the same shape: its ~120 launches are recorded once and replayed
        # (cultionet_amd/replay.py) -- at the reference CLI's default batch of 4 the eager forward is host-bound
        self.replay = bool(replay)
        # ``batch_size`` is the reference's loop granularity (scripts/args.yml:248-254: 4 windows per forward), chosen for
        # GPUs where memory binds. The eval forward is independent per window (running statistics, no cross-sample op), so
        # consecutive batches are PACKED into one forward until it holds ~pixels_per_launch padded pixels (36 windows of
        # 110^2): a 4-window forward is ~165 dependent launches of a few microseconds each -- dispatch-bound at 23 Mpx/s
        # -- while the packed one fills the chip (50 Mpx/s). Same windows, same kernels, same mosaic.
        S = self.ws + 2 * self.pad
        self.launch_bs = self.bs if not pixels_per_launch else max(self.bs, -(-int(pixels_per_launch) // (S * S)))

    @torch.no_grad()
    def predict_scene(self, scene: torch.Tensor) -> torch.Tensor:
        if not scene.is_cuda:
            raise RuntimeError("predict_scene needs the scene on the GPU (there is no CPU fallback)")
        if scene.dim() != 4 or scene.dtype not in _DTYPES:
            raise ValueError("scene must be [C, T, H, W] of dtype f32 / i32 / i16 / u16")
        scene = scene.contiguous()
        C, Tn, H, W = scene.shape
        dev = scene.device
        S = self.ws + 2 * self.pad
        origins = window_origins(H, W, self.ws)
        rc = torch.tensor(origins, dtype=torch.int32).to(dev)
        out = torch.zeros((3, H, W), dtype=torch.uint16, device=dev)
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).reshape(-1).contiguous() if t is not None else None
        mean, std = f32(self.mean), f32(self.std)
        if mean is not None and mean.numel() != C:
            raise ValueError("mean / std must hold one value per channel")
        was_training = self.lit.training
        self.lit.eval()
        model = self.lit.cultionet_model.mask_model
        prev_replay = model.replay
        model.replay = self.replay
        try:
            per = self.launch_bs
            if per > self.bs:  # packed: even launches, and no ragged tail of a few windows (it costs a full forward)
                per = -(-len(origins) // max(1, round(len(origins) / per)))
            for i in range(0, len(origins), per):
                n = min(per, len(origins) - i)
                x = None
                if self.replay:  # write the window batch straight into the plan's input buffer (no copy)
                    from .replay import plan_input

                    x = plan_input(model, (n, C, Tn, S, S), self.bf16, dev)
                if x is None:
                    x = torch.empty((n, C, Tn, S, S), dtype=torch.float32, device=dev)
                args = (scene.data_ptr(), _DTYPES[scene.dtype], x.data_ptr(), rc[i:i + n].data_ptr(), n, C, Tn, H, W, S,
                        self.pad, mean.data_ptr() if mean is not None else None,
                        std.data_ptr() if std is not None else None, self.scale, self.lo, self.hi)
                if self.log_transform:
                    _lib.call("cn_window_chips_log_f32", *args, LOG_GAIN, LOG_FLOOR, _stream())
                else:
                    _lib.call("cn_window_chips_f32", *args, _stream())
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.bf16):
                    pred = model(x)
                d, e, c = (pred[k].float().contiguous() for k in ("distance", "edge", "crop"))
                _lib.call("cn_stitch_predictions_u16", d.data_ptr(), e.data_ptr(), c.data_ptr(), out.data_ptr(),
                          rc[i:i + n].data_ptr(), n, S, self.pad, self.ws, H, W, float(SCALE_FACTOR), _stream())
        finally:
            model.replay = prev_replay
            self.lit.train(was_training)
        return out
