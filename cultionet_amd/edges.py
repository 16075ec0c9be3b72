"""Device-side input / output edges of the hot path.

``prepare_chips`` fuses what ``EdgeDataset.get`` + ``NormValues`` do on the CPU per sample
(/root/reference/src/cultionet/data/datasets.py:443-446, utils/normalize.py:63-82) into one HBM pass over the
collated batch: raw (integer) reflectances -> x/10000 -> clip(1e-9, 1) -> z-score, fp32.
``predictions_to_uint16`` is the arithmetic of ``LightningGTiffWriter.write_on_batch_end``
(callbacks.py:176-227): drop the window padding, x10000, clip, uint16 (the file IO stays with the caller).
"""
from __future__ import annotations

import typing as T

import torch

from . import _lib
from .engine import _stream

SCALE_FACTOR = 10_000.0
# ``--log-transform`` of the reference (scripts/args.yml:281-286; EdgeDataset.get, data/datasets.py:481-484):
# x = torch.log(x * 50.0 + 1.0).clamp_min(1e-9) after scale / clip / augmentation and before the z-score
LOG_GAIN, LOG_FLOOR = 50.0, 1e-9
_DTYPES = {torch.float32: 0, torch.int32: 1, torch.int16: 2, torch.uint16: 3}


def prepare_chips(x_raw: torch.Tensor, mean: T.Optional[torch.Tensor] = None, std: T.Optional[torch.Tensor] = None,
                  scale: float = 1.0 / SCALE_FACTOR, lo: float = 1e-9, hi: float = 1.0,
                  log_transform: bool = False) -> torch.Tensor:
    """x_raw: [B, C, T, H, W] on the GPU (f32 / i32 / i16 / u16); mean / std: exactly C values each (any shape), each
    optional on its own: the kernel indexes both by channel. ``log_transform``: the reference's ``--log-transform``,
    log(v * 50 + 1) floored at 1e-9 between the clip and the z-score, in the same pass (cn_prepare_chips_log_f32); mean and
    std must then be statistics of the transformed values."""
    if not x_raw.is_cuda:
        raise RuntimeError("prepare_chips needs a device tensor")
    if x_raw.dtype not in _DTYPES:
        raise TypeError(f"unsupported raw dtype {x_raw.dtype}")
    x_raw = x_raw.contiguous()
    B, C = x_raw.shape[0], x_raw.shape[1]
    L = int(x_raw[0, 0].numel())
    out = torch.empty(x_raw.shape, dtype=torch.float32, device=x_raw.device)
    m = mean.to(device=x_raw.device, dtype=torch.float32).reshape(-1).contiguous() if mean is not None else None
    s = std.to(device=x_raw.device, dtype=torch.float32).reshape(-1).contiguous() if std is not None else None
    if m is not None and m.numel() != C:
        raise ValueError("mean must hold one value per channel")
    if s is not None and s.numel() != C:
        raise ValueError("std must hold one value per channel")
    args = (x_raw.data_ptr(), _DTYPES[x_raw.dtype], out.data_ptr(), m.data_ptr() if m is not None else None,
            s.data_ptr() if s is not None else None, B, C, L, float(scale), float(lo), float(hi))
    if log_transform:
        _lib.call("cn_prepare_chips_log_f32", *args, LOG_GAIN, LOG_FLOOR, _stream())
    else:
        _lib.call("cn_prepare_chips_f32", *args, _stream())
    return out


def predictions_to_uint16(prediction: T.Dict[str, torch.Tensor], padding: int, height: int, width: int,
                          scale: float = SCALE_FACTOR) -> torch.Tensor:
    """{distance, edge, crop}: [B,1,H,W] device maps of one shape, fp32 or a narrower float type (the bf16-mixed forward
    returns bf16 maps; they are widened to fp32 first) -> uint16 [B,3,height,width] with the window padding removed."""
    maps = [prediction[k] for k in ("distance", "edge", "crop")]
    for k, t in zip(("distance", "edge", "crop"), maps):
        if not t.is_cuda:
            raise ValueError(f"predictions_to_uint16 needs device tensors, {k} is on {t.device}")
        if not t.is_floating_point():
            raise ValueError(f"{k} must be a floating-point map, got {t.dtype}")
        if t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"{k} must be [B, 1, H, W], got {tuple(t.shape)}")
        if t.shape != maps[0].shape or t.device != maps[0].device:
            raise ValueError(f"{k} is {tuple(t.shape)} on {t.device}, distance is {tuple(maps[0].shape)} on "
                             f"{maps[0].device}")
    B, _, H, W = maps[0].shape
    padding, height, width = int(padding), int(height), int(width)
    if padding < 0 or height < 0 or width < 0 or padding + height > H or padding + width > W:
        raise ValueError(f"padding {padding} + window {height} x {width} does not fit the {H} x {W} maps")
    d, e, c = (t.float().contiguous() for t in maps)
    out = torch.empty((B, 3, height, width), dtype=torch.uint16, device=d.device)
    _lib.call("cn_predictions_to_u16", d.data_ptr(), e.data_ptr(), c.data_ptr(), out.data_ptr(), B, H, W, padding,
              padding, height, width, float(scale), _stream())
    return out
