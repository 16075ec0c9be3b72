"""Float64 / bit-exact references of the pointwise kernels, shared by tests/test_pointwise_exact_gpu.py (GPU) and pinned
on the CPU by tests/test_pointwise_ref.py. Plain torch / numpy: no GPU, no import of the package's kernels.

* resize_matrix: F.interpolate(mode="bilinear", align_corners=True) as a matrix. The WEIGHTS are the fp32 ones ATen
  (and cn_bl_src of cn_index.h) computes -- index arithmetic restated in numpy.float32 -- held in float64; the
  contraction is float64. A float64 F.interpolate computes the weights in double and sits hundreds of fp32 units away.
* sca_ref64: SpatialChannelAttention as ResidualAConv applies it (nn.AdaptiveMaxPool2d(1) for the H*W maximum: first
  maximum; torch.amax for the channel maximum: gradient split evenly among ties).
* final_combine_ref: TowerUNetFinalCombine + SigmoidCrisp from the formula in the header of
  cn_final_combine_fwd_kernel.
* window_chips_ref / stitch_ref: numpy restatements of cn_window_chips_f32 / cn_stitch_predictions_u16. Every step is
  one IEEE fp32 operation with one rounding, so these are bit-exact, not approximate.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# bilinear resize, align_corners=True
# ---------------------------------------------------------------------------------------------------------------------

def resize_source(n_in: int, n_out: int):
    """i0, i1 (int64) and l1, h (float32) of every output index: ATen's area_pixel_compute_source_index in fp32."""
    f = np.float32
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)  # one rounding, no fused multiply-add
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    h = (f(1) - l1).astype(np.float32)
    return i0, i1, l1, h


def resize_matrix(n_in: int, n_out: int) -> torch.Tensor:
    """[n_out, n_in] float64: row o holds h at i0 and l1 at i1 (their float64 sum where the two coincide)."""
    i0, i1, l1, h = resize_source(n_in, n_out)
    R = np.zeros((n_out, n_in), dtype=np.float64)
    o = np.arange(n_out)
    np.add.at(R, (o, i0), h.astype(np.float64))
    np.add.at(R, (o, i1), l1.astype(np.float64))
    return torch.from_numpy(R)


def resize_fwd(x: torch.Tensor, Ho: int, Wo: int) -> torch.Tensor:
    """Ry @ x @ Rx^T in float64 over the last two axes."""
    Ry, Rx = resize_matrix(x.shape[-2], Ho), resize_matrix(x.shape[-1], Wo)
    return Ry @ x.double() @ Rx.t()


def resize_adj(dy: torch.Tensor, Hi: int, Wi: int) -> torch.Tensor:
    """The adjoint: Ry^T @ dy @ Rx."""
    Ry, Rx = resize_matrix(Hi, dy.shape[-2]), resize_matrix(Wi, dy.shape[-1])
    return Ry.t() @ dy.double() @ Rx


def candidates(n_in: int, n_out: int) -> torch.Tensor:
    """Per input index: how many outputs read it with a nonzero weight."""
    return (resize_matrix(n_in, n_out) != 0).sum(0)


# ---------------------------------------------------------------------------------------------------------------------
# spatial-channel attention
# ---------------------------------------------------------------------------------------------------------------------

def sca_ref64(mod, skip, out):
    """The reference's SpatialChannelAttention applied as ResidualAConv does, in float64 (torch.amax channel max,
    nn.AdaptiveMaxPool2d(1) H*W max). Returns y and the float64 leaves of the parameters by name."""
    fc1, fc2 = mod.channel_attention.fc1, mod.channel_attention.fc2
    w = lambda m: m.weight.detach().double().requires_grad_(True)
    w1a, w2a, w1m, w2m, wc = w(fc1[0]), w(fc1[2]), w(fc2[0]), w(fc2[2]), w(mod.spatial_attention.conv)
    gamma = mod.gamma.detach().double().requires_grad_(True)
    mlp = lambda v, a, b: F.conv2d(F.silu(F.conv2d(v, a)), b)
    ca = torch.sigmoid(mlp(skip.mean((2, 3), keepdim=True), w1a, w2a) + mlp(F.adaptive_max_pool2d(skip, 1), w1m, w2m))
    pooled = torch.cat([skip.mean(1, keepdim=True), skip.amax(1, keepdim=True)], 1)
    sa = torch.sigmoid(F.conv2d(pooled, wc, padding=1))
    y = out * (1.0 + gamma * ((ca + sa) * 0.5))
    names = {"channel_attention.fc1.0.weight": w1a, "channel_attention.fc1.2.weight": w2a,
             "channel_attention.fc2.0.weight": w1m, "channel_attention.fc2.2.weight": w2m,
             "spatial_attention.conv.weight": wc, "gamma": gamma}
    return y, names


def sca_pools64(x):
    """avg, mx [B,C] (first-maximum gradient), idx [B,C], channel mean and channel max [B,H,W] of a float64 x."""
    B, C = x.shape[:2]
    mx, idx = F.adaptive_max_pool2d(x, 1, return_indices=True)
    return x.mean((2, 3)), mx.view(B, C), idx.view(B, C), x.mean(1), x.amax(1)


# ---------------------------------------------------------------------------------------------------------------------
# TowerUNetFinalCombine + SigmoidCrisp
# ---------------------------------------------------------------------------------------------------------------------

def final_combine_ref(ha, hb, hc, params, smooth):
    """ha, hb, hc: float64 [B,3,H,W]; params: 16 float64 scalars, [3k+t] gamma of task k tower t, [9+k] weight,
    [12+k] bias, [15] crisp gamma. s_k = sum_t h_t[:, k] / gamma[k][t]; z_k = w_k s_k + b_k; dist, crop = sigmoid(z);
    edge = sigmoid(z_1 / (smooth + sigmoid(crisp))). Returns dist, edge, crop [B,1,H,W]."""
    outs = []
    for k in range(3):
        s = ha[:, k:k + 1] / params[3 * k] + hb[:, k:k + 1] / params[3 * k + 1] + hc[:, k:k + 1] / params[3 * k + 2]
        z = params[9 + k] * s + params[12 + k]
        if k == 1:
            z = z / (smooth + torch.sigmoid(params[15]))
        outs.append(torch.sigmoid(z))
    return tuple(outs)


# ---------------------------------------------------------------------------------------------------------------------
# predict tiling
# ---------------------------------------------------------------------------------------------------------------------

def window_chips_ref(scene, win_rc, T, S, pad, mean, std, scale, lo, hi):
    """scene: numpy [C*T][H][W] of float32 / int32 / int16 / uint16; win_rc: [(r0, c0)]; mean / std: float32 [C] or
    None. Window n = the crop at (r0 - pad, c0 - pad) of side S of the zero-extended scene, * scale, clipped to
    [lo, hi], z-scored with the fp32 reciprocal of std. float32 [nwin][C*T][S][S]."""
    f = np.float32
    P, H, W = scene.shape
    out = np.zeros((len(win_rc), P, S, S), dtype=np.float32)
    sc = scene.astype(np.float32)
    m = np.zeros(P, dtype=np.float32) if mean is None else np.repeat(np.asarray(mean, dtype=np.float32), T)
    inv = np.ones(P, dtype=np.float32) if std is None else (f(1) / np.repeat(np.asarray(std, dtype=np.float32), T))
    for n, (r0, c0) in enumerate(win_rc):
        ext = np.zeros((P, S, S), dtype=np.float32)
        ya, yb = max(r0 - pad, 0), min(r0 - pad + S, H)
        xa, xb = max(c0 - pad, 0), min(c0 - pad + S, W)
        if yb > ya and xb > xa:
            ext[:, ya - (r0 - pad):yb - (r0 - pad), xa - (c0 - pad):xb - (c0 - pad)] = sc[:, ya:yb, xa:xb]
        v = (ext * f(scale)).astype(np.float32)
        v = np.fmin(np.fmax(v, f(lo)), f(hi))
        out[n] = ((v - m[:, None, None]).astype(np.float32) * inv[:, None, None]).astype(np.float32)
    return out


def stitch_ref(dist, edge, crop, win_rc, S, pad, ws, H, W, scale):
    """dist / edge / crop: float32 [nwin][S][S]. Drops the padding, * scale in float32, clips to [0, scale] (a NaN
    clips to 0, as fmaxf), truncates to uint16 and writes each window, clipped at the scene's bottom and right edge,
    into a zero [3][H][W] mosaic."""
    f = np.float32
    out = np.zeros((3, H, W), dtype=np.uint16)
    for k, src in enumerate((dist, edge, crop)):
        for n, (r0, c0) in enumerate(win_rc):
            h, w = min(ws, H - r0), min(ws, W - c0)
            if h <= 0 or w <= 0:
                continue
            v = (np.asarray(src[n], dtype=np.float32)[pad:pad + h, pad:pad + w] * f(scale)).astype(np.float32)
            v = np.fmin(np.fmax(v, f(0)), f(scale))
            out[k, r0:r0 + h, c0:c0 + w] = v.astype(np.uint16)
    return out
