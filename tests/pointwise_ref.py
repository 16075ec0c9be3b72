"""Float64 / bit-exact references of the pointwise kernels, shared by tests/test_pointwise_exact_gpu.py (GPU) and pinned
on the CPU by tests/test_pointwise_ref.py. Plain torch / numpy: no GPU, no import of the package's kernels.

* resize_matrix: F.interpolate(mode="bilinear", align_corners=True) as a matrix. The WEIGHTS are the fp32 ones ATen
  (and cn_bl_src of cn_index.h) computes -- index arithmetic restated in numpy.float32 -- held in float64; the
  contraction is float64. A float64 F.interpolate computes the weights in double and sits hundreds of fp32 units away.
* sca_ref64: SpatialChannelAttention as ResidualAConv applies it (nn.AdaptiveMaxPool2d(1) for the H*W maximum: first
  maximum; torch.amax for the channel maximum: gradient split evenly among ties).
* final_combine_ref: TowerUNetFinalCombine + SigmoidCrisp from the formula in the header of
  cn_final_combine_fwd_kernel.
* window_chips_ref / stitch_ref / prepare_chips_ref / predictions_u16_ref: numpy restatements of cn_window_chips_f32 /
  cn_stitch_predictions_u16 / cn_prepare_chips_f32 / cn_predictions_to_u16. Every step is one IEEE fp32 operation with
  one rounding, so these are bit-exact, not approximate.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from conv_exact_worker import half_ulp_bf16, ints

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

def sca_ref64(mod, skip, out, paths=False):
    """The reference's SpatialChannelAttention applied as ResidualAConv does, in float64 (torch.amax channel max,
    nn.AdaptiveMaxPool2d(1) H*W max). Returns y and the float64 leaves of the parameters by name.

    paths=True: each of the four pools (H*W average, H*W max, channel mean, channel max) reads its own leaf copy of
    skip, and the four leaves are returned as a third value: after y.backward() their .grad are the four paths'
    gradients into skip (their sum is d skip; `skip` itself then receives no gradient)."""
    fc1, fc2 = mod.channel_attention.fc1, mod.channel_attention.fc2
    w = lambda m: m.weight.detach().double().requires_grad_(True)
    w1a, w2a, w1m, w2m, wc = w(fc1[0]), w(fc1[2]), w(fc2[0]), w(fc2[2]), w(mod.spatial_attention.conv)
    gamma = mod.gamma.detach().double().requires_grad_(True)
    mlp = lambda v, a, b: F.conv2d(F.silu(F.conv2d(v, a)), b)
    s = [skip.detach().clone().requires_grad_(True) for _ in range(4)] if paths else [skip] * 4
    ca = torch.sigmoid(mlp(s[0].mean((2, 3), keepdim=True), w1a, w2a) + mlp(F.adaptive_max_pool2d(s[1], 1), w1m, w2m))
    pooled = torch.cat([s[2].mean(1, keepdim=True), s[3].amax(1, keepdim=True)], 1)
    sa = torch.sigmoid(F.conv2d(pooled, wc, padding=1))
    y = out * (1.0 + gamma * ((ca + sa) * 0.5))
    names = {"channel_attention.fc1.0.weight": w1a, "channel_attention.fc1.2.weight": w2a,
             "channel_attention.fc2.0.weight": w1m, "channel_attention.fc2.2.weight": w2m,
             "spatial_attention.conv.weight": wc, "gamma": gamma}
    return (y, names, s) if paths else (y, names)


def sca_pools64(x):
    """avg, mx [B,C] (first-maximum gradient), idx [B,C], channel mean and channel max [B,H,W] of a float64 x."""
    B, C = x.shape[:2]
    mx, idx = F.adaptive_max_pool2d(x, 1, return_indices=True)
    return x.mean((2, 3)), mx.view(B, C), idx.view(B, C), x.mean(1), x.amax(1)


def sca_pool_bwd_terms64(x, davg, dmx, dpool):
    """float64 autograd of the four pools, path by path: the gradients into x of the H*W average (davg / L), the H*W
    max (dmx to the FIRST maximum, nn.AdaptiveMaxPool2d(1)), the channel mean (dpool[:, 0] / C) and the channel max
    (dpool[:, 1] split evenly among the tied channels, torch.amax), and the sum of their absolute values."""
    B, C = x.shape[:2]
    xr = x.clone().requires_grad_(True)
    terms = [(xr.mean((2, 3)), davg), (F.adaptive_max_pool2d(xr, 1).view(B, C), dmx), (xr.mean(1), dpool[:, 0]),
             (xr.amax(1), dpool[:, 1])]
    grads = [torch.autograd.grad((t * d).sum(), xr, retain_graph=True)[0] for t, d in terms]
    return grads, sum(g.abs() for g in grads)


def sca_att64(ca, sconv, gamma):
    """att = 1 + g (a + sa), g = gamma / 2 (exact), with its fp32 error: sigmoid (|s| + 8) u sa, the add, the product
    and the add of 1 (one rounding each)."""
    B, C = ca.shape
    g = 0.5 * float(gamma)
    sa = torch.sigmoid(sconv)                                  # [B,1,H,W]
    inner = ca.view(B, C, 1, 1) + sa
    e_inner = (sconv.abs() + 8) * U32 * sa + U32 * inner
    att = 1 + g * inner
    mag = 1 + abs(g) * inner
    e_att = abs(g) * e_inner + U32 * abs(g) * inner + U32 * mag
    return g, sa, inner, e_inner, att, mag, e_att


# ---------------------------------------------------------------------------------------------------------------------
# bf16 spatial-channel attention and adaptive max pool (cn_sca_bf16.hip): tiling, cases, inputs, bounds
# ---------------------------------------------------------------------------------------------------------------------

def sca_tile(C, L):
    """G, R, pixels per block, blocks per image: 256 threads = R pixel rows x G = C/8 channel groups (R = 256 // G,
    threads past R*G idle), a block walks 8 such rows of pixels of one image."""
    G = C // 8
    R = 256 // G
    return G, R, 8 * R, -(-L // (8 * R))


# B, C, H, W, ld -- the corners of the tiling (see sca_tile)
SCA_BF16_SHAPES = [
    (2, 8, 5, 7, 16),          # 2048 px/block (s_max / s_dmax / s_dmean full), one partial block
    (1, 8, 3, 683, 8),         # L = 2049: one pixel in the second block
    (2, 24, 9, 11, 32),        # G = 3, R = 85: 680 px/block, one idle thread
    (1, 24, 3, 227, 24),       # L = 681: one pixel in the second block
    (1, 96, 25, 25, 104),      # 168 px/block
    (2, 1024, 5, 7, 1024),     # the launcher's limit: R = 2, 16 px/block, s_cs full
    (2, 256, 33, 33, 264),
]
# B, C, H, W -- planes of 2^k pixels: the backward's fl(1/L) and davg * fl(1/L) are exact
SCA_BF16_POW2 = [(2, 8, 32, 64), (2, 24, 32, 32), (1, 96, 16, 16), (1, 1024, 4, 8)]
SCA_POOL_BWD_D = 7  # fp32 roundings of cn_sca_pool_bwd_bf16 before the store, see sca_pool_bwd_bound


def bf_randn(shape, seed, scale=1.0):
    """bf16-representable N(0, scale^2) values as float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g, dtype=torch.float64) * scale).float().to(torch.bfloat16).double()


def f32_randn(shape, seed, scale=1.0):
    """fp32-representable N(0, scale^2) values as float64."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g, dtype=torch.float64) * scale).float().double()


def bf_few(shape, seed):
    """Multiples of 1/2 from five values (-1 .. 1): ties everywhere."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, tuple(shape), generator=g, dtype=torch.int64).double() * 0.5


def bf16_store_bound(ref, D, A, old=None):
    """Per-element bound of a bf16 store of an fp32 value that took D roundings on the way, each at most u = 2^-24 of
    A (the same expression on absolute values), and was then added to the buffer's old value (one more rounding, on
    A + |old|): e = D u A [+ u (A + |old|)]; the store rounds once more, half a bf16 ulp at |ref| + e."""
    e = D * U32 * A
    if old is not None:
        e = e + U32 * (A + old.abs())
    return e + half_ulp_bf16(ref.abs() + e)


def sca_pool_bwd_inputs(B, C, H, W, few, seed):
    """x (bf16-representable; few-valued or random), fp32 davg, dmx ~ N(0, 16), dpool ~ N(0, 1), bf16 base."""
    x = bf_few((B, C, H, W), seed) if few else bf_randn((B, C, H, W), seed)
    return x, f32_randn((B, C), seed + 1, 4.0), f32_randn((B, C), seed + 2, 4.0), \
        f32_randn((B, 2, H, W), seed + 3), bf_randn((B, C, H, W), seed + 4, 0.05)


def sca_pool_bwd_bound(ref, A, old=None):
    """cn_sca_pool_bwd_bf16: fl(1/L) (1) and davg * fl(1/L) (1), dpool0 / C (1), dpool1 / n (1), three adds (3):
    D = 7 on A = the sum of the four absolute terms; dmx and the masks are exact. `old`: the accumulated-into value."""
    return bf16_store_bound(ref, SCA_POOL_BWD_D, A, old)


def sca_pool_bwd_exact_inputs(B, C, H, W, seed):
    """The exact layer's data: per pixel 1, 2, 4 or 8 channels hold the pixel's maximum (1/2 or 1), the others are
    smaller multiples of 1/2; davg = integers * L, dmx integers, dpool0 = integers * C, dpool1 = integers * 8, base
    integers: every quotient and every sum of the kernel is an integer."""
    g = torch.Generator().manual_seed(seed)
    n = 2 ** torch.randint(0, 4, (B, 1, H, W), generator=g)
    rank = torch.rand(B, C, H, W, generator=g).argsort(1).argsort(1)
    top = torch.randint(1, 3, (B, 1, H, W), generator=g).double() * 0.5
    low = torch.randint(-2, 1, (B, C, H, W), generator=g, dtype=torch.int64).double() * 0.5
    x = torch.where(rank < n, top.expand(B, C, H, W), low)
    L = H * W
    davg, dmx = ints((B, C), -3, 3, seed + 1) * L, ints((B, C), -3, 3, seed + 2)
    dpool = torch.stack([ints((B, H, W), -3, 3, seed + 3) * C, ints((B, H, W), -3, 3, seed + 4) * 8], 1)
    return x, davg, dmx, dpool, ints((B, C, H, W), -8, 8, seed + 5)


def maxpool_bwd64(x, dy, size):
    """F.adaptive_max_pool2d's float64 y, idx, dx, the same on |dy| and the number of windows whose first maximum
    each input pixel is."""
    xr = x.clone().requires_grad_(True)
    y, idx = F.adaptive_max_pool2d(xr, size, return_indices=True)
    dx, dxa, cnt = (torch.autograd.grad(y, xr, g, retain_graph=True)[0] for g in (dy, dy.abs(), torch.ones_like(dy)))
    return y.detach(), idx, dx, dxa, cnt


# B, C, H, W, ld, few-valued x, accumulate: every bounded pool-backward case of the GPU module
SCA_POOL_BWD_BOUNDED = [s + (few, acc) for s in SCA_BF16_SHAPES for few in (True, False) for acc in (0, 1)]


def sca_gate_bound(v, att, mag, e_att, old=None):
    """bf16 store of v * att [+ old] (cn_sca_apply_fwd_bf16's y, cn_sca_apply_bwd_bf16's dout), att = 1 + g (ca + sa)
    within e_att of the fp32 factor (sca_att64): the factor's error, the product's rounding, with `old` one more add,
    then the store. Returns the float64 value and its bound."""
    ref = v * att + (0.0 if old is None else old)
    e = v.abs() * e_att + U32 * v.abs() * (mag + e_att)
    if old is not None:
        e = e + U32 * (v.abs() * (mag + e_att) + old.abs())
    return ref, e + half_ulp_bf16(ref.abs() + e)


# B, C, Hi, Wi, Ho, Wo, ld
MAXPOOL_BF16_CASES = [
    (2, 8, 7, 7, 3, 3, 16),          # windows [0,3) [2,5) [4,7): four of them share a pixel
    (1, 24, 25, 25, 12, 12, 32),
    (2, 8, 5, 9, 5, 9, 8),           # the identity window
]


def maxpool_inputs(B, C, Hi, Wi, Ho, Wo, seed):
    """Few-valued x (multiples of 1/2) with a strict maximum planted, in every plane, on one pixel that four windows
    share and on one that two share (where the windows overlap at all)."""
    x = bf_few((B, C, Hi, Wi), seed)
    own = lambda n_in, n_out: [sum(1 for o in range(n_out) if (o * n_in) // n_out <= i < -(-(o + 1) * n_in // n_out))
                               for i in range(n_in)]
    ny, nx = own(Hi, Ho), own(Wi, Wo)
    if max(ny) > 1 and max(nx) > 1:
        y2, x2 = ny.index(2), nx.index(2)
        x[:, :, y2, x2] = 2.0                       # in 2 x 2 windows
        x1 = max(i for i, n in enumerate(nx) if n == 1 and abs(i - x2) > 2)
        x[:, :, y2, x1] = 1.5                       # in 2 x 1 windows
    return x


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


def prepare_chips_ref(x, mean, std, scale, lo, hi):
    """x: numpy [B][C][...] of float32 / int32 / int16 / uint16; mean / std: float32 [C] or None, each on its own.
    cn_prepare_chips_f32 step by step, every step one IEEE fp32 operation with one rounding: x.astype(f32) * f32(scale),
    fmin(fmax(v, lo), hi) (a NaN clips to lo, as fmaxf), (v - mean[c]) * (f32(1) / std[c]). float32, the shape of x.

    Bit-exact against the kernel, NOT against the reference's (x / 10000).clip(1e-9, 1), (. - mean) / std: the rounded
    constant 1e-4 and the reciprocal-multiply move about a quarter of all values in their last bits.
    tests/test_pointwise_ref.py bounds that distance."""
    f = np.float32
    x = np.asarray(x)
    per_c = (1, x.shape[1]) + (1,) * (x.ndim - 2)
    v = (x.astype(np.float32) * f(scale)).astype(np.float32)
    v = np.fmin(np.fmax(v, f(lo)), f(hi))
    if mean is not None:
        v = (v - np.asarray(mean, dtype=np.float32).reshape(per_c)).astype(np.float32)
    if std is not None:
        v = (v * (f(1) / np.asarray(std, dtype=np.float32).reshape(per_c)).astype(np.float32)).astype(np.float32)
    return v


def predictions_u16_ref(dist, edge, crop, pad_top, pad_left, h, w, scale):
    """dist / edge / crop: float32 [B][1][H][W] (or [B][H][W]). cn_predictions_to_u16: the arithmetic of stitch_ref for
    one window per sample -- drop the padding, * scale in float32, clip to [0, scale] (a NaN clips to 0), truncate.
    uint16 [B][3][h][w]."""
    f = np.float32
    B = np.asarray(dist).shape[0]
    out = np.zeros((B, 3, h, w), dtype=np.uint16)
    for k, src in enumerate((dist, edge, crop)):
        s = np.asarray(src, dtype=np.float32)
        s = s.reshape(B, s.shape[-2], s.shape[-1])
        v = (s[:, pad_top:pad_top + h, pad_left:pad_left + w] * f(scale)).astype(np.float32)
        v = np.fmin(np.fmax(v, f(0)), f(scale))
        out[:, k] = v.astype(np.uint16)
    return out


def count_neighbours(n, seed, scale=10000.0):
    """n float32 probabilities on and next to integer counts: k / scale for random k in 0..scale, a third of them moved
    to the fp32 neighbour below and a third to the one above (the values of test_stitch_predictions_u16_bit_exact)."""
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, int(scale) + 1, n) / scale).astype(np.float32)
    step = rng.integers(-1, 2, n)
    v = np.where(step < 0, np.nextafter(v, np.float32(-1)), np.where(step > 0, np.nextafter(v, np.float32(2)), v))
    return v.astype(np.float32)


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
