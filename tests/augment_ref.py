"""Float64 numpy restatement of the device augmentation stage (cultionet_amd/csrc/cn_augment.hip): the nine ops, the
pipeline around them and the counter-based Box-Muller noise. tests/test_augment_ref.py pins it to independent code
(torch's flip / rot90 / interpolate / conv2d, the reference's own Perlin generator through a recorded fixture);
tests/test_augment_gpu.py holds the kernels to it.

A sample is x [C, T, H, W], bdist [H, W], y [H, W]; a plan entry is a dict {"op": name, ...} with the op's parameters:
  gaussian: sigma      saltpepper: seed      cropresize: div, top, left      perlin: r, theta, phi ([2, r+1, r+1])

Where float32 enters the DEFINITION of an op it is kept: the resize source coordinates are what torch computes, in
float32 (scale = (float) in / out; bilinear max((d + 0.5) * s - 0.5, 0), nearest floor(d * s)), and the noise uniforms
are 24-bit dyadic rationals. Everything else is float64.
"""
import numpy as np

from attention_ref import splitmix64

OPS = ("none", "rot90", "rot180", "rot270", "fliplr", "flipud", "gaussian", "saltpepper", "cropresize", "perlin")
X_ONLY = ("gaussian", "saltpepper", "perlin")
F32 = np.float32


# ---- geometry -------------------------------------------------------------------------------------------------------

def permute(a, op):
    """Flips and rotations of the last two dims, written as explicit index maps (rot90 is counter-clockwise)."""
    H, W = a.shape[-2:]
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if op == "fliplr":
        return a[..., i, W - 1 - j]
    if op == "flipud":
        return a[..., H - 1 - i, j]
    if op == "rot180":
        return a[..., H - 1 - i, W - 1 - j]
    assert H == W, "rot90 / rot270 need a square plane"
    if op == "rot90":   # out[i][j] = in[j][N-1-i]
        return a[..., j, H - 1 - i]
    if op == "rot270":  # out[i][j] = in[N-1-j][i]
        return a[..., H - 1 - j, i]
    raise KeyError(op)


def bilinear_coords(out_size, in_size):
    """(i0, i1, weight of i1) per output index: align_corners=False, coordinates in float32 as torch evaluates them."""
    s = F32(in_size) / F32(out_size)
    d = np.arange(out_size, dtype=F32)
    f = np.maximum((d + F32(0.5)) * s - F32(0.5), F32(0.0))
    assert f.dtype == F32
    i0 = np.minimum(f.astype(np.int64), in_size - 1)
    i1 = np.minimum(i0 + 1, in_size - 1)
    return i0, i1, f.astype(np.float64) - i0


def nearest_coords(out_size, in_size):
    s = F32(in_size) / F32(out_size)
    f = np.floor(np.arange(out_size, dtype=F32) * s)
    assert f.dtype == F32
    return np.minimum(f.astype(np.int64), in_size - 1)


def resize_bilinear(a, H, W):
    h, w = a.shape[-2:]
    y0, y1, ly = bilinear_coords(H, h)
    x0, x1, lx = bilinear_coords(W, w)
    ly, lx = ly[:, None], lx[None, :]
    top = a[..., y0, :][..., x0] * (1 - lx) + a[..., y0, :][..., x1] * lx
    bot = a[..., y1, :][..., x0] * (1 - lx) + a[..., y1, :][..., x1] * lx
    return top * (1 - ly) + bot * ly


def resize_nearest(a, H, W):
    h, w = a.shape[-2:]
    return a[..., nearest_coords(H, h), :][..., nearest_coords(W, w)]


def crop(a, div, top, left):
    H, W = a.shape[-2:]
    h, w = H // div, W // div
    assert 0 <= top <= H - h and 0 <= left <= W - w
    return a[..., top:top + h, left:left + w]


# ---- x-only ops -----------------------------------------------------------------------------------------------------

def gaussian_taps(sigma):
    k = np.exp(-0.5 * (np.array([-1.0, 0.0, 1.0]) / float(sigma)) ** 2)
    return k / k.sum()


def gaussian_blur(x, sigma):
    """Separable 3 x 3 blur of every plane, reflect padding."""
    k = gaussian_taps(sigma)
    pad = [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)]
    p = np.pad(x, pad, mode="reflect")
    rows = k[0] * p[..., :, :-2] + k[1] * p[..., :, 1:-1] + k[2] * p[..., :, 2:]
    return k[0] * rows[..., :-2, :] + k[1] * rows[..., 1:-1, :] + k[2] * rows[..., 2:, :]


def normal_noise(seed, n):
    """n(i), i < n: Box-Muller on u1 = (top 24 bits of splitmix64(seed + 2i) + 1) / 2^24 in (0, 1] and
    u2 = (top 24 bits of splitmix64(seed + 2i + 1)) / 2^24 in [0, 1): sqrt(-2 ln u1) cos(2 pi u2)."""
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        c = np.uint64(seed) + np.uint64(2) * i
        z1, z2 = splitmix64(c), splitmix64(c + np.uint64(1))
    u1 = ((z1 >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (z2 >> np.uint64(40)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def perlin_field(T, H, W, r, theta, phi):
    """generate_perlin_noise_3d(shape=(T, H, W), res=(1, r, r), out_range=(-0.03, 0.03)) for given gradient angles."""
    assert H % r == 0 and W % r == 0
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    g = np.stack((np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)), axis=-1)  # [2, r+1, r+1, 3]
    dH, dW = H // r, W // r
    t, h, w = np.meshgrid(np.arange(T), np.arange(H), np.arange(W), indexing="ij")
    ih, iw = h // dH, w // dW
    ft, fh, fw = t / T, (h % dH) / dH, (w % dW) / dW

    def q(u):
        return u * u * u * (u * (u * 6 - 15) + 10)

    def corner(k, a, b):
        gv = g[k, ih + a, iw + b]
        return (ft - k) * gv[..., 0] + (fh - a) * gv[..., 1] + (fw - b) * gv[..., 2]

    qt, qh, qw = q(ft), q(fh), q(fw)
    n00 = corner(0, 0, 0) * (1 - qt) + qt * corner(1, 0, 0)
    n10 = corner(0, 1, 0) * (1 - qt) + qt * corner(1, 1, 0)
    n01 = corner(0, 0, 1) * (1 - qt) + qt * corner(1, 0, 1)
    n11 = corner(0, 1, 1) * (1 - qt) + qt * corner(1, 1, 1)
    n0 = (1 - qh) * n00 + qh * n10
    n1 = (1 - qh) * n01 + qh * n11
    return 0.06 * ((1 - qw) * n0 + qw * n1)


# ---- one sample, one batch ------------------------------------------------------------------------------------------

def augment_sample(x, bdist, y, entry):
    """Step 2 of the pipeline on values already in [1e-9, 1]: (x, bdist, y) -> (x, bdist, y)."""
    op = entry["op"]
    C, T, H, W = x.shape
    if op == "none":
        return x, bdist, y
    if op in ("rot90", "rot180", "rot270", "fliplr", "flipud"):
        return permute(x, op), permute(bdist, op), permute(y, op)
    if op == "gaussian":
        return gaussian_blur(x, entry["sigma"]), bdist, y
    if op == "saltpepper":
        return x + 0.01 * normal_noise(entry["seed"], x.size).reshape(x.shape), bdist, y
    if op == "cropresize":
        a = (entry["div"], entry["top"], entry["left"])
        return resize_bilinear(crop(x, *a), H, W), resize_bilinear(crop(bdist, *a), H, W), resize_nearest(crop(y, *a), H, W)
    if op == "perlin":
        return x + perlin_field(T, H, W, entry["r"], entry["theta"], entry["phi"])[None], bdist, y
    raise KeyError(op)


def pipeline(x_raw, bdist_raw, y, entries, mean=None, std=None, scale=1e-4, lo=1e-9, hi=1.0):
    """x_raw [B, C, T, H, W], bdist_raw [B, H, W], y [B, H, W] -> (x float64 z-scored, bdist float64, y int64):
    clip(raw * scale, lo, hi) -> op -> x.clip(lo, hi), bdist.clip(0, hi), y as int64 -> (x - mean[c]) / std[c]."""
    x = np.clip(np.asarray(x_raw, dtype=np.float64) * scale, lo, hi)
    bd = np.clip(np.asarray(bdist_raw, dtype=np.float64) * scale, lo, hi)
    y = np.asarray(y).astype(np.int64)
    xs, bs, ys = [], [], []
    for b, entry in enumerate(entries):
        xa, ba, ya = augment_sample(x[b], bd[b], y[b], entry)
        xs.append(np.clip(xa, lo, hi))
        bs.append(np.clip(ba, 0.0, hi))
        ys.append(ya.astype(np.int64))
    xo, bo, yo = np.stack(xs), np.stack(bs), np.stack(ys)
    if mean is not None:
        xo = xo - np.asarray(mean, dtype=np.float64).reshape(1, -1, 1, 1, 1)
    if std is not None:
        xo = xo / np.asarray(std, dtype=np.float64).reshape(1, -1, 1, 1, 1)
    return xo, bo, yo


def entries_of(plan):
    """The entries of a cultionet_amd.augment.AugmentPlan, read from its tables."""
    out = []
    for b in range(len(plan)):
        row = plan.table[b]
        e = {"op": OPS[int(row[0])], "div": int(row[1]), "top": int(row[2]), "left": int(row[3]), "r": int(row[4]),
             "sigma": float(row[5:6].view(np.float32)[0]),
             "seed": (int(row[6:8].view(np.uint32)[1]) << 32) | int(row[6:8].view(np.uint32)[0])}
        if e["op"] == "perlin":
            n = 2 * (e["r"] + 1) ** 2
            e["theta"] = plan.perlin[b, :n].reshape(2, e["r"] + 1, e["r"] + 1)
            e["phi"] = plan.perlin[b, n:2 * n].reshape(2, e["r"] + 1, e["r"] + 1)
        out.append(e)
    return out
