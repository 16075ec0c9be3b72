"""Numpy restatement of the parcel side of the device augmentation stage (cultionet_amd/csrc/cn_parcels.hip and the
`roll` op of cn_augment.hip), without scipy: the GPU tests must not need it. tests/test_parcel_ref.py pins `label4` to
scipy.ndimage.label and `roll_parcels` to the reference's own roll_time (tests/golden/augment_roll.npz);
tests/test_parcel_augment_gpu.py holds the kernels to both.

  label4(y, crop_value)          y [H, W] or [B, H, W] -> (labels int32, counts int32 [B] or int): 4-connected components of
                                 y == crop_value, 0 on background, 1..n in raster order of each component's first pixel
  roll_parcels(x, labels, s)     x [C, T, H, W], labels [H, W], s [256]: out[c, t, h, w] = x[c, (t - s[k & 255]) mod T, h, w]
  fields                         the label planes both test files use
"""
import numpy as np

ROLL = 10  # op code of a `roll` plan row
PARCEL_SHIFTS = 256


def _label4_plane(fg):
    H, W = fg.shape
    labels = np.zeros((H, W), dtype=np.int32)
    n = 0
    for h0 in range(H):
        for w0 in range(W):
            if not fg[h0, w0] or labels[h0, w0]:
                continue
            n += 1  # first pixel of a new component in raster order
            labels[h0, w0] = n
            stack = [(h0, w0)]
            while stack:
                h, w = stack.pop()
                for a, b in ((h - 1, w), (h + 1, w), (h, w - 1), (h, w + 1)):
                    if 0 <= a < H and 0 <= b < W and fg[a, b] and not labels[a, b]:
                        labels[a, b] = n
                        stack.append((a, b))
    return labels, n


def label4(y, crop_value=1):
    y = np.asarray(y)
    if y.ndim == 2:
        return _label4_plane(y == crop_value)
    out = [_label4_plane(p == crop_value) for p in y]
    return np.stack([l for l, _ in out]), np.array([n for _, n in out], dtype=np.int32)


def roll_parcels(x, labels, shifts):
    x, labels, shifts = np.asarray(x), np.asarray(labels), np.asarray(shifts)
    C, T, H, W = x.shape
    assert labels.shape == (H, W) and shifts.shape == (PARCEL_SHIFTS,) and shifts[0] == 0
    s = shifts[labels & (PARCEL_SHIFTS - 1)]                       # [H, W]
    src = (np.arange(T).reshape(T, 1, 1) - s[None]) % T           # numpy's % is a true modulus
    return np.take_along_axis(x, np.broadcast_to(src[None], x.shape), axis=1)


def roll_entries(plan):
    """The `roll` rows of a cultionet_amd.augment.AugmentPlan: {b: shifts [256]}; every other word of such a row is 0."""
    out = {}
    for b in range(len(plan)):
        if int(plan.table[b, 0]) == ROLL:
            assert not plan.table[b, 1:].any()
            out[b] = plan.parcel[b].copy()
    return out


def shifts_of_props(prop_labels, prop_shifts):
    """The plan's table from the shifts the reference drew per prop (props carry the uint8 segment values)."""
    s = np.zeros(PARCEL_SHIFTS, dtype=np.int32)
    s[np.asarray(prop_labels)] = np.asarray(prop_shifts)
    return s


# ---- label planes ---------------------------------------------------------------------------------------------------

def checkerboard(H, W):
    return ((np.add.outer(np.arange(H), np.arange(W)) % 2) == 0).astype(np.int64)


def comb(N):
    """Vertical teeth in every other column, joined only along the bottom row: the equivalences resolve late."""
    y = np.zeros((N, N), dtype=np.int64)
    y[:, ::2] = 1
    y[N - 1, :] = 1
    return y


def spiral(N):
    """A one-pixel-wide spiral from the top-left corner inwards, one component, one background line between its arms."""
    y = np.zeros((N, N), dtype=np.int64)
    h, w, d, turns = 0, 0, 0, 0
    y[0, 0] = 1
    while turns < 2:
        dh, dw = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        a, b, a2, b2 = h + dh, w + dw, h + 2 * dh, w + 2 * dw
        free = 0 <= a < N and 0 <= b < N and not y[a, b] and not (0 <= a2 < N and 0 <= b2 < N and y[a2, b2])
        if free:
            h, w, turns = a, b, 0
            y[h, w] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return y


def lattice(N):
    y = np.zeros((N, N), dtype=np.int64)
    y[::2, ::2] = 1
    return y


def random_field(H, W, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.int64)


def classes_field(H, W, seed):
    """y in {-1, 0, 1, 2, 3}: unlabelled, background, crop, edge and one more class."""
    return np.random.default_rng(seed).integers(-1, 4, (H, W))


def fields():
    """name -> y [H, W] (crop pixels are 1): every plane the labelling is tested on."""
    out = {"1x1_fg": np.ones((1, 1), dtype=np.int64), "1x1_bg": np.zeros((1, 1), dtype=np.int64),
           "1x9": np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1]]), "9x1": np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1]]).T.copy(),
           "all_fg_13": np.ones((13, 13), dtype=np.int64), "all_bg_13": np.zeros((13, 13), dtype=np.int64),
           "checkerboard_13": checkerboard(13, 13), "comb_20": comb(20), "spiral_21": spiral(21),
           "lattice_34": lattice(34), "random_40": random_field(40, 40, 0.55, 40),
           "random_10x28": random_field(10, 28, 0.55, 28)}
    for density in (0.45, 0.59, 0.75):
        for seed in (1, 2, 3):
            out[f"random_64_{density}_{seed}"] = random_field(64, 64, density, 100 * seed + int(100 * density))
    # The kernel keeps its union-find plane in LDS up to 16 320 pixels and in the output plane beyond: the last plane
    # that fits, the first that does not, and the hard patterns again on the far side.
    out["random_120x136"] = random_field(120, 136, 0.59, 120)
    out["random_19x859"] = random_field(19, 859, 0.59, 19)
    out["random_127"] = random_field(127, 127, 0.59, 127)
    for density in (0.45, 0.59, 0.75):
        out[f"random_128_{density}"] = random_field(128, 128, density, 128 + int(100 * density))
    out.update({"checkerboard_129": checkerboard(129, 129), "comb_130": comb(130), "spiral_131": spiral(131),
                "lattice_130": lattice(130), "all_fg_128": np.ones((128, 128), dtype=np.int64)})
    return out
