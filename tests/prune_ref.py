"""The global magnitude pruning rule of cultionet_amd.pruning / csrc/cn_prune.hip restated with a sort (numpy, CPU).

A round prunes the ``k`` alive prunable entries first in the order (bits(|w|), flat index). Flags: one uint8 per flat
element, bit 0 alive, bit 1 prunable. Helpers for tests; no test lives here.
"""
import numpy as np

ALIVE, PRUNABLE = 1, 2


def keys(flat: np.ndarray) -> np.ndarray:
    """bits(|w|) of a float32 array: -0.0 and +0.0 share key 0, inf / NaN order above every finite value."""
    return np.ascontiguousarray(flat, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def round_count(amount, alive: int) -> int:
    """torch.nn.utils.prune._compute_nparams_toprune with the alive entries as the tensor size."""
    return int(amount) if isinstance(amount, int) else round(amount * alive)


def prune_round(flat: np.ndarray, flags: np.ndarray, k: int) -> np.ndarray:
    """The flags after a round of ``k``: a stable sort by key over the alive prunable entries in index order."""
    idx = np.nonzero((flags & 3) == 3)[0]
    assert 0 <= k <= idx.size
    order = np.argsort(keys(flat[idx]), kind="stable")
    out = flags.copy()
    out[idx[order[:k]]] &= np.uint8(0xFF ^ ALIVE)
    return out


def layout(sizes):
    """Offsets of a ParamStore over tensors of ``sizes`` elements (slices padded to 4) and the padded length."""
    offs, n = [], 0
    for s in sizes:
        offs.append(n)
        n += (s + 3) // 4 * 4
    return offs, n


def masked(src: np.ndarray, flags: np.ndarray) -> np.ndarray:
    """cn_mask_select_f32: +0.0 where pruned, ``src`` bit for bit elsewhere."""
    out = src.copy()
    out[(flags & 3) == PRUNABLE] = 0.0
    return out
