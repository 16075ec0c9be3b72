"""The bound of the mixed-precision predict tests: a bf16 mosaic may differ from the fp32 one by no more than 1.5 x what
the REFERENCE's own bf16 run (oracle/predict_ref.predict_scene(autocast=True)) differs from its fp32 run on the same
scene -- the margin test_bf16_train_step_matches_reference gives over the reference's bf16 step. Nine statistics: the
mean, the 99.9th percentile and the max of |a - b| in counts, for each of the three bands (distance, edge, crop).

Shared by tests/test_predict_ref.py (CPU: the yardstick is steady from scene to scene, and mutants of the model exceed
the bound), tests/test_predict_edges_gpu.py and tests/test_sca_maxpool_bf16_model_gpu.py. Plain numpy.

Blind spots, shown by tests/test_predict_ref.py: an error below the bf16 noise of the whole model -- BatchNorm eps 1e-3
for 1e-5, a running_var off by 10 % -- stays under the bound; the per-kernel exact suites are what catch that class.
"""
from __future__ import annotations

import numpy as np

MARGIN = 1.5
BANDS = ("distance", "edge", "crop")
STATS = ("mean", "p99.9", "max")


def band_stats(a, b) -> np.ndarray:
    """[3 bands][mean, 99.9th percentile, max] of |a - b| for two [3, H, W] mosaics in counts."""
    d = np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)).astype(np.float64)
    assert d.ndim == 3 and d.shape[0] == 3
    return np.array([[band.mean(), np.percentile(band, 99.9), band.max()] for band in d])


def ratios(got: np.ndarray, yardstick: np.ndarray) -> np.ndarray:
    assert got.shape == yardstick.shape == (3, 3) and (yardstick > 0).all(), yardstick
    return got / yardstick


def assert_within_spread(what: str, got: np.ndarray, yardstick: np.ndarray) -> np.ndarray:
    """Every one of the nine statistics of `got` is at most MARGIN x the yardstick's; prints the ratios."""
    r = ratios(got, yardstick)
    for b, name in enumerate(BANDS):
        print(f"BOUND {what} {name}: " + ", ".join(
            f"{s} {got[b, j]:.1f} / {yardstick[b, j]:.1f} = {r[b, j]:.2f}" for j, s in enumerate(STATS)))
    assert (r <= MARGIN).all(), f"{what}: ratios to the reference's own bf16 spread {r.round(3).tolist()} exceed {MARGIN}"
    return r
