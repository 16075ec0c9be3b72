"""Float64 restatement of the fused validation-metrics kernel (cn_eval_metrics_f32 of cn_loss.hip), shared by
tests/test_edges_metrics_exact_gpu.py (GPU) and pinned on the CPU against the torchmetrics restatement
oracle/metrics_ref.py by tests/test_metrics_ref.py. Plain numpy: no GPU, no import of the package's kernels.

* eval_counts_ref: the 11 counts {n, sum |d|, sum d^2, edge tp / fp / fn / tn, crop tp / fp / fn / tn} over the pixels
  whose label is not -1. d = dist - bdist and |d| are formed in fp32, d^2 as a product of doubles, as in the kernel;
  every term is then exact in double and the two sums are correctly rounded (math.fsum), so only the ORDER of the
  kernel's double sum separates it from these: at most n 2^-53 of the sum. The eight confusion counts are integers.
  "Predicted positive" is strictly greater than the threshold in fp32; a NaN probability is not greater than anything.
* eval_metrics_ref: the 7 outputs {dist_mae, dist_mse, edge_f, crop_f, edge_mcc, crop_mcc, score} from the counts and
  the loss, with the three branches of ev_mcc and its eps-regularised ratio.
* eval_cases: the random maps and the four degenerate confusion matrices of
  test_eval_transfer_gpu.py::test_eval_metrics_kernel_against_restatement, for any edge class.
"""
from __future__ import annotations

import math

import numpy as np

EPS32 = 1.1920928955078125e-07  # float32 machine epsilon, the eps of torchmetrics' _matthews_corrcoef_reduce
NAMES = ("n", "sum|d|", "sum d^2", "edge tp", "edge fp", "edge fn", "edge tn", "crop tp", "crop fp", "crop fn", "crop tn")
OUT_NAMES = ("dist_mae", "dist_mse", "edge_f", "crop_f", "edge_mcc", "crop_mcc", "score")


def eval_counts_ref(dist, edge, crop, bdist, labels, klass, thresh):
    """dist / edge / crop / bdist: float32 arrays of one size (any shape); labels: integers of that size. Returns the
    11 counts as float64."""
    f = np.float32
    dist, edge, crop, bdist = (np.asarray(a, dtype=np.float32).reshape(-1) for a in (dist, edge, crop, bdist))
    y = np.asarray(labels).reshape(-1).astype(np.int64)
    valid = y != -1
    d = (dist[valid] - bdist[valid]).astype(np.float32)
    ad = np.abs(d).astype(np.float64)
    dd = d.astype(np.float64)
    c = np.zeros(11, dtype=np.float64)
    c[0] = float(valid.sum())
    c[1] = math.fsum(ad.tolist())
    c[2] = math.fsum((dd * dd).tolist())
    yv = y[valid]
    for at, truth, prob in ((3, yv == klass, edge[valid]), (7, (yv > 0) & (yv < klass), crop[valid])):
        with np.errstate(invalid="ignore"):
            pos = prob > f(thresh)
        c[at:at + 4] = [(pos & truth).sum(), (pos & ~truth).sum(), (~pos & truth).sum(), (~pos & ~truth).sum()]
    return c


def mcc_ref(tp, fp, fn, tn):
    """ev_mcc: every prediction right -> 1, every prediction wrong -> -1, the regular formula, and with an empty
    marginal the eps-regularised ratio."""
    if tp + tn != 0.0 and fp + fn == 0.0:
        return 1.0
    if tp + tn == 0.0 and fp + fn != 0.0:
        return -1.0
    den = (tp + fp) * (tp + fn) * (tn + fp) * (tn + fn)
    if den > 0.0:
        return (tp * tn - fp * fn) / math.sqrt(den)
    num = math.sqrt(EPS32) * ((tp + tn) - (fp + fn))
    return num / math.sqrt((tp + fp + EPS32) * (tp + fn + EPS32) * (tn + fp + EPS32) * (tn + fn + EPS32))


def eval_metrics_ref(counts, loss):
    """The finalize kernel in float64: counts as eval_counts_ref gives them, loss a float. 7 float64 values; an empty
    selection (n = 0) divides by 1."""
    c = [float(v) for v in counts]
    n = c[0] if c[0] > 0.0 else 1.0
    mae, mse = c[1] / n, c[2] / n
    ef, cf = (c[3] + c[6]) / n, (c[7] + c[10]) / n
    em, cm = mcc_ref(*c[3:7]), mcc_ref(*c[7:11])
    score = float(loss) + (1.0 - ef) + (1.0 - cf) + mae + (1.0 - (em if em > 0.0 else 0.0)) + \
        (1.0 - (cm if cm > 0.0 else 0.0))
    return np.array([mae, mse, ef, cf, em, cm, score], dtype=np.float64)


def half_ulp32(v):
    """Half an fp32 ulp at |v| (float64 array): spacing 2^(e-24) in the binade [2^(e-1), 2^e); 0 at 0."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, e - 25), 0.0)


def out_bound(ref, n):
    """Bound of the kernel's fp32 outputs against eval_metrics_ref: the store rounds once (half an fp32 ulp), the two
    double sums differ from the correctly rounded ones by their order (n 2^-53 each, n 2^-52 carried to a quotient and
    to the score), and the finalize kernel's fewer than 100 double operations on O(1) values stay below 1e-12."""
    ref = np.asarray(ref, dtype=np.float64)
    return half_ulp32(ref) + n * 2.0 ** -52 * np.abs(ref) + 1e-12


GRID = 1024  # grid_inputs: dist and bdist are k / GRID


def grid_inputs(n, seed, lo=-1, hi=3):
    """(dist, edge, crop, bdist, labels) with dist and bdist on the grid k / 1024 in [0, 1), edge and crop ~ U[0, 1),
    labels in lo..hi. On that grid d = dist - bdist is a multiple of 2^-10 below 1 in size, so d, |d| (fp32) and d * d
    (double, a multiple of 2^-20 below 1) are exact, and any partial sum of up to 2^20 of them is a multiple of 2^-20
    below 2^20: 40 significant bits, exact in double. The kernel's two real sums are then the same double WHATEVER the
    order of its additions (threads, blocks, atomics); grid_premise asserts all of this on the arrays themselves."""
    rng = np.random.default_rng(seed)
    dist, bdist = (rng.integers(0, GRID, n).astype(np.float32) / np.float32(GRID) for _ in range(2))
    edge, crop = (rng.random(n, dtype=np.float32) for _ in range(2))
    return dist, edge, crop, bdist, rng.integers(lo, hi + 1, n)


def grid_premise(dist, bdist, labels):
    """The premise under which the two real sums do not depend on the order of the additions, asserted on the inputs
    (NaN is allowed where the label is -1: the kernel never reads those pixels into a sum): at most 2^20 pixels, every
    valid dist and bdist is k / 1024 with 0 <= k < 1024, so that every |d| is a multiple of 2^-10 and every d^2 a
    multiple of 2^-20, both below 1 -- each partial sum is an integer below 2^40 times 2^-20."""
    dist, bdist = (np.asarray(a, dtype=np.float32).reshape(-1) for a in (dist, bdist))
    valid = np.asarray(labels).reshape(-1) != -1
    assert dist.size <= 1 << 20
    for a in (dist[valid], bdist[valid]):
        k = a.astype(np.float64) * GRID
        assert np.array_equal(k, np.round(k)) and (k >= 0).all() and (k < GRID).all()
    d = (dist[valid] - bdist[valid]).astype(np.float32)
    assert np.array_equal(d.astype(np.float64), dist[valid].astype(np.float64) - bdist[valid].astype(np.float64))
    ad, dd = np.abs(d).astype(np.float64), d.astype(np.float64) ** 2
    for t, step in ((ad, 2.0 ** 10), (dd, 2.0 ** 20)):
        assert np.array_equal(t * step, np.round(t * step)) and (t < 1.0).all()
        assert t.size * step < 2.0 ** 53  # every partial sum is an integer below 2^53, counted in units of 1 / step


def eval_cases(klass, seed=5, shape=(3, 37, 41)):
    """(name, dist, edge, crop, bdist, y) of test_eval_metrics_kernel_against_restatement for edge class `klass`, labels
    in -1..klass: random maps with and without masked pixels and the four degenerate confusion matrices -- no positive
    edge prediction (eps ratio), every edge prediction right and every crop prediction wrong (1 and -1), neither a true
    nor a predicted edge (1), and an empty truth marginal with some predictions (eps ratio)."""
    rng = np.random.default_rng(seed + klass)
    for name in ("masked", "unmasked", "no positive edge prediction", "edge all right, crop all wrong",
                 "no true and no predicted edge", "no true edge, some predicted"):
        dist, edge, crop, bdist = (rng.random(shape, dtype=np.float32) for _ in range(4))
        y = rng.integers(0 if name == "unmasked" else -1, klass + 1, shape)
        is_crop = (y > 0) & (y < klass)
        if name == "no positive edge prediction":
            edge = (edge * np.float32(0.4)).astype(np.float32)
        if name == "edge all right, crop all wrong":
            edge = np.where(y == klass, np.float32(0.9), np.float32(0.1)).astype(np.float32)
            crop = np.where(is_crop, np.float32(0.1), np.float32(0.9)).astype(np.float32)
        if name == "no true and no predicted edge":
            y = np.where(y == klass, 1, y)
            edge = (edge * np.float32(0.4)).astype(np.float32)
        if name == "no true edge, some predicted":
            y = np.where(y == klass, 0, y)
        yield name, dist, edge, crop, bdist, y
