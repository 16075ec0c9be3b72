"""Known answers for oracle/metrics_ref.MatthewsCorrCoef (the checker of the HIP metrics kernel): the regular formula
and the degenerate 2x2 branches of torchmetrics >= 1.0 (`_matthews_corrcoef_reduce`), computed by hand."""
import math

import numpy as np
import pytest
import torch


def _mcc(tp, fp, fn, tn):
    from oracle import metrics_ref as M

    preds = torch.tensor([1] * tp + [1] * fp + [0] * fn + [0] * tn)
    target = torch.tensor([1] * tp + [0] * fp + [1] * fn + [0] * tn)
    return float(M.MatthewsCorrCoef()(preds, target))


def test_regular_case():
    # tp 6, fp 1, fn 2, tn 3: (18 - 2) / sqrt(7 * 8 * 4 * 5)
    assert abs(_mcc(6, 1, 2, 3) - 16 / math.sqrt(1120)) < 1e-6


def test_all_right_and_all_wrong():
    assert _mcc(4, 0, 0, 5) == 1.0
    assert _mcc(0, 0, 0, 7) == 1.0   # a background chip predicted as background: no positives anywhere
    assert _mcc(0, 3, 2, 0) == -1.0


def test_empty_marginal_uses_the_eps_ratio():
    # no positive prediction, truth mixed: tp 0, fp 0, fn 3, tn 5 -> sqrt(eps) * (5 - 3) / sqrt(eps * 3 * 5 * 8)
    assert abs(_mcc(0, 0, 3, 5) - 2 / math.sqrt(120)) < 1e-5
    # no true positive, some predicted: tp 0, fn 0, fp 2, tn 6 -> sqrt(eps) * (6 - 2) / sqrt(2 * eps * 8 * 6)
    assert abs(_mcc(0, 2, 0, 6) - 4 / math.sqrt(96)) < 1e-5
    # more wrong than right with an empty marginal: negative
    assert _mcc(0, 0, 5, 1) < 0


# ---------------------------------------------------------------------------------------------------------------------
# tests/metrics_ref.py (the float64 restatement of cn_eval_metrics_f32) against oracle/metrics_ref.py
# ---------------------------------------------------------------------------------------------------------------------

def _torchmetrics_side(dist, edge, crop, bdist, y, klass, loss):
    """The reference's _shared_eval_step on the restated torchmetrics scorers (float32)."""
    from oracle import metrics_ref as M

    dist, edge, crop, bdist, y = (torch.from_numpy(np.ascontiguousarray(a)) for a in (dist, edge, crop, bdist, y))
    valid = y != -1
    te, tc = (y == klass).long()[valid], ((y > 0) & (y < klass)).long()[valid]
    pe, pc = (edge > 0.5).long()[valid], (crop > 0.5).long()[valid]
    mae, mse = M.MeanAbsoluteError()(dist[valid], bdist[valid]), M.MeanSquaredError()(dist[valid], bdist[valid])
    ef, cf = M.FBetaScore(beta=2.0)(pe, te), M.FBetaScore(beta=2.0)(pc, tc)
    em, cm = M.MatthewsCorrCoef()(pe, te), M.MatthewsCorrCoef()(pc, tc)
    score = loss + (1 - ef) + (1 - cf) + mae + (1 - em.clamp_min(0)) + (1 - cm.clamp_min(0))
    return torch.stack([mae, mse, ef, cf, em, cm, score]).float().numpy()


@pytest.mark.parametrize("klass", [2, 3])
def test_eval_metrics_ref_matches_the_torchmetrics_restatement(klass):
    """Random maps (with and without masked pixels) and the degenerate confusion matrices, each reaching the branch it
    is named for. 2e-6: the torchmetrics side is float32."""
    import metrics_ref as E

    seen = set()
    for name, dist, edge, crop, bdist, y in E.eval_cases(klass):
        c = E.eval_counts_ref(dist, edge, crop, bdist, y, klass, 0.5)
        got = E.eval_metrics_ref(c, 0.625)
        want = _torchmetrics_side(dist, edge, crop, bdist, y, klass, torch.tensor(0.625))
        worst = float(np.abs(got - want).max())
        print(f"eval_metrics_ref klass={klass} {name}: worst |diff| {worst:.2e} of 2e-6")
        assert worst <= 2e-6, (name, got, want)
        assert c[0] == (y != -1).sum() and c[3:7].sum() == c[0] and c[7:11].sum() == c[0]
        etp, efp, efn, etn = c[3:7]
        if name == "no positive edge prediction":
            assert etp + efp == 0 and efn > 0 and etn > 0 and 0 < abs(got[4]) < 1
        if name == "edge all right, crop all wrong":
            assert got[4] == 1.0 and got[5] == -1.0 and etp > 0 and c[8] > 0 and c[9] > 0
        if name == "no true and no predicted edge":
            assert etp + efp + efn == 0 and got[4] == 1.0
        if name == "no true edge, some predicted":
            assert etp + efn == 0 and efp > 0 and etn > 0 and 0 < abs(got[4]) < 1
        if name == "unmasked":
            assert c[0] == y.size
        seen.add(name)
    assert len(seen) == 6


def test_eval_counts_ref_rules():
    """Strictly greater than the threshold; labels above the edge class are neither edge nor crop; masked pixels,
    NaNs under them included, are skipped; a NaN at a valid pixel reaches the two sums and no confusion count."""
    import metrics_ref as E

    f = np.float32
    t = f(0.5)
    edge = np.array([np.nextafter(t, f(0)), t, np.nextafter(t, f(1)), 0.9, 0.9], dtype=np.float32)
    crop = edge[::-1].copy()
    dist = np.array([0.5, 0.25, 1.0, 0.75, np.nan], dtype=np.float32)
    bdist = np.array([0.25, 0.5, 0.0, 0.75, 0.0], dtype=np.float32)
    y = np.array([2, 2, 2, 3, -1])
    c = E.eval_counts_ref(dist, edge, crop, bdist, y, 2, 0.5)
    assert c.tolist() == [4, 1.5, 1.125, 1, 1, 2, 0, 0, 3, 0, 1]
    assert E.eval_counts_ref(dist, edge, crop, bdist, y, 3, 0.5).tolist() == [4, 1.5, 1.125, 1, 1, 0, 2, 3, 0, 0, 1]
    y[4] = 1
    c = E.eval_counts_ref(dist, edge, crop, bdist, y, 2, 0.5)
    assert c[0] == 5 and math.isnan(c[1]) and math.isnan(c[2]) and c[3:].tolist() == [1, 2, 2, 0, 0, 3, 1, 1]
    out = E.eval_metrics_ref(c, 0.5)
    assert math.isnan(out[0]) and math.isnan(out[1]) and math.isnan(out[6]) and np.isfinite(out[2:6]).all()


def test_eval_metrics_ref_of_an_empty_selection():
    """All pixels masked: n -> 1, zeros, the eps branch of the MCC (0 / eps^2 = 0), score = loss + 4."""
    import metrics_ref as E

    c = E.eval_counts_ref(np.ones(5, np.float32), np.ones(5, np.float32), np.ones(5, np.float32),
                          np.zeros(5, np.float32), np.full(5, -1), 2, 0.5)
    assert c.tolist() == [0.0] * 11
    assert E.eval_metrics_ref(c, 0.625).tolist() == [0, 0, 0, 0, 0, 0, 4.625]
    assert E.mcc_ref(6, 1, 2, 3) == 16 / math.sqrt(1120) and E.mcc_ref(0, 3, 2, 0) == -1.0 and E.mcc_ref(0, 0, 0, 7) == 1.0
    assert abs(E.mcc_ref(0, 0, 3, 5) - 2 / math.sqrt(120)) < 1e-7
    assert E.half_ulp32(np.array([1.0, 0.75, 0.0, 3.0])).tolist() == [2.0 ** -24, 2.0 ** -25, 0.0, 2.0 ** -23]
