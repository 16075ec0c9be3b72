"""The loss and optimizer kernels (cn_loss.hip, cn_optim.hip) against float64 references at training shapes.

Losses: the oracle's own functions (oracle.towerunet_oracle) evaluated in float64 on the CPU on the same fp32 values,
with autograd for the gradients. AdamW: a float64 restatement of torch.optim.AdamW + clip_grad_norm_ stepping from the
kernel's own state, so every step is checked on its own.

Tolerances come from the arithmetic. The kernels sum in double and finalize in double, so a loss is one fp32 rounding
away from the reference: 2e-7 absolute. Gradients are fp32 expressions of fp32-rounded coefficients: 1e-5 of max|ref|,
with NO floor of 1.0 (a Tanimoto gradient is ~1/(B*C*H*W), and a floor would accept an all-zero gradient). Every
comparison prints its worst ratio (error / allowed) so the margins can be read from a -s run.
"""
import math
import types
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_ABS = 2e-7   # losses: a few fp32 ulps below 1
GRAD_REL = 1e-5   # gradients, AdamW updates and moments: of max|ref|
F32_EPS = 2.0 ** -23


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rel(got, ref, tol, what, floor=0.0):
    """max|got - ref| <= tol * max|ref| (+ floor): no 1.0 floor on the scale; 1e-30 only for an all-zero ref."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    scale = max(float(ref.abs().max()), 1e-30) if ref.numel() else 1e-30
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    bound = tol * scale + floor
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / bound:.3f}")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e} (scale {scale:.3e})"


def _abs(got, ref, tol, what):
    err = abs(float(got) - float(ref))
    print(f"{what}: err {err:.3e} ratio {err / tol:.3f}")
    assert err <= tol, f"{what}: {float(got)!r} vs {float(ref)!r} (err {err:.3e} > {tol:.3e})"


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference of one loss head
# ---------------------------------------------------------------------------------------------------------------------

def _ref_loss(pred, kind, tmode, *, labels=None, target_f=None, mask=None, mmode=0, klass=0, smooth=1e-5, depth=5):
    """(loss, dL/dpred) in float64 through the oracle: true_labels / loss_preprocess / the two distance functions."""
    from cultionet_amd import engine as E
    from oracle import towerunet_oracle as O

    C = pred.shape[1]
    x = pred.double().requires_grad_(True)
    if tmode == E.TGT_FLOAT:
        tgt, onehot = target_f.double().reshape(pred.shape), False
    elif tmode == E.TGT_ONEHOT:
        tgt, onehot = labels.clamp(min=0), True  # -1 pixels are masked; one_hot() needs a class index there
    else:
        te, tc, _ = O.true_labels(labels, klass)
        tgt, onehot = (te if tmode == E.TGT_EQ else tc), True
    m = None
    if mmode == E.MSK_LABEL:
        m = (labels != -1).long().unsqueeze(1)
    elif mmode in (E.MSK_I64, E.MSK_F32):
        m = mask.reshape(pred.shape[0], 1, *pred.shape[2:])
        m = m.double() if m.dtype == torch.float32 else m
    xi, t = O.loss_preprocess(x, tgt, m, onehot)
    t = t.double()
    assert xi.shape == t.shape == pred.shape or C == 1

    def comp():
        return ((O.tanimoto_complement_distance(t, xi, smooth, depth)
                 + O.tanimoto_complement_distance(1.0 - t, 1.0 - xi, smooth, depth)) * 0.5).mean()

    def dist():
        return ((O._tanimoto_dist(xi, t, smooth) + O._tanimoto_dist(1.0 - xi, 1.0 - t, smooth)) * 0.5).mean()

    loss = comp() if kind == 0 else dist() if kind == 1 else 0.5 * (dist() + comp())
    loss.backward()
    return float(loss.detach()), x.grad


def _inputs(B, C, H, W, tmode, mmode, klass, neg, seed):
    """fp32 CPU inputs of one head: pred in [0, 1], labels with (neg) or without -1, binary / fractional masks."""
    from cultionet_amd import engine as E

    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, C, H, W, generator=g)
    hi = C if tmode == E.TGT_ONEHOT else klass + 1
    labels = torch.randint(-1 if neg else 0, hi, (B, H, W), generator=g)
    target_f = torch.rand(B, C, H, W, generator=g) if tmode == E.TGT_FLOAT else None
    mask = None
    if mmode == E.MSK_I64:
        mask = torch.randint(0, 2, (B, 1, H, W), generator=g)
    elif mmode == E.MSK_F32:
        mask = torch.rand(B, 1, H, W, generator=g)
        mask[mask < 0.15] = 0.0  # exact zeros and ones beside the fractions
        mask[mask > 0.85] = 1.0
    uses_labels = tmode != E.TGT_FLOAT or mmode == E.MSK_LABEL
    return pred, (labels if uses_labels else None), target_f, mask


def _to(dev, t):
    return t.to(dev) if torch.is_tensor(t) else t


# ---------------------------------------------------------------------------------------------------------------------
# single head: engine.tanimoto_loss
# ---------------------------------------------------------------------------------------------------------------------
# id: (kind, target mode, C, klass, mask mode, -1 labels, (B, H, W), depth, smooth, weight)
T_FLOAT, T_EQ, T_RANGE, T_ONEHOT = 0, 1, 2, 3
M_NONE, M_LABEL, M_I64, M_F32 = 0, 1, 2, 3
SINGLE_CASES = {
    "float_c1_none_2x20": (0, T_FLOAT, 1, 0, M_NONE, False, (2, 20, 20), 5, 1e-5, 1.0),
    "float_c3_f32_2x20": (1, T_FLOAT, 3, 0, M_F32, False, (2, 20, 20), 5, 1e-2, 0.5),
    "eq_k2_label_neg_8x100": (0, T_EQ, 1, 2, M_LABEL, True, (8, 100, 100), 5, 1e-5, 1.0),
    "range_k2_label_noneg_32x100": (2, T_RANGE, 1, 2, M_LABEL, False, (32, 100, 100), 5, 1e-5, 1.0),
    "eq_k3_i64_odd": (1, T_EQ, 1, 3, M_I64, False, (3, 13, 9), 3, 1e-5, 2.5),
    "range_k3_none_4x256": (0, T_RANGE, 1, 3, M_NONE, False, (4, 256, 256), 8, 1e-5, 1.0),
    "onehot_c2_label_neg_2x20": (2, T_ONEHOT, 2, 0, M_LABEL, True, (2, 20, 20), 1, 1e-5, 1.0),
    "onehot_c3_f32_4x256": (0, T_ONEHOT, 3, 0, M_F32, False, (4, 256, 256), 5, 1e-2, 1.0),
    "onehot_c4_i64_odd": (1, T_ONEHOT, 4, 0, M_I64, False, (3, 13, 9), 5, 1e-5, 0.25),
    "float_c1_none_1x1": (0, T_FLOAT, 1, 0, M_NONE, False, (1, 1, 1), 3, 1e-5, 1.0),
    "onehot_c3_label_1x1": (2, T_ONEHOT, 3, 0, M_LABEL, False, (1, 1, 1), 5, 1e-2, 1.0),
    "eq_k2_label_neg_513": (0, T_EQ, 1, 2, M_LABEL, True, (513, 3, 3), 5, 1e-5, 0.75),
    "float_c1_f32_513": (2, T_FLOAT, 1, 0, M_F32, False, (513, 3, 3), 8, 1e-5, 1.0),
    "range_k2_i64_32x100": (1, T_RANGE, 1, 2, M_I64, False, (32, 100, 100), 1, 1e-2, 1.0 / 3.0),
    "eq_k3_label_neg_8x100": (2, T_EQ, 1, 3, M_LABEL, True, (8, 100, 100), 3, 1e-5, 1.0),
}


@pytest.mark.parametrize("case", list(SINGLE_CASES), ids=list(SINGLE_CASES))
def test_tanimoto_single_vs_float64(case):
    from cultionet_amd import engine as E

    kind, tmode, C, klass, mmode, neg, (B, H, W), depth, smooth, weight = SINGLE_CASES[case]
    dev = _dev()
    pred, labels, target_f, mask = _inputs(B, C, H, W, tmode, mmode, klass, neg, seed=zlib.crc32(case.encode()) % 10007)
    ref, gref = _ref_loss(pred, kind, tmode, labels=labels, target_f=target_f, mask=mask, mmode=mmode, klass=klass,
                          smooth=smooth, depth=depth)
    sentinel = 0.375
    total = torch.full((1,), sentinel, device=dev)
    with E.recording(True) as tape:
        pv = E.Var(pred.to(dev), True)
        loss = E.tanimoto_loss(pv, target_f=_to(dev, target_f), labels=_to(dev, labels), mask=_to(dev, mask),
                               target_mode=tmode, mask_mode=mmode, klass=klass, loss_kind=kind, weight=weight,
                               smooth=smooth, depth=depth, total=total)
        tape.backward()
    torch.cuda.synchronize()
    _abs(loss.item(), ref, LOSS_ABS, f"{case} loss")
    # the single kernel ADDS weight * loss to total (one fp32 multiply and add on top of the loss' own rounding)
    _abs(total.item(), sentinel + weight * ref, LOSS_ABS * weight + 2 * F32_EPS * (sentinel + weight), f"{case} total")
    _rel(pv.grad, weight * gref, GRAD_REL, f"{case} grad")
    if mmode != M_NONE:  # masked pixels: exactly zero gradient
        m = (labels != -1).unsqueeze(1) if mmode == M_LABEL else mask.reshape(B, 1, H, W) != 0
        assert (pv.grad.cpu()[~m.expand(B, C, H, W)] == 0).all(), case


def _parent_slice(parent_t, c0, c1, old_grad):
    """A Var that is channel slice [c0, c1) of a parent Var whose gradient already holds old_grad (engine.grad_buffer:
    the slice's gradient is then a strided view of the parent's, written with accumulate=1)."""
    from cultionet_amd import engine as E

    parent = E.Var(parent_t, True)
    parent.grad = old_grad.clone()
    v = E.Var(parent_t[:, c0:c1], True)
    v.parent = (parent, c0, c1)
    return parent, v


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_tanimoto_strided_pred_and_accumulated_slice_grad(kind):
    """pred is a channel slice of a wider tensor (pbs != C*HW); its gradient accumulates into the slice of a parent
    gradient holding random values (dbs != C*HW, accumulate=1); the parent's other channels stay bit-identical."""
    from cultionet_amd import engine as E

    dev = _dev()
    B, C, H, W, c0, wide = 8, 3, 25, 25, 2, 7
    g = torch.Generator().manual_seed(500 + kind)
    pred, labels, _, _ = _inputs(B, C, H, W, T_ONEHOT, M_LABEL, 0, True, seed=510 + kind)
    full = torch.rand(B, wide, H, W, generator=g)
    full[:, c0:c0 + C] = pred
    weight = 0.625
    ref, gref = _ref_loss(pred, kind, T_ONEHOT, labels=labels, mmode=M_LABEL)
    gscale = float(gref.abs().max()) * weight
    old = torch.randn(B, wide, H, W, generator=g) * gscale  # the same size as the gradient: a lost accumulate shows
    parent, pv = _parent_slice(full.to(dev), c0, c0 + C, old.to(dev))
    assert E.bstride(pv.t) == wide * H * W
    with E.recording(True) as tape:
        loss = E.tanimoto_loss(pv, labels=labels.to(dev), target_mode=T_ONEHOT, mask_mode=M_LABEL, loss_kind=kind,
                               weight=weight)
        tape.backward()
    torch.cuda.synchronize()
    _abs(loss.item(), ref, LOSS_ABS, f"strided kind {kind} loss")
    got = parent.grad.cpu()
    want = old[:, c0:c0 + C].double() + weight * gref
    _rel(got[:, c0:c0 + C] - old[:, c0:c0 + C], weight * gref, GRAD_REL, f"strided kind {kind} accumulated grad",
         floor=F32_EPS * float(want.abs().max()))
    assert torch.equal(got[:, :c0], old[:, :c0]) and torch.equal(got[:, c0 + C:], old[:, c0 + C:])


# ---------------------------------------------------------------------------------------------------------------------
# edge values
# ---------------------------------------------------------------------------------------------------------------------

def _single(pred, kind, **kw):
    from cultionet_amd import engine as E

    dev = _dev()
    with E.recording(True) as tape:
        pv = E.Var(pred.to(dev), True)
        loss = E.tanimoto_loss(pv, loss_kind=kind, **{k: _to(dev, v) for k, v in kw.items()})
        tape.backward()
    torch.cuda.synchronize()
    return loss.item(), pv.grad.cpu()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_tanimoto_fully_masked_sample(kind):
    B, C, H, W = 4, 2, 20, 20
    pred, labels, _, mask = _inputs(B, C, H, W, T_ONEHOT, M_I64, 0, False, seed=600 + kind)
    mask[2] = 0
    ref, gref = _ref_loss(pred, kind, T_ONEHOT, labels=labels, mask=mask, mmode=M_I64)
    loss, grad = _single(pred, kind, labels=labels, mask=mask, target_mode=T_ONEHOT, mask_mode=M_I64)
    _abs(loss, ref, LOSS_ABS, f"fully masked kind {kind} loss")
    assert (grad[2] == 0).all()
    _rel(grad, gref, GRAD_REL, f"fully masked kind {kind} grad")


EDGE_VALUES = ["pred_eq_target_binary", "all_zero", "pred_all_ones"]


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("case", EDGE_VALUES)
def test_tanimoto_edge_values(case, kind):
    """Exact 0/1 predictions: pred == binary target, pred and target all zero, pred all ones.

    In the first two both distances sit at their minimum and the exact gradient is 0 (all zero: the 1/smooth
    coefficients multiply y = yhat = 0). The kernel gets there by cancelling terms of the ordinary gradient's size, so
    the bound there is 1e-5 of the oracle's gradient at random predictions of the same shape and target."""
    B, C, H, W = 3, 1, 16, 16
    g = torch.Generator().manual_seed(700)
    target = (torch.rand(B, C, H, W, generator=g) > 0.5).float()
    if case == "pred_eq_target_binary":
        pred = target.clone()
    elif case == "all_zero":
        pred, target = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    else:
        pred = torch.ones(B, C, H, W)
    ref, gref = _ref_loss(pred, kind, T_FLOAT, target_f=target)
    loss, grad = _single(pred, kind, target_f=target, target_mode=T_FLOAT, mask_mode=M_NONE)
    _abs(loss, ref, LOSS_ABS, f"{case} kind {kind} loss")
    floor = 0.0
    if case != "pred_all_ones":
        _, gtyp = _ref_loss(torch.rand(B, C, H, W, generator=g), kind, T_FLOAT, target_f=target)
        floor = GRAD_REL * float(gtyp.abs().max())
    _rel(grad, gref, GRAD_REL, f"{case} kind {kind} grad", floor=floor)


# ---------------------------------------------------------------------------------------------------------------------
# several heads in one launch: engine.tanimoto_loss_multi
# ---------------------------------------------------------------------------------------------------------------------
# head: (C, target mode, klass, mask mode, -1 labels, accumulate into a parent slice)
MULTI_CASES = {
    "n1_b1": (1, (8, 8), [(2, T_ONEHOT, 0, M_LABEL, True, False)], [0.25], 0),
    "n2_b8": (8, (20, 20), [(3, T_FLOAT, 0, M_F32, False, True), (1, T_EQ, 2, M_I64, False, False)], [2.5, 1.0], 1),
    "n3_b32": (32, (25, 25), [(4, T_ONEHOT, 0, M_NONE, False, False), (1, T_RANGE, 3, M_LABEL, True, True),
                              (2, T_FLOAT, 0, M_LABEL, True, False)], [1.0, 2.5, 1.0 / 3.0], 2),
    "n4_b300_large_first": (300, (9, 11), [(4, T_ONEHOT, 0, M_I64, False, True), (3, T_FLOAT, 0, M_NONE, False, False),
                                           (2, T_ONEHOT, 0, M_LABEL, True, True), (1, T_EQ, 2, M_F32, False, False)],
                            [0.25, 1.0, 2.5, 1.0 / 3.0], 0),
    "n4_b8_mixed_c": (8, (100, 100), [(1, T_EQ, 3, M_LABEL, True, False), (3, T_FLOAT, 0, M_I64, False, True),
                                      (2, T_ONEHOT, 0, M_F32, False, False), (4, T_ONEHOT, 0, M_NONE, False, True)],
                      [0.25, 1.0, 2.5, 1.0 / 3.0], 1),
}


@pytest.mark.parametrize("case", list(MULTI_CASES), ids=list(MULTI_CASES))
def test_tanimoto_multi_vs_float64_and_single_calls(case):
    from cultionet_amd import engine as E

    B, (H, W), heads, weights, kind = MULTI_CASES[case]
    dev = _dev()
    wide = 5
    ins, refs, preds, parents, olds, terms = [], [], [], [], [], []
    for h, (C, tm, kl, mm, neg, acc) in enumerate(heads):
        pred, labels, tf, mask = _inputs(B, C, H, W, tm, mm, kl, neg, seed=800 + 31 * h + zlib.crc32(case.encode()) % 1000)
        ref, gref = _ref_loss(pred, kind, tm, labels=labels, target_f=tf, mask=mask, mmode=mm, klass=kl)
        refs.append((ref, weights[h] * gref))
        kw = dict(labels=_to(dev, labels), target_f=_to(dev, tf), mask=_to(dev, mask), target_mode=tm, mask_mode=mm,
                  klass=kl)
        terms.append(kw)
        ins.append((pred, kw))
        if acc:  # gradient accumulated into a parent slice that already holds values of the gradient's size
            full = torch.rand(B, wide, H, W)
            full[:, 1:1 + C] = pred
            old = torch.randn(B, wide, H, W) * float(refs[-1][1].abs().max())
            parent, pv = _parent_slice(full.to(dev), 1, 1 + C, old.to(dev))
            parents.append(parent)
            olds.append(old)
        else:
            pv = E.Var(pred.to(dev), True)
            parents.append(None)
            olds.append(None)
        preds.append(pv)
    sentinel = 7.0
    total = torch.full((1,), sentinel, device=dev)
    with E.recording(True) as tape:
        losses = E.tanimoto_loss_multi(preds, terms, loss_kind=kind, weights=weights, total=total)
        tape.backward()
    torch.cuda.synchronize()
    losses = losses.cpu()
    # n separate single-head calls on the same inputs (fresh Vars, no accumulation)
    singles = []
    for h, (pred, kw) in enumerate(ins):
        with E.recording(True) as tape:
            sv = E.Var(pred.to(dev), True)
            sl = E.tanimoto_loss(sv, loss_kind=kind, weight=weights[h], **kw)
            tape.backward()
        torch.cuda.synchronize()
        singles.append((sl.item(), sv.grad.cpu()))
    wl = sum(abs(w * r) for w, (r, _) in zip(weights, refs))
    # the total is WRITTEN with sum_h w_h * loss_h (fp32 products and sums, head order): the sentinel must be gone
    _abs(total.item(), sum(w * r for w, (r, _) in zip(weights, refs)),
         LOSS_ABS * sum(abs(w) for w in weights) + 2 * len(heads) * F32_EPS * wl, f"{case} total")
    for h, (C, tm, kl, mm, neg, acc) in enumerate(heads):
        ref, gref = refs[h]
        _abs(losses[h], ref, LOSS_ABS, f"{case} head {h} loss")
        _abs(losses[h], singles[h][0], LOSS_ABS, f"{case} head {h} loss vs single call")
        if acc:
            got = parents[h].grad.cpu()
            old = olds[h]
            _rel(got[:, 1:1 + C] - old[:, 1:1 + C], gref, GRAD_REL, f"{case} head {h} accumulated grad",
                 floor=F32_EPS * float((old[:, 1:1 + C].double() + gref).abs().max()))
            assert torch.equal(got[:, :1], old[:, :1]) and torch.equal(got[:, 1 + C:], old[:, 1 + C:])
        else:
            grad = preds[h].grad.cpu()
            _rel(grad, gref, GRAD_REL, f"{case} head {h} grad")
            _rel(grad, singles[h][1].double(), GRAD_REL, f"{case} head {h} grad vs single call")


@pytest.mark.parametrize("B,edge_class,kind", [(8, 2, 0), (32, 3, 0), (8, 3, 2), (32, 2, 1)])
def test_production_loss_terms_vs_calc_loss(B, edge_class, kind):
    """HipTrainer's loss: lit._loss_terms through tanimoto_loss_multi (weights 1/3) vs the oracle's calc_loss."""
    from cultionet_amd import engine as E
    from cultionet_amd.lightning import CultionetLitModel
    from oracle import towerunet_oracle as O

    dev = _dev()
    H = W = 100
    g = torch.Generator().manual_seed(900 + B + edge_class)
    y = torch.randint(-1, edge_class + 1, (B, H, W), generator=g)
    bdist = torch.rand(B, H, W, generator=g)
    pred = {k: torch.rand(B, 1, H, W, generator=g) for k in ("distance", "edge", "crop")}
    name = {0: "TanimotoComplementLoss", 1: "TanimotoDistLoss", 2: "TanimotoCombined"}[kind]
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=8, edge_class=edge_class, loss_name=name)
    terms = lit._loss_terms(types.SimpleNamespace(y=y.to(dev), bdist=bdist.to(dev)))
    p64 = {k: v.double().requires_grad_(True) for k, v in pred.items()}
    ref, parts = O.calc_loss(p64, y, bdist.double(), loss_name=name, edge_class=edge_class)
    ref.backward()
    total = torch.full((1,), -3.0, device=dev)
    with E.recording(True) as tape:
        pvs = [E.Var(pred[str(key)].to(dev), True) for key, _ in terms]
        losses = E.tanimoto_loss_multi(pvs, [kw for _, kw in terms], loss_kind=kind, weights=[1.0 / 3.0] * 3,
                                       total=total)
        tape.backward()
    torch.cuda.synchronize()
    _abs(total.item(), float(ref), LOSS_ABS + 6 * F32_EPS, f"B{B} e{edge_class} total")
    for h, part in enumerate(("dloss", "eloss", "closs")):
        _abs(losses[h].item(), float(parts[part]), LOSS_ABS, f"B{B} e{edge_class} {part}")
    for pv, (key, _) in zip(pvs, terms):
        _rel(pv.grad, p64[str(key)].grad, GRAD_REL, f"B{B} e{edge_class} grad {key}")


# ---------------------------------------------------------------------------------------------------------------------
# input checks: every one of these is rejected in Python, before any launch
# ---------------------------------------------------------------------------------------------------------------------

def _bad_single_inputs(dev):
    B, C, H, W = 2, 1, 6, 6
    ok = torch.rand(B, C, H, W, device=dev)
    lab = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    tf = torch.rand(B, C, H, W, device=dev)
    mk = torch.ones(B, 1, H, W, dtype=torch.int64, device=dev)
    wide = torch.rand(B, C, H, 2 * W, device=dev)
    return {
        "pred_bf16": (ok.to(torch.bfloat16).contiguous(memory_format=torch.channels_last),
                      dict(target_f=tf, target_mode=T_FLOAT, mask_mode=M_NONE)),
        "pred_f64": (ok.double(), dict(target_f=tf, target_mode=T_FLOAT, mask_mode=M_NONE)),
        "pred_inner_strided": (wide[..., ::2], dict(target_f=tf, target_mode=T_FLOAT, mask_mode=M_NONE)),
        "labels_missing_eq": (ok, dict(target_mode=T_EQ, mask_mode=M_NONE, klass=2)),
        "labels_missing_mask": (ok, dict(target_f=tf, target_mode=T_FLOAT, mask_mode=M_LABEL)),
        "labels_int32": (ok, dict(labels=lab.int(), target_mode=T_RANGE, mask_mode=M_NONE, klass=2)),
        "labels_strided": (ok, dict(labels=lab.transpose(1, 2), target_mode=T_EQ, mask_mode=M_NONE, klass=2)),
        "labels_batch_one": (ok, dict(labels=lab[:1], target_mode=T_EQ, mask_mode=M_LABEL, klass=2)),
        "target_missing": (ok, dict(target_mode=T_FLOAT, mask_mode=M_NONE)),
        "target_f64": (ok, dict(target_f=tf.double(), target_mode=T_FLOAT, mask_mode=M_NONE)),
        "target_strided": (ok, dict(target_f=tf.transpose(2, 3), target_mode=T_FLOAT, mask_mode=M_NONE)),
        "target_short": (ok, dict(target_f=tf[:1], target_mode=T_FLOAT, mask_mode=M_NONE)),
        "mask_missing": (ok, dict(target_f=tf, target_mode=T_FLOAT, mask_mode=M_I64)),
        "mask_f32_for_i64": (ok, dict(target_f=tf, mask=mk.float(), target_mode=T_FLOAT, mask_mode=M_I64)),
        "mask_i64_for_f32": (ok, dict(target_f=tf, mask=mk, target_mode=T_FLOAT, mask_mode=M_F32)),
        "mask_strided": (ok, dict(target_f=tf, mask=mk.transpose(2, 3), target_mode=T_FLOAT, mask_mode=M_I64)),
        "mask_batch_one": (ok, dict(target_f=tf, mask=mk[:1], target_mode=T_FLOAT, mask_mode=M_I64)),
        "mask_per_channel": (torch.rand(B, 3, H, W, device=dev),
                             dict(labels=lab, mask=mk.expand(B, 3, H, W).contiguous(), target_mode=T_ONEHOT,
                                  mask_mode=M_I64)),
        "mask_cpu": (ok, dict(target_f=tf, mask=mk.cpu(), target_mode=T_FLOAT, mask_mode=M_I64)),
        "unknown_mode": (ok, dict(target_f=tf, target_mode=7, mask_mode=M_NONE)),
    }


BAD_SINGLE = ["pred_bf16", "pred_f64", "pred_inner_strided", "labels_missing_eq", "labels_missing_mask", "labels_int32",
              "labels_strided", "labels_batch_one", "target_missing", "target_f64", "target_strided", "target_short",
              "mask_missing", "mask_f32_for_i64", "mask_i64_for_f32", "mask_strided", "mask_batch_one",
              "mask_per_channel", "mask_cpu", "unknown_mode"]


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("case", BAD_SINGLE)
def test_tanimoto_rejects_bad_inputs(case, multi):
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    dev = _dev()
    pred, kw = _bad_single_inputs(dev)[case]
    before = _lib.query("cn_launch_count", 0)
    with E.recording(False):
        with pytest.raises((RuntimeError, ValueError)):
            if multi:  # the bad head second, behind a valid one of the same shape
                good = dict(target_f=torch.rand(pred.shape[0], 1, *pred.shape[2:], device=dev), target_mode=T_FLOAT,
                            mask_mode=M_NONE)
                E.tanimoto_loss_multi([E.Var(torch.rand_like(good["target_f"])), E.Var(pred)], [good, kw])
            else:
                E.tanimoto_loss(E.Var(pred), **kw)
    assert _lib.query("cn_launch_count", 0) == before, "a launch happened before the check"


def test_tanimoto_multi_rejects_bad_head_counts():
    from cultionet_amd import engine as E

    dev = _dev()
    t = torch.rand(2, 1, 4, 4, device=dev)
    kw = dict(target_f=t, target_mode=T_FLOAT, mask_mode=M_NONE)
    with E.recording(False):
        with pytest.raises(ValueError):
            E.tanimoto_loss_multi([], [])
        with pytest.raises(ValueError):
            E.tanimoto_loss_multi([E.Var(t)] * 5, [kw] * 5)
        with pytest.raises(ValueError):
            E.tanimoto_loss_multi([E.Var(t)] * 2, [kw])
        with pytest.raises(ValueError):
            E.tanimoto_loss_multi([E.Var(t)] * 2, [kw] * 2, weights=[1.0])


# ---------------------------------------------------------------------------------------------------------------------
# the drop-in nn.Module losses: broadcast masks / targets as LossPreprocessing takes them
# ---------------------------------------------------------------------------------------------------------------------
BROADCAST_CASES = {
    # id: (loss class, C, targets shape, mask shape or None, mask dtype)
    "mask_1x1xHxW_onehot": ("TanimotoComplementLoss", 3, "BHW", (1, 1), torch.int64),
    "mask_BxHxW_float": ("TanimotoDistLoss", 1, "BHW", ("B",), torch.float32),
    "labels_1xHxW_onehot": ("CombinedLoss", 3, "1HW", ("B", 1), torch.int64),
    "targets_1xHxW_float_mask_HxW": ("TanimotoComplementLoss", 1, "1HW", (), torch.float32),
}


@pytest.mark.parametrize("case", list(BROADCAST_CASES), ids=list(BROADCAST_CASES))
def test_module_losses_broadcast_like_loss_preprocess(case):
    from cultionet_amd import losses as L
    from oracle import towerunet_oracle as O

    cls, C, tshape, mshape, mdtype = BROADCAST_CASES[case]
    dev = _dev()
    B, H, W = 4, 12, 10
    g = torch.Generator().manual_seed(1000 + zlib.crc32(case.encode()) % 1000)
    pred = torch.rand(B, C, H, W, generator=g)
    nb = B if tshape == "BHW" else 1
    if C > 1:
        targets = torch.randint(0, C, (nb, H, W), generator=g)
    else:
        targets = torch.rand(nb, H, W, generator=g)
    mask = None
    if mshape is not None:
        shape = tuple(B if d == "B" else d for d in mshape) + (H, W)
        mask = torch.randint(0, 2, shape, generator=g).to(mdtype)
        if mdtype == torch.float32:
            mask = mask * torch.rand(shape, generator=g)  # fractional
    if cls == "CombinedLoss":
        mod = L.CombinedLoss([L.TanimotoDistLoss(), L.TanimotoComplementLoss()])
        ofn = O.tanimoto_combined_loss
    else:
        mod = getattr(L, cls)()
        ofn = O.tanimoto_complement_loss if cls == "TanimotoComplementLoss" else O.tanimoto_dist_loss
    x64 = pred.double().requires_grad_(True)
    m64 = mask.double() if mask is not None and mask.is_floating_point() else mask
    t64 = targets.double() if targets.is_floating_point() else targets
    ref = ofn(x64, t64, m64)
    ref.backward()
    pd = pred.to(dev).requires_grad_(True)
    loss = mod(pd, targets.to(dev), mask.to(dev) if mask is not None else None)
    loss.backward()
    torch.cuda.synchronize()
    _abs(loss.item(), float(ref), LOSS_ABS, f"{case} loss")
    _rel(pd.grad, x64.grad, GRAD_REL, f"{case} grad")


def test_module_losses_reject_per_channel_mask():
    from cultionet_amd import losses as L

    dev = _dev()
    pred = torch.rand(2, 3, 8, 8, device=dev)
    targets = torch.randint(0, 3, (2, 8, 8), device=dev)
    with pytest.raises(NotImplementedError):
        L.TanimotoComplementLoss()(pred, targets, torch.ones(2, 3, 8, 8, dtype=torch.int64, device=dev))


# ---------------------------------------------------------------------------------------------------------------------
# optimizer: cn_grad_sumsq_f32, cn_adamw_step_f32
# ---------------------------------------------------------------------------------------------------------------------

def _store_numel_h32():
    """The trainer's flat parameter count at hidden 32 (ParamStore pads every parameter to 4 elements)."""
    from cultionet_amd.lightning import CultionetLitModel

    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=32, dropout=0.0)
    return lit.cultionet_model.mask_model.to(_dev()).param_store().numel


@pytest.mark.parametrize("n", [0, 1, 255, 2048 * 1024 + 1, "store_h32"])
def test_grad_sumsq(n):
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    dev = _dev()
    if n == "store_h32":
        n = _store_numel_h32()
        assert n > 2048 * 1024
    g = torch.Generator().manual_seed(1100)
    x = torch.randn(max(n, 1), generator=g) * 3.0
    xd = x.to(dev)
    out = torch.full((1,), 12345.0, dtype=torch.float64, device=dev)  # the call must zero it first
    _lib.call("cn_grad_sumsq_f32", xd.data_ptr(), n, out.data_ptr(), E._stream())
    torch.cuda.synchronize()
    ref = float((x[:n].double() ** 2).sum())
    if n == 0:
        assert out.item() == 0.0
    else:
        err = abs(out.item() - ref) / ref
        print(f"sumsq n={n}: rel err {err:.3e}")
        assert err <= 1e-12, (n, out.item(), ref)


def _adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, scale, max_norm):
    """torch.optim.AdamW (amsgrad=False, maximize=False; torch/optim/adamw.py single-tensor path) after
    torch.nn.utils.clip_grad_norm_(max_norm) of the gradient scaled by `scale` (DDP: the all-reduced sum / world)."""
    g = g * scale
    if max_norm is not None:
        g = g * min(1.0, max_norm / (float(g.norm()) + 1e-6))
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def _adamw_run(n, steps, sched, scale, max_norm, wd, gnorm, what, eps=1e-4, b2=0.98):
    """Run `steps` kernel steps; each is compared with _adamw_ref started from the kernel's own state (fp64 copies)."""
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    dev = _dev()
    gen = torch.Generator().manual_seed(1200 + n % 97)
    p = (torch.randn(n, generator=gen) * 0.02).to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
    worst = {"dp": 0.0, "m": 0.0, "v": 0.0}
    for step in range(1, steps + 1):
        lr, b1 = sched(step)
        g = torch.randn(n, generator=gen)
        g[torch.rand(n, generator=gen) < 0.1] = 0.0  # exact zeros
        g = g * (gnorm / float(g.norm()))
        p0, m0, v0 = p.cpu().double(), m.cpu().double(), v.cpu().double()
        gd = g.to(dev)
        if max_norm is not None:
            _lib.call("cn_grad_sumsq_f32", gd.data_ptr(), n, sumsq.data_ptr(), E._stream())
        _lib.call("cn_adamw_step_f32", p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, float(lr), float(b1),
                  b2, eps, wd, step, float(scale), sumsq.data_ptr() if max_norm is not None else None,
                  float(max_norm) if max_norm is not None else 0.0, E._stream())
        torch.cuda.synchronize()
        # the reference gets the fp32 values the kernel received
        f = lambda x: float(torch.tensor(x, dtype=torch.float32))
        pr, mr, vr = _adamw_ref(p0, g.double(), m0, v0, f(lr), f(b1), f(b2), f(eps), f(wd), step, f(scale), max_norm)
        dp = pr - p0
        # p is stored in fp32: its own rounding (and that of p * (1 - lr * wd)) is allowed on top of 1e-5 of max|dp|
        perr = ((p.cpu().double() - pr).abs() - 2 * F32_EPS * pr.abs()).clamp(min=0).max()
        for k, err, scale_ in (("dp", float(perr), float(dp.abs().max())),
                               ("m", float((m.cpu().double() - mr).abs().max()), float(mr.abs().max())),
                               ("v", float((v.cpu().double() - vr).abs().max()), float(vr.abs().max()))):
            r = err / (GRAD_REL * max(scale_, 1e-30))
            worst[k] = max(worst[k], r)
            assert r <= 1.0, f"{what} step {step} {k}: err {err:.3e} > {GRAD_REL:.0e} * {scale_:.3e}"
    print(f"{what}: worst ratio " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()))


N_OPT = 2048 * 1024 + 2053  # past cn_adamw_step_f32's 2048-block grid cap: the grid-stride loop iterates

ADAMW_CASES = {
    # id: (grad_scale, max_norm, weight_decay, norm of the (summed) gradient)
    "clip_active": (1.0, 1.0, 1e-3, 7.0),
    "clip_inactive": (1.0, 1.0, 0.0, 0.4),
    "no_clip": (1.0, None, 1e-3, 7.0),
    "ddp2_clip_active": (0.5, 1.0, 1e-3, 10.0),     # averaged norm 5: coefficient 0.2 (0.1 on the summed norm)
    "ddp8_clip_inactive": (0.125, 1.0, 0.0, 4.0),  # averaged norm 0.5: no clip (the summed norm 4 would clip)
}


@pytest.mark.parametrize("case", list(ADAMW_CASES), ids=list(ADAMW_CASES))
def test_adamw_regimes(case):
    scale, max_norm, wd, gnorm = ADAMW_CASES[case]
    _adamw_run(N_OPT, 3, lambda s: (0.01, 0.9), scale, max_norm, wd, gnorm, case)


def test_adamw_one_cycle_50_steps():
    """HipTrainer's schedule: (lr, beta1) of the project's OneCycleLR at every step, given to both sides."""
    from cultionet_amd.schedules import OneCycleLR

    sched = OneCycleLR(max_lr=0.01, total_steps=50)
    _adamw_run(300_007, 50, sched, 1.0, 1.0, 1e-3, 3.0, "one_cycle")
