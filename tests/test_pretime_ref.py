"""CPU tests of tests/pretime_ref.py, the float64 restatement and error bounds the GPU tests of the fused
PreTimeReduction kernels are held to (tests/test_pretime_exact_gpu.py):

* the restatement agrees with oracle.towerunet_oracle.PreTimeReduction run in float64, to float64 roundoff (forward,
  autograd gradients, running statistics; train and eval; odd Tp in both branches; T = 5 where the k = 5 branch has Tp = 1);
* an fp32 evaluation of the same chain -- the oracle module in fp32, its batch statistics re-summed from the fp32
  convolution outputs in fp32 chunks of the claimed depth D and E[x^2] - m^2 form -- stays inside every bound at every
  configuration the GPU file uses (each check prints its worst err/bound);
* every mutation of pretime_ref.MUTATIONS leaves the bound of at least one output at every configuration it applies
  to, with the exceptions listed (and explained) in NOT_SEPARATED."""
import pytest
import torch

import pretime_ref as R


def _configs():
    """id -> dict(B, C, T, HW, Cout, kind, training, backward, accumulate): every configuration of the GPU file."""
    out = {}

    def add(tag, name, case, **kw):
        B, C, T, HW, Cout, kind = case
        out[f"{tag}-{name}"] = dict(dict(B=B, C=C, T=T, HW=HW, Cout=Cout, kind=kind, training=True, backward=True,
                                         accumulate=False), **kw)

    for name, case in R.dispatch_cases().items():
        add("dispatch", name, case, backward=not name.startswith(R.NO_BACKWARD))
    for name, case in R.WIDE_CASES.items():
        add("wide-train", name, case, backward=False)
        add("wide-infer", name, case, backward=False, training=False)
    for name, case in R.EVAL_CASES.items():
        add("eval", name, case, training=False)
    for name, case in R.ACCUM_CASES.items():
        add("accum", name, case, accumulate=True)
    for cube, (C, T) in R.EDGE_CUBES.items():
        for P, (B, HW) in R.EDGE_PIXELS.items():
            add("edge", f"{cube}-p{P}", (B, C, T, HW, 8, 0))
    for name, (B, C, T, HW, Cout, kind, train) in R.TILE_CASES.items():
        add("tiles", name, (B, C, T, HW, Cout, kind), training=train, backward=train)
    add("offsets", "c3t12", R.OFFSET_CASE, backward=False)
    return out


CONFIGS = _configs()
SMALL = [k for k in CONFIGS if not k.startswith("tiles")]


def _problem(cfg):
    return R.problem(cfg["B"], cfg["C"], cfg["T"], cfg["HW"], cfg["Cout"], cfg["kind"], cfg["training"], cfg["backward"],
                     cfg["accumulate"])


# ---------------------------------------------------------------------------------------------------------------------
# the restatement is the oracle module
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,C,T,HW,Cout", [(2, 3, 7, 13, 8), (2, 4, 5, 11, 24), (1, 3, 12, 9, 40), (3, 8, 5, 5, 16)])
def test_restatement_agrees_with_the_oracle_in_float64(B, C, T, HW, Cout, training):
    x, prm, dy, g0 = R.make_problem(B, C, T, HW, Cout, seed=3)
    ref = R.reference(x, prm, dy, training=training)
    mod = R.to_oracle(prm, C, T).train(training)
    y = mod(x.double().view(B, C, T, 1, HW))
    y.backward(dy.double().view(B, Cout, 1, HW))
    got = R.oracle_tensors(mod)
    got["y"] = y.detach().view(B, Cout, HW)
    for name in ["y"] + R.RUN_NAMES + R.GRAD_NAMES:
        a, b = ref[name][0], got[name].reshape(ref[name][0].shape)
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 1e-11 * max(scale, 1.0), name
    if training:  # the saved statistics against their definition
        for k, conv in zip(R.BR, (mod.conv3, mod.conv5)):
            h = conv.seq[0](x.double().view(B, C, T, 1, HW))
            m, var = h.mean((0, 2, 3, 4)), h.var((0, 2, 3, 4), unbiased=False)
            assert torch.allclose(ref[f"mean3_{k}"][0], m, rtol=1e-12, atol=1e-13)
            assert torch.allclose(ref[f"rstd3_{k}"][0], (var + R.BN_EPS).rsqrt(), rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# an fp32 evaluation stays inside the bounds
# ---------------------------------------------------------------------------------------------------------------------

def _chunked_stats(h, D, eps):
    """mean and rstd per channel of an fp32 [B, ch, ...] tensor: fp32 sums of x and x^2 in serial chunks of D, the
    chunk totals in float64, variance as E[x^2] - m^2 -- the summation the kernels' D stands for."""
    v = h.detach().transpose(0, 1).reshape(h.shape[1], -1).float()
    n = v.shape[1]
    pad = (-n) % D
    v = torch.cat([v, v.new_zeros(v.shape[0], pad)], 1).view(v.shape[0], -1, D)
    s, q = torch.zeros_like(v[..., 0]), torch.zeros_like(v[..., 0])
    for i in range(D):
        s = s + v[..., i]
        q = q + v[..., i] * v[..., i]
    m = s.double().sum(1) / n
    var = (q.double().sum(1) / n - m * m).clamp_min(0)
    return m, 1.0 / (var + eps).sqrt()


def fp32_evaluation(cfg):
    B, C, T, HW, Cout = cfg["B"], cfg["C"], cfg["T"], cfg["HW"], cfg["Cout"]
    x, prm, dy, g0, _ = _problem(cfg)
    mod = R.to_oracle(prm, C, T, torch.float32).train(cfg["training"])
    seen = {}
    hooks = []
    for k, conv in zip(R.BR, (mod.conv3, mod.conv5)):
        for idx, tag in ((1, "3"), (5, "2")):
            hooks.append(conv.seq[idx].register_forward_pre_hook(
                lambda m_, inp, key=(tag, k): seen.__setitem__(key, inp[0])))
    if g0 is not None:
        named = {}
        for k, conv in zip(R.BR, (mod.conv3, mod.conv5)):
            s = conv.seq
            named.update({f"dwa_{k}": s[0].weight, f"dwb_{k}": s[3].weight, f"dg3_{k}": s[1].weight, f"db3_{k}": s[1].bias,
                          f"dg2_{k}": s[5].weight, f"db2_{k}": s[5].bias})
        named["dgL"], named["dbL"] = mod.layer_norm[1].weight, mod.layer_norm[1].bias
        for n, t in named.items():
            t.grad = g0[n].clone().reshape(t.shape)
    y = mod(x.view(B, C, T, 1, HW))
    if cfg["backward"]:
        y.backward(dy.view(B, Cout, 1, HW))
    for h in hooks:
        h.remove()
    got = R.oracle_tensors(mod)
    y = y.detach().view(B, Cout, HW)
    got["y"] = y.to(torch.bfloat16).float() if cfg["kind"] == 1 else y
    if cfg["training"]:
        for k in R.BR:
            D = R.depths(B * HW, C, T, Cout, k)
            got[f"mean3_{k}"], got[f"rstd3_{k}"] = _chunked_stats(seen[("3", k)], D["bn3"], R.BN_EPS)
            got[f"mean2_{k}"], got[f"rstd2_{k}"] = _chunked_stats(seen[("2", k)], D["bn2"], R.BN_EPS)
    return got


def _names(cfg):
    names = ["y"] + R.RUN_NAMES
    if cfg["training"]:
        names += R.STAT_NAMES
    if cfg["backward"]:
        names += R.GRAD_NAMES
    return names


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_fp32_evaluation_stays_inside_every_bound(cid):
    cfg = CONFIGS[cid]
    ref = _problem(cfg)[4]
    got = fp32_evaluation(cfg)
    record = {}
    for name in _names(cfg):
        R.within(got[name], ref[name], f"{cid} {name}", record, R.group_of(name, cfg["kind"]))
    print("fp32 worst per group:", cid, {k: round(v, 4) for k, v in record.items()})


# ---------------------------------------------------------------------------------------------------------------------
# mutations leave the bounds
# ---------------------------------------------------------------------------------------------------------------------

def _applies(mut, cfg):
    train, back = cfg["training"], cfg["backward"]
    return {"tap5": True, "odd_tail": cfg["T"] % 2 == 1, "biased": train, "eps_outside": True,
            "c_swap": train and back, "dsilu_sigmoid": back, "ln_cp": cfg["Cout"] % 32 != 0, "swap_wb": True,
            "overwrite": back and cfg["accumulate"], "eval_keeps_means": back and not train}[mut]


# (mutation, configuration prefix) pairs the bound cannot separate, each with its reason.
NOT_SEPARATED = {
    # Biased instead of unbiased running variance changes rv by mom var / (cnt - 1). At P = 129 033 and 65 547 the
    # BatchNorm3d count is P Tp > 10^5 .. 10^6: 1 / cnt is at or below the c u = 9.5e-7 the momentum blend is allowed. For
    # BatchNorm2d (cnt = P, 1 / P ~ 1e-5) the variance itself is only known to dv / var ~ 3e-5: the E[r^2] - m^2 term
    # 3 D u (m^2 + var) plus the rounding of the C Tp-term convolution behind every r. The factor is separated at
    # every small configuration, where 1 / cnt is 1e-4 .. 0.5.
    ("biased", "tiles-reg-c3t12"), ("biased", "tiles-gen-c5t6"),
}


@pytest.mark.parametrize("cid", list(CONFIGS))
def test_mutations_leave_the_bounds(cid):
    cfg = CONFIGS[cid]
    x, prm, dy, g0, ref = _problem(cfg)
    names = _names(cfg)
    failed = []
    for mut in R.MUTATIONS:
        if not _applies(mut, cfg):
            continue
        bad = R.reference(x, prm, dy if cfg["backward"] else None, training=cfg["training"], mut=mut, grads0=g0,
                          bf16=cfg["kind"] == 1)
        ratios = {n: R.worst_ratio(bad[n][0], ref[n][0], ref[n][1], n)[0] for n in names}
        top = max(ratios, key=ratios.get)
        print(f"{cid} {mut}: leaves the bound of {sum(v > 1 for v in ratios.values())} outputs, worst {top} "
              f"{ratios[top]:.3g}")
        if not ratios[top] > 1.0 and (mut, cid) not in NOT_SEPARATED:
            failed.append((mut, top, ratios[top]))
    assert not failed, failed
