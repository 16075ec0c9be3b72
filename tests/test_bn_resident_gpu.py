"""The single-launch ("resident") fp32 BatchNorm kernels of cn_norm.hip and the rule that chooses between them and the
two-pass kernels -- which keep the channels that do not fit a block, also behind one dy for all groups -- against the
float64 restatement of tests/test_norm_ref.py (bn_fwd64, bn_bwd64) through the C ABI. The single-tensor and the
grouped entry points run the same kernels, resident and two-pass: the cases reach both through either entry, and
test_bn_single_equals_grouped_g1 asks for identical bits from the two.

Every comparison is per element with the bound forms of tests/test_norm_gpu.py's docstring (c = 16, u = 2^-24, D = 0:
the sums are fp64), through that file's _bn_check. Each case names the number of launches it expects from
cn_launch_count -- one for the resident path, two for the two-pass one -- so a wrong rule fails here instead of hiding
behind the fallback. Outputs, statistics and the workspace are prefilled with NaN (a value left unwritten shows), and
the gaps of strided outputs must still hold NaN afterwards (a stray store shows).

Channel 0 of every input is the constant 0.75 (variance exactly 0: mean and rstd are compared bit for bit), channel 1
has mean 10^3 and unit spread.

The rule the expectations restate (bn_resident_plan): a channel goes resident when its B*L values fit a block shape --
16-byte units: 81 920 values forward (40 960 / 20 480 per group with 2 / 3 summed groups, which share a block; 4 never
do) and 40 960 backward (always one group per block); dword units a quarter of that -- and the launch has at least 128
blocks or its blocks hold at most 20 480 values (all summed groups counted).
"""
import ctypes
import math

import pytest
import torch

from test_norm_gpu import _bn_check, _bn_stat_allowance, _bn_y_bound, _dev, _randn, _s, _tab, _within
from test_norm_ref import bn_bwd64, bn_fwd64

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
NAN = float("nan")


def _buf(B, C, L, gaps=False, odd=False):
    """A [B, C, L] view of a NaN-filled flat buffer and the mask of the flat elements that belong to it. gaps: channel
    slice 1 .. C of a [B, C + 3, L] buffer (batch stride (C + 3) * L); odd: one float past a 16-byte boundary."""
    CC, lead = (C + 3, 1) if gaps else (C, 0)
    n, off = B * CC * L, 1 if odd else 0
    flat = torch.full((n + 4,), NAN, device=_dev())
    mask = torch.zeros(n + 4, dtype=torch.bool, device=_dev())
    mask[off:off + n].view(B, CC, L)[:, lead:lead + C] = True
    return flat[off:off + n].view(B, CC, L)[:, lead:lead + C], flat, mask


def _put(t, gaps, odd):
    v, flat, mask = _buf(*t.shape, gaps=gaps, odd=odd)
    v.copy_(t)
    return v, flat, mask


def _x(B, C, L, seed):
    x = _randn((B, C, L), seed, 1.5) + _randn((1, C, 1), seed + 1, 0.5)
    x[:, 0] = 0.75
    if C > 1:
        x[:, 1] = _randn((B, L), seed + 2) + 1000.0
    return x


def _launches():
    from cultionet_amd import _lib

    return _lib.query("cn_launch_count", 0)


def _case(G, B, C, L, *, summed=False, res=False, act=1, layout="dense", training=1, shared=None, acc=None, null=None,
          acc_params=1, single=False, fwd=1, bwd=1):
    return dict(G=G, B=B, C=C, L=L, summed=summed, res=res, act=act, layout=layout, training=training,
                shared=summed if shared is None else shared, acc=acc or (0,) * G, null=null, acc_params=acc_params,
                single=single, fwd=fwd, bwd=bwd)


CASES = {
    # shapes and alignment: 16-byte planes, dword planes (625, 169, 7 x 9), strided batches, an odd base pointer
    "g2_L64": _case(2, 3, 5, 64),
    "g2_L625": _case(2, 4, 5, 625),
    "g2_L169": _case(2, 8, 6, 169),
    "g2_L63": _case(2, 3, 4, 63),
    "g2_gaps": _case(2, 3, 5, 64, layout="gaps"),
    "g2_gaps_L63": _case(2, 3, 5, 63, layout="gaps"),
    "g2_odd": _case(2, 3, 5, 64, layout="odd"),
    "g2_partial_slot": _case(2, 3, 4, 700),  # 525 units on 512 threads: the second slot is partly filled
    "one_L64": _case(1, 3, 5, 64, single=True, res=True),
    "one_L625": _case(1, 4, 5, 625, single=True),
    "one_L169": _case(1, 8, 6, 169, single=True, res=True),
    "one_L63": _case(1, 3, 4, 63, single=True, act=0),
    "one_gaps": _case(1, 3, 5, 64, single=True, res=True, layout="gaps"),
    "one_odd": _case(1, 3, 5, 64, single=True, layout="odd"),
    "one_partial_slot": _case(1, 3, 4, 700, single=True, acc=(1,)),
    "one_c31_2048": _case(1, 8, 31, 256, single=True),  # fewer than 32 channels: tiny tensors are always resident
    # a block's capacity, and one 16-byte piece per plane above it (128 channels: enough blocks for the large planes)
    "fwd_cap": _case(1, 2, 128, 40960, fwd=1, bwd=2),
    "fwd_cap_plus": _case(1, 2, 128, 40964, fwd=2, bwd=2),
    "bwd_cap": _case(1, 2, 128, 20480, fwd=1, bwd=1),
    "bwd_cap_plus": _case(1, 2, 128, 20484, fwd=1, bwd=2),
    "one_bwd_cap": _case(1, 2, 128, 20480, single=True, fwd=1, bwd=1),
    "one_bwd_cap_plus": _case(1, 2, 128, 20484, single=True, fwd=1, bwd=2),
    "sum2_cap": _case(2, 2, 128, 20480, summed=True, res=True, fwd=1, bwd=1),  # backward: one group per block
    "sum2_cap_plus": _case(2, 2, 128, 20484, summed=True, res=True, fwd=2, bwd=2),
    "few_blocks_20000": _case(2, 8, 32, 2500),  # 64 blocks of 20 000 values: still resident
    "few_blocks_20800": _case(2, 8, 32, 2600, fwd=2, bwd=2),  # 64 blocks of 20 800 values: two wide launches
    "few_blocks_sum_20800": _case(2, 4, 32, 2600, summed=True, res=True, fwd=2, bwd=1),  # forward: 2 x 10 400 per block
    # grouped forward
    **{f"sep_G{G}_act{a}": _case(G, 3, 5, 64, act=a) for G in (1, 2, 3, 4) for a in (0, 1)},
    **{f"sum_G{G}_res{r}_act{a}": _case(G, 3, 5, 64, summed=True, res=bool(r), act=a)
       for G in (2, 3) for r in (0, 1) for a in (0, 1)},
    "sum_G1_res": _case(1, 3, 5, 64, summed=True, res=True),
    "sum_G2_L625": _case(2, 4, 5, 625, summed=True, res=True),
    "sum_G4": _case(4, 3, 5, 64, summed=True, res=True, fwd=2, bwd=1),  # four summed groups do not share a block
    # backward
    "bwd_sep_G3_mixed_acc": _case(3, 3, 5, 64, acc=(1, 0, 1)),
    "bwd_sep_G2_null": _case(2, 3, 5, 64, null=0, acc=(0, 1)),
    "bwd_shared_G3_mixed_null": _case(3, 3, 5, 64, summed=True, res=True, acc=(0, 1, 0), null=2),
    "bwd_shared_G2_acc": _case(2, 4, 5, 625, summed=True, acc=(1, 1)),
    "bwd_shared_sep_fwd": _case(2, 3, 5, 64, shared=True, acc=(0, 1)),  # one dy after a separate forward
    "bwd_sep_after_sum": _case(2, 3, 5, 64, summed=True, shared=False),
    "bwd_shared_G3_L625": _case(3, 4, 5, 625, summed=True, acc=(0, 0, 1)),
    "bwd_params_write": _case(2, 3, 5, 64, acc_params=0),
    "bwd_params_write_shared": _case(2, 3, 5, 64, summed=True, acc_params=0, null=1),
    "eval_G2": _case(2, 3, 5, 64, training=0, fwd=1, bwd=1),  # the eval forward is the apply kernel alone
    "eval_G2_shared": _case(2, 3, 5, 64, training=0, summed=True, res=True, fwd=1, bwd=1),
    "eval_one": _case(1, 3, 5, 64, training=0, single=True, fwd=1, bwd=1),
    # channels that fit no block, behind one dy for all groups: the two-pass kernels
    "twopass_shared_G2": _case(2, 8, 4, 10000, summed=True, res=True, fwd=2, bwd=2),
    "twopass_shared_G3_mixed": _case(3, 3, 4, 10000, summed=True, acc=(1, 0, 0), null=2, fwd=2, bwd=2),
    "twopass_shared_G4": _case(4, 3, 4, 10000, summed=True, res=True, acc=(0, 1, 0, 1), fwd=2, bwd=2),
    "twopass_shared_scalar": _case(2, 5, 4, 2501, summed=True, res=True, acc=(0, 1), fwd=2, bwd=2),
    "twopass_shared_params_write": _case(2, 3, 4, 10000, summed=True, acc_params=0, null=0, fwd=2, bwd=2),
    "twopass_shared_eval": _case(2, 3, 4, 10000, summed=True, training=0, fwd=1, bwd=2),
    "twopass_all_null": _case(2, 3, 4, 10000, null="all", fwd=2, bwd=2),  # no dx at all: one block per channel and group
    # the same two-pass kernels through the single entry points (4 blocks of 30 000 values; 12 505 and 22 509 dwords)
    "one_twopass": _case(1, 3, 4, 10000, single=True, res=True, fwd=2, bwd=2),
    # 12 505 dword values fit the forward's largest block shape (20 480), not the backward's (10 240)
    "one_twopass_scalar": _case(1, 5, 4, 2501, single=True, res=True, acc=(1,), fwd=1, bwd=2),
    "one_twopass_scalar_fwd": _case(1, 9, 4, 2501, single=True, res=True, acc=(1,), fwd=2, bwd=2),
    "one_twopass_gaps": _case(1, 3, 4, 10000, single=True, layout="gaps", fwd=2, bwd=2),
    "one_twopass_odd": _case(1, 3, 4, 10000, single=True, layout="odd", fwd=2, bwd=2),  # L % 4 == 0 on dwords
    "one_twopass_params_write": _case(1, 3, 4, 10000, single=True, null=0, acc_params=0, fwd=2, bwd=2),
    "one_twopass_eval": _case(1, 3, 4, 10000, single=True, training=0, fwd=1, bwd=2),
}


@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_bn_resident_vs_float64(name):
    from cultionet_amd import _lib

    k = CASES[name]
    G, B, C, L, act, training = k["G"], k["B"], k["C"], k["L"], k["act"], k["training"]
    summed, single = k["summed"], k["single"]
    gaps, odd = k["layout"] == "gaps", k["layout"] == "odd"
    dev = _dev()
    gen = torch.Generator().manual_seed(C * 1000 + L)
    xs = [_x(B, C, L, 10 + 7 * g) for g in range(G)]
    gammas = [(1 + 0.2 * torch.randn(C, generator=gen)).to(dev) for _ in range(G)]
    betas = [(0.2 * torch.randn(C, generator=gen)).to(dev) for _ in range(G)]
    olds = [((0.2 * torch.randn(C, generator=gen)).to(dev), (0.5 + torch.rand(C, generator=gen)).to(dev))
            for _ in range(G)]
    r = _randn((B, C, L), 90) if k["res"] else None
    dys = [_randn((B, C, L), 100)] * G if k["shared"] else [_randn((B, C, L), 100 + g) for g in range(G)]
    priors = [_randn((B, C, L), 200 + g) if k["acc"][g] else None for g in range(G)]
    pg = [_randn((C,), 300 + g) for g in range(G)]
    pb = [_randn((C,), 400 + g) for g in range(G)]

    # float64 references
    fwds, bwds, ress = [], [], []
    run = r.double() if r is not None else torch.zeros(B, C, L, dtype=torch.float64, device=dev)
    for g in range(G):
        f = bn_fwd64(xs[g], gammas[g], betas[g], olds[g][0], olds[g][1], training=bool(training), momentum=MOM, eps=EPS,
                     act=act, res=r if (single and r is not None) else None)
        fwds.append(f)
        bwds.append(bn_bwd64(f, gammas[g], dys[g], training=bool(training), act=act))
        ress.append(run)
        run = run + f["y"]
    y_sum = run

    # device buffers
    x_in = [_put(x, gaps, odd)[0] for x in xs]
    r_in = _put(r, gaps, odd)[0] if r is not None else None
    if k["shared"]:
        dy_in = [_put(dys[0], gaps, odd)[0]] * G
    else:
        dy_in = [_put(d, gaps, odd)[0] for d in dys]
    y_out = [_buf(B, C, L, gaps, odd) for _ in range(1 if summed else G)]
    dx_out = []
    for g in range(G):
        v, flat, mask = _buf(B, C, L, gaps, odd)
        if priors[g] is not None:
            v.copy_(priors[g])
        dx_out.append((v, flat, mask))
    means = [torch.full((C,), NAN, device=dev) for _ in range(G)]
    rstds = [torch.full((C,), NAN, device=dev) for _ in range(G)]
    rms = [o[0].clone() for o in olds]
    rvs = [o[1].clone() for o in olds]
    dgs = [p.clone() if k["acc_params"] else torch.full((C,), NAN, device=dev) for p in pg]
    dbs = [p.clone() if k["acc_params"] else torch.full((C,), NAN, device=dev) for p in pb]
    ws = torch.full((G * _lib.query("cn_bn_workspace_doubles", C),), NAN, dtype=torch.float64, device=dev)
    coef = torch.full((2 * C,), NAN, device=dev)
    xbs, ybs, dybs, dxbs = x_in[0].stride(0), y_out[0][0].stride(0), dy_in[0].stride(0), dx_out[0][0].stride(0)
    dx_ptr = [None if k["null"] in (g, "all") else dx_out[g][0].data_ptr() for g in range(G)]
    P = lambda ts: _tab([t.data_ptr() for t in ts])

    n0 = _launches()
    if single:
        _lib.call("cn_bn_act_fwd_f32", x_in[0].data_ptr(), xbs, gammas[0].data_ptr(), betas[0].data_ptr(),
                  rms[0].data_ptr(), rvs[0].data_ptr(), r_in.data_ptr() if r_in is not None else None,
                  r_in.stride(0) if r_in is not None else 0, y_out[0][0].data_ptr(), ybs, means[0].data_ptr(),
                  rstds[0].data_ptr(), ws.data_ptr(), B, C, L, training, MOM, EPS, act, _s())
    else:
        _lib.call("cn_bn_act_group_fwd_f32", G, P(x_in), xbs, P(gammas), P(betas), P(rms), P(rvs),
                  r_in.data_ptr() if r_in is not None else None, r_in.stride(0) if r_in is not None else 0,
                  _tab([y_out[0 if summed else g][0].data_ptr() for g in range(G)]), ybs, P(means), P(rstds),
                  ws.data_ptr(), B, C, L, training, MOM, EPS, act, 1 if summed else 0, _s())
    n1 = _launches()
    if single:
        _lib.call("cn_bn_act_bwd_f32", x_in[0].data_ptr(), xbs, dy_in[0].data_ptr(), dybs, means[0].data_ptr(),
                  rstds[0].data_ptr(), gammas[0].data_ptr(), betas[0].data_ptr(), dx_ptr[0], dxbs, dgs[0].data_ptr(),
                  dbs[0].data_ptr(), coef.data_ptr(), ws.data_ptr(), B, C, L, training, act, k["acc"][0],
                  k["acc_params"], _s())
    else:
        _lib.call("cn_bn_act_group_bwd_f32", G, P(x_in), xbs, P(dy_in), dybs, P(means), P(rstds), P(gammas), P(betas),
                  _tab(dx_ptr), dxbs, (ctypes.c_int * G)(*k["acc"]), P(dgs), P(dbs), ws.data_ptr(), B, C, L, training,
                  act, k["acc_params"], _s())
    n2 = _launches()
    torch.cuda.synchronize()
    print(f"{name}: forward {n1 - n0} launch(es), backward {n2 - n1}")
    assert n1 - n0 == k["fwd"], f"{name}: forward took {n1 - n0} launches, the rule says {k['fwd']}"
    assert n2 - n1 == k["bwd"], f"{name}: backward took {n2 - n1} launches, the rule says {k['bwd']}"

    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    rstd0 = torch.tensor(1.0 / math.sqrt(eps32), dtype=torch.float64).float().item()
    for g in range(G):
        got = dict(mean=means[g], rstd=rstds[g], dgamma=dgs[g], dbeta=dbs[g])
        if training:
            got.update(running_mean=rms[g], running_var=rvs[g])
            assert means[g][0].item() == 0.75 and rstds[g][0].item() == rstd0, \
                f"{name} layer {g}: a constant channel has variance exactly 0 ({means[g][0].item()!r}, {rstds[g][0].item()!r})"
        else:
            assert torch.equal(rms[g], olds[g][0]) and torch.equal(rvs[g], olds[g][1])
        if not summed:
            got["y"] = y_out[g][0]
        ref = dict(bwds[g])
        if k["null"] in (g, "all"):
            assert torch.isnan(dx_out[g][1]).all(), f"{name} layer {g}: no dx buffer was passed"
        else:
            got["dx"] = dx_out[g][0]
            if priors[g] is not None:
                ref["dx"] = ref["dx"] + priors[g].double()
            assert torch.isnan(dx_out[g][1][~dx_out[g][2]]).all(), f"{name} layer {g}: a store outside dx"
        if k["acc_params"]:
            ref["dgamma"], ref["dbeta"] = ref["dgamma"] + pg[g].double(), ref["dbeta"] + pb[g].double()
        _bn_check(f"{name} layer{g}", fwds[g], ref, xs[g], gammas[g], betas[g], r if (single and r is not None) else None,
                  dys[g], act=act, training=bool(training), momentum=MOM, got=got, old=olds[g], dx_prior=priors[g])
    for v, flat, mask in y_out:
        assert torch.isnan(flat[~mask]).all(), f"{name}: a store outside y"
    if summed:  # bound of the sum: the per-layer bounds added up (each layer adds its rounding to the running sum)
        bound = 0.0
        for g in range(G):
            dm, _, rrel = _bn_stat_allowance(fwds[g], bool(training), 0)
            bound = bound + _bn_y_bound(fwds[g], xs[g].double(), gammas[g], betas[g], ress[g], dm, rrel)
        _within(y_out[0][0], y_sum, bound, f"{name} sum")


@pytest.mark.parametrize("training", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("B,C,L", [(3, 4, 10000), (5, 4, 2501)])
def test_bn_single_equals_grouped_g1(B, C, L, res, training):
    """One body: cn_bn_act_{fwd,bwd}_f32 and cn_bn_act_group_{fwd,bwd}_f32 with G = 1 (sum_outputs = 1 where there is a
    residual) give bit-identical y, mean, rstd, running statistics, dx, dgamma and dbeta on the same inputs. At both
    shapes the two entries cut a channel into the same number of partial rows (20 and 5: both capped by
    (L + 511) / 512), so equal kernels see equal arguments. Outputs start as NaN: torch.equal fails on a value left
    unwritten."""
    from cultionet_amd import _lib

    dev = _dev()
    gen = torch.Generator().manual_seed(C * 1000 + L)
    x = _x(B, C, L, 10)
    gamma = (1 + 0.2 * torch.randn(C, generator=gen)).to(dev)
    beta = (0.2 * torch.randn(C, generator=gen)).to(dev)
    old_m, old_v = (0.2 * torch.randn(C, generator=gen)).to(dev), (0.5 + torch.rand(C, generator=gen)).to(dev)
    r = _randn((B, C, L), 90) if res else None
    dy = _randn((B, C, L), 100)
    rp, rbs = (r.data_ptr(), r.stride(0)) if res else (None, 0)
    nan = lambda *shape: torch.full(shape, NAN, device=dev)

    def run(single):
        o = dict(y=nan(B, C, L), mean=nan(C), rstd=nan(C), running_mean=old_m.clone(), running_var=old_v.clone(),
                 dx=nan(B, C, L), dgamma=nan(C), dbeta=nan(C))
        ws = torch.full((_lib.query("cn_bn_workspace_doubles", C),), NAN, dtype=torch.float64, device=dev)
        bs = x.stride(0)
        if single:
            _lib.call("cn_bn_act_fwd_f32", x.data_ptr(), bs, gamma.data_ptr(), beta.data_ptr(),
                      o["running_mean"].data_ptr(), o["running_var"].data_ptr(), rp, rbs, o["y"].data_ptr(), bs,
                      o["mean"].data_ptr(), o["rstd"].data_ptr(), ws.data_ptr(), B, C, L, training, MOM, EPS, 1, _s())
            _lib.call("cn_bn_act_bwd_f32", x.data_ptr(), bs, dy.data_ptr(), bs, o["mean"].data_ptr(),
                      o["rstd"].data_ptr(), gamma.data_ptr(), beta.data_ptr(), o["dx"].data_ptr(), bs,
                      o["dgamma"].data_ptr(), o["dbeta"].data_ptr(), None, ws.data_ptr(), B, C, L, training, 1, 0, 0,
                      _s())
        else:
            P = lambda t: _tab([t.data_ptr()])
            _lib.call("cn_bn_act_group_fwd_f32", 1, P(x), bs, P(gamma), P(beta), P(o["running_mean"]),
                      P(o["running_var"]), rp, rbs, P(o["y"]), bs, P(o["mean"]), P(o["rstd"]), ws.data_ptr(), B, C, L,
                      training, MOM, EPS, 1, 1 if res else 0, _s())
            _lib.call("cn_bn_act_group_bwd_f32", 1, P(x), bs, P(dy), bs, P(o["mean"]), P(o["rstd"]), P(gamma), P(beta),
                      P(o["dx"]), bs, (ctypes.c_int * 1)(0), P(o["dgamma"]), P(o["dbeta"]), ws.data_ptr(), B, C, L,
                      training, 1, 0, _s())
        torch.cuda.synchronize()
        return o

    one, grouped = run(True), run(False)
    for key in one:
        assert torch.equal(one[key], grouped[key]), f"{key}: the single and the grouped entry differ"
