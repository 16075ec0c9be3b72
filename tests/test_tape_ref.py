"""Pins tests/tape_ref.py on the CPU, so that the exact GPU tests of the tape (tests/test_tape_exact_gpu.py) and of the
glue kernels (tests/test_glue_kernels_exact_gpu.py) can fail:

* every use of every Var in every graph carries weight: with that one use detached some input gradient of the float64
  reference changes, or, where the use belongs to an input that needs no gradient or feeds only a convolution's
  weight gradient, some weight gradient, which the GPU test compares as well (uses that only reach an output without
  dy change nothing, and that is asserted too); so an engine that drops a contribution, or overwrites where it has to accumulate, cannot equal the reference;
* every graph keeps the integer-within-256 premise under which bf16 and fp32 are both exact;
* every graph still has the structure its name claims;
* the bound of cn_channel_sum_bf16 holds for a sequential fp32 restatement of the kernel's order of sums and fails
  for a sum that drops the last row.
"""
import pytest
import torch

import tape_ref as R
from conv_exact_worker import BF

IDS = [c.name for c in R.CASES]


def _all_grads(r):
    return {**{"d" + k: v for k, v in r.grads.items()}, **{"dw:" + k: v for k, v in r.wgrads.items()}}


def _differs(a, b):
    if a is None or b is None:
        return (a is None) != (b is None)
    return not torch.equal(a, b)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_premise(case):
    worst = R.premise256(case)
    assert worst >= 2  # not a graph of zeros


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_use_carries_weight(case):
    full = R.run_ref(case)
    g0 = _all_grads(full)
    live = R.live_steps(case)
    edges = R.uses(case)
    assert edges
    for sid, j, name in edges:
        cut = R.run_ref(case, full.xs, full.ws, full.dys, cut=(sid, j))
        for k in case.outs:  # detaching changes no forward value
            assert torch.equal(cut.outs[k], full.outs[k])
        g1 = _all_grads(cut)
        changed = [k for k in g0 if _differs(g0[k], g1[k])]
        if sid in live and _reaches_grad(case, name):
            assert changed, f"{case}: detaching input {j} ({name}) of step {sid} changes no gradient"
        else:
            assert not changed, f"{case}: step {sid} reaches no dy, but detaching its input {name} changed {changed}"


def _reaches_grad(case, name):
    """Does Var `name` depend on an input that requires a gradient, or on a weight?"""
    res = R._canon(case)
    needs = {k for k, (_, req) in case.inputs.items() if req}
    for _, (op, ins, out, kw) in sorted(R.walk(case.steps), key=lambda e: e[0]):
        if op in ("spawn", "sync", "buffer"):
            continue
        outs = out if isinstance(out, tuple) else (out,)
        if op == "conv" or any(res(n) in needs for n in ins):
            needs.update(res(o) for o in outs)
    return res(name) in needs


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_structure_claims(case):
    r = R.run_ref(case)
    for claim in case.claims:
        kind = claim[0]
        if kind == "consumers":
            _, name, kinds = claim
            assert tuple(R.consumers_of(case, name)) == tuple(kinds), (case, name, R.consumers_of(case, name))
        elif kind == "sliced":
            _, name, nslices, nused = claim
            (split,) = [st for _, st in R.walk(case.steps) if st[0] == "split" and st[1] == (name,)]
            assert len(split[2]) == nslices
            used = [s for s in split[2] if R.consumers_of(case, s)]
            assert len(used) == nused, (case, used)
            if 0 < nused < nslices and r.grads.get(name) is not None:  # the unused slice's part of the gradient is 0
                c0 = 0
                for s, c in zip(split[2], split[3]["sizes"]):
                    if s not in used:
                        assert not bool(r.grads[name][:, c0:c0 + c].any())
                    else:
                        assert bool(r.grads[name][:, c0:c0 + c].any())
                    c0 += c
        elif kind == "no-grad":
            assert r.grads[claim[1]] is None
        elif kind == "order":
            _, name, op, where = claim
            ids = sorted(R.walk(case.steps), key=lambda e: e[0])
            split_at = [sid for sid, st in ids if st[0] == "split" and st[1] == (name,)][0]
            slices = [st for _, st in ids if st[0] == "split" and st[1] == (name,)][0][2]
            direct = [sid for sid, st in ids if st[0] not in R.NO_USE and name in st[1]]
            sliced = [sid for sid, st in ids if st[0] not in R.NO_USE and set(st[1]) & set(slices)]
            assert direct and sliced
            if where == "before":
                assert max(direct) < split_at < min(sliced)
            else:
                assert max(sliced) < min(direct)
            assert op in R.consumers_of(case, name)
        elif kind == "branch":
            _, name, nops = claim
            (sp,) = [st for _, st in R.walk(case.steps) if st[0] == "spawn" and st[2] == name]
            assert len(sp[3]["steps"]) == nops
            main = [k for k in R.consumers_of(case, sp[1][0])]
            assert len(main) >= 2  # the branch's input is read by the main stream too
        else:
            raise AssertionError(claim)


def test_case_list_covers_the_patterns():
    names = set(IDS)
    kinds = ("cat", "add", "addb", "join", "conv1", "conv3", "pool", "flip")
    for k in kinds:
        assert f"fanout1-{k}" in names
    for a in R.PLUMBING:  # both orders of every (give_grad consumer, grad_buffer consumer) pair
        for b in R.KERNELS:
            assert f"fanout2-{a}-{b}" in names and f"fanout2-{b}-{a}" in names
    assert sum(n.startswith("fanout3-") for n in names) == 18
    assert {c.B for c in R.CASES} == {1, 3} and {(c.H, c.W) for c in R.CASES} == {(5, 7), (9, 9)}
    for c in R.CASES:
        assert all(ch % 8 == 0 for ch, _ in c.inputs.values())
        assert all(co % 8 == 0 and ci % 8 == 0 and k in (1, 3) for co, ci, k in c.weights.values())


def test_integers_are_bf16_exact():
    v = torch.arange(-256, 257, dtype=torch.float64)
    assert torch.equal(v.float().to(BF).double(), v)
    assert float(torch.tensor(257.0).to(BF)) != 257.0


# ---------------------------------------------------------------------------------------------------------------------
# cn_channel_sum_bf16: the bound holds for the kernel's order of sums and fails for a dropped row
# ---------------------------------------------------------------------------------------------------------------------

def _bf16_data(P, C, seed):
    """The data of test_channel_sum_bf16_bounded."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((P, C), generator=g) * 3.0 + 0.5).to(BF).float()


CS_SHAPES = [(C, P) for C in (8, 24, 128, 2048) for P in R.channel_sum_rows(C)]  # the shapes of the GPU test


@pytest.mark.parametrize("C,P", CS_SHAPES)
def test_channel_sum_bound_holds_for_the_kernels_order(C, P):
    x = _bf16_data(P, C, C + P)
    ref = x.double().sum(0)
    bound = R.channel_sum_bound(x, P, C)
    err = (R.channel_sum_emulated(x).double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"channel sum C={C} P={P} D={R.channel_sum_depth(P, C)}: emulated err/bound {ratio:.3f}")
    assert bool((err <= bound).all())
    if P > 1:
        bad = (R.channel_sum_emulated(x, drop_last_row=True).double() - ref).abs()
        assert bool((bad > bound).any()), "a sum without the last row passes the bound"
    # accumulating (the old values of test_channel_sum_bf16_bounded): one more fp32 add
    old = torch.randn((C,), generator=torch.Generator().manual_seed(C + P + 1)) * 50.0
    got = (old + R.channel_sum_emulated(x)).double()
    bound = R.channel_sum_bound(x, P, C, old)
    err = (got - (ref + old.double())).abs()
    print(f"channel sum C={C} P={P} accumulate: emulated err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    if P > 1:
        bad = ((old + R.channel_sum_emulated(x, drop_last_row=True)).double() - (ref + old.double())).abs()
        assert bool((bad > bound).any()), "an accumulated sum without the last row passes the bound"


def test_channel_sum_emulation_is_exact_on_integers():
    for C, P in CS_SHAPES:
        g = torch.Generator().manual_seed(P)
        x = torch.randint(-3, 4, (P, C), generator=g).float()
        assert torch.equal(R.channel_sum_emulated(x).double(), x.double().sum(0))


def test_bbn_grid_matches_norm_depth():
    import test_norm_gpu as N

    for C, P in CS_SHAPES:
        assert R.channel_sum_depth(P, C) == N.bbn_depth(P, C) + 1
