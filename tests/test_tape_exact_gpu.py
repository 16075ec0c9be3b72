"""The tape's gradient plumbing (cultionet_amd/tape.py: grad_buffer, give_grad, channel-slice parents, spawn / join
aliases) and the plumbing ops of the engine (cat_channels, split_channels, join_channels, add, to_bf16, to_f32) held
EXACTLY against float64 autograd.

The graphs are the data of tests/tape_ref.py: every fan-out order of give_grad and grad_buffer consumers, slices
(used, unused, twice, reordered, beside a direct read of their parent), cat into fresh and preallocated buffers, every
branch of add's backward, chains of precision converters with fan-out on both sides, outputs without dy, and spawned
branches. Inputs, weights and upstream gradients are small integers; tests/test_tape_ref.py asserts on the CPU that
every value and every accumulated gradient of every graph stays an integer within +-256, where fp32 AND bf16 are exact,
and that removing any single use changes a gradient. So every output, every input gradient and every weight gradient
must EQUAL the float64 reference in both precisions: an aliased buffer that is written twice, an overwrite in place of
an accumulate, a missing zero-fill or a contribution left out each change at least one integer.

A bf16 run enters through to_bf16 and leaves through to_f32 (rounding integers to bf16 is the identity).
"""
import pytest
import torch
import torch.nn as nn

import tape_ref as R
from conv_exact_worker import assert_exact, dev

pytestmark = pytest.mark.gpu

IDS = [c.name for c in R.CASES]
_REF = {}


def ref_of(case):
    """The float64 reference of a case, computed once and shared (never modified)."""
    if case.name not in _REF:
        r = R.run_ref(case)
        R.premise256(case, r)
        _REF[case.name] = r
    return _REF[case.name]


def _module(case, r, d, trainable=True):
    m = nn.ModuleDict({k: nn.Conv2d(ci, co, ks, padding=ks // 2, bias=False) for k, (co, ci, ks) in case.weights.items()})
    if not case.weights:
        m["unused"] = nn.Linear(1, 1)
    with torch.no_grad():
        for k in case.weights:
            m[k].weight.copy_(r.ws[k].float())
    for p in m.parameters():
        p.requires_grad_(trainable)
    return m.to(d)


class EngineRun:
    pass


def run_engine(case, bf16, enabled=True, req=True, trainable=True):
    """The graph in engine ops under ParamStore / using_store / recording; backward with the reference's dys."""
    from cultionet_amd import engine as E

    d = dev()
    r = ref_of(case)
    mod = _module(case, r, d, trainable)
    store = E.ParamStore(mod)
    store.zero_grad()
    out = EngineRun()
    with E.using_store(store), E.recording(enabled) as tape:
        entry = {k: E.Var(v.float().to(d).contiguous(), case.inputs[k][1] and req) for k, v in r.xs.items()}
        env = {k: (E.to_bf16(v) if bf16 else v) for k, v in entry.items()}
        bufs, branches = {}, {}

        def run(steps):
            for op, ins, o, kw in steps:
                a = [env[n] for n in ins] if op not in ("buffer", "sync") else None
                if op == "conv":
                    ks = case.weights[kw["w"]][2]
                    dst = None
                    if "out" in kw:
                        b, c0 = kw["out"]
                        dst = bufs[b][:, c0:c0 + case.weights[kw["w"]][0]]
                    env[o] = E.conv2d(a[0], mod[kw["w"]], 1, ks // 2, 1, out=dst)
                elif op == "pool":
                    env[o] = E.adaptive_max_pool2d(a[0], kw["size"])
                elif op == "cat":
                    env[o] = E.cat_channels(a, buf=bufs[kw["buf"]] if kw.get("buf") else None)
                elif op == "join":
                    env[o] = E.join_channels(a, bufs[kw["buf"]])
                elif op == "add":
                    env[o] = E.add(a[0], a[1])
                elif op == "flip":
                    env[o] = E.to_f32(a[0]) if E.is16(a[0].t) else E.to_bf16(a[0])
                    assert env[o] is not a[0]
                elif op == "split":
                    for name, v in zip(o, E.split_channels(a[0], kw["sizes"])):
                        env[name] = v
                elif op == "buffer":
                    bufs[o] = E.new_buffer((case.B, kw["C"], case.H, case.W), env[kw["like"]].t)
                elif op == "spawn":
                    def body(*aliases, kw=kw):
                        for n, v in zip(kw["args"], aliases):
                            env[n] = v
                        run(kw["steps"])
                        return env[kw["result"]]

                    branches[o], env[o] = E.spawn(body, a, 0)
                elif op == "sync":
                    E.join([branches[ins[0]]])
                else:
                    raise ValueError(op)

        run(case.steps)
        out.branched = any(b is not None for b in branches.values())
        exits = {k: E.to_f32(env[k]) for k in case.outs}
        out.nodes_recorded = len(tape.nodes)
        for k, dy in r.dys.items():
            if exits[k].req:
                exits[k].grad = dy.float().to(d).contiguous()
        tape.backward()
        out.nodes_left = list(tape.nodes)
    torch.cuda.synchronize()
    out.outs = {k: v.t.cpu() for k, v in exits.items()}
    out.grads = {k: (v.grad.cpu() if v.grad is not None else None) for k, v in entry.items()}
    out.wgrads = {k: store.grad_of(mod[k].weight).cpu() for k in case.weights}
    return out


def compare(case, got, r, what):
    for k in case.outs:
        assert_exact(got.outs[k], r.outs[k], f"{what} output {k}")
    for k in case.inputs:
        if r.grads[k] is None:
            assert got.grads[k] is None, f"{what}: input {k} has a gradient, the reference has none"
        else:
            assert got.grads[k] is not None, f"{what}: input {k} has no gradient"
            assert_exact(got.grads[k], r.grads[k], f"{what} d{k}")
    for k in case.weights:
        assert_exact(got.wgrads[k], r.wgrads[k], f"{what} dw {k}")
    assert got.nodes_left == [], f"{what}: tape nodes left after backward"


def _keepalive_empty():
    from cultionet_amd import engine as E

    ka = E._keepalive()
    assert ka.depth == 0 and not ka.keep and not getattr(E._state, "alloc_sinks", None)
    assert not getattr(E._state, "open_branches", [])


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_graph_equals_float64(case, bf16):
    got = run_engine(case, bf16)
    assert got.nodes_recorded > 0
    compare(case, got, ref_of(case), f"{case} {'bf16' if bf16 else 'f32'}")
    _keepalive_empty()


SPAWN = [c for c in R.CASES if c.name.startswith("spawn-")]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", SPAWN, ids=[c.name for c in SPAWN])
def test_branch_streams_on_and_off(case, bf16):
    """The same graph with the branch on the auxiliary stream and inline: equal to each other and to float64, and
    nothing is left in the keep-alive."""
    from cultionet_amd import engine as E

    r = ref_of(case)
    with E.branch_streams(True):
        on = run_engine(case, bf16)
    _keepalive_empty()
    with E.branch_streams(False):
        off = run_engine(case, bf16)
    _keepalive_empty()
    assert on.branched and not off.branched
    compare(case, on, r, f"{case} streams on")
    compare(case, off, r, f"{case} streams off")
    for k in case.outs:
        assert torch.equal(on.outs[k], off.outs[k])
    for k in case.inputs:
        assert torch.equal(on.grads[k], off.grads[k])
    for k in case.weights:
        assert torch.equal(on.wgrads[k], off.wgrads[k])


QUIET = [R.BY_NAME[n] for n in ("fanout3-cat-conv3-flip", "fanout3-join-add-pool", "slice-used-twice", "cat-buf-mixed",
                                "add-b-present", "precision-chain-others-after", "spawn-branch")]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("how", ["tape-off", "nothing-requires"])
@pytest.mark.parametrize("case", QUIET, ids=[c.name for c in QUIET])
def test_no_gradients_wanted(case, how, bf16):
    """recording(False), and a recording tape on which neither an input nor a parameter needs a gradient: no tape node,
    every gradient stays None (the weight gradients zero), outputs as with gradients. The one exception: spawn() and
    join() file their fork and join on a recording tape before they can know whether the branch's result will need a
    gradient, so a spawned branch leaves those two nodes, which do no gradient work."""
    r = ref_of(case)
    got = run_engine(case, bf16, enabled=how != "tape-off", req=how == "tape-off", trainable=how == "tape-off")
    # (a branch on a recording tape files its fork and join, which hold no gradient work)
    assert got.nodes_recorded == (2 if got.branched and how != "tape-off" else 0) and got.nodes_left == []
    for k in case.outs:
        assert_exact(got.outs[k], r.outs[k], f"{case} {how} output {k}")
    assert all(g is None for g in got.grads.values())
    for k in case.weights:
        assert not bool(got.wgrads[k].any())
    _keepalive_empty()


def test_frozen_weights_still_pass_gradients_on():
    """Frozen parameters, inputs that need gradients: input gradients as before, weight gradients stay zero."""
    case = R.BY_NAME["fanout3-cat-conv3-flip"]
    r = ref_of(case)
    for bf16 in (False, True):
        got = run_engine(case, bf16, trainable=False)
        for k in case.inputs:
            assert_exact(got.grads[k], r.grads[k], f"frozen d{k}")
        assert all(not bool(g.any()) for g in got.wgrads.values())


def test_marks_name_the_earliest_node_of_a_parameter():
    """Tape.marks: flat offset of a trainable parameter -> index of the FIRST node that uses it (its gradient is final
    once backward has passed that node); a module applied twice keeps the earlier index; frozen parameters and ops
    without parameters leave no mark."""
    from cultionet_amd import engine as E

    d = dev()
    m = nn.ModuleDict({"a": nn.Conv2d(8, 8, 1, bias=True), "b": nn.Conv2d(8, 8, 3, padding=1, bias=False),
                       "c": nn.Conv2d(8, 8, 1, bias=False)}).to(d)
    m["c"].weight.requires_grad_(False)
    store = E.ParamStore(m)
    store.zero_grad()
    off = lambda p: (p.data_ptr() - store._base) // 4
    with E.using_store(store), E.recording(True) as tape:
        x = E.Var(torch.zeros(1, 8, 5, 7, device=d), True)
        h0 = E.conv2d(x, m["b"], 1, 1, 1)       # node 0
        h1 = E.add(h0, x)                       # node 1
        h2 = E.conv2d(h1, m["a"], 1, 0, 1)      # node 2
        h3 = E.conv2d(h2, m["c"], 1, 0, 1)      # node 3 (frozen weight)
        h4 = E.conv2d(h3, m["a"], 1, 0, 1)      # node 4: a again
        h5 = E.conv2d(h4, m["b"], 1, 1, 1)      # node 5: b again
        assert len(tape.nodes) == 6
        assert tape.marks == {off(m["b"].weight): 0, off(m["a"].weight): 2, off(m["a"].bias): 2}
        assert off(m["c"].weight) not in tape.marks
        h5.grad = torch.zeros_like(h5.t)
        tape.backward()
        assert tape.nodes == []
    torch.cuda.synchronize()
