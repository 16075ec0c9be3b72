"""Reference of the tape layer (cultionet_amd/tape.py) and of the pure-plumbing ops of the engine, for
tests/test_tape_ref.py (CPU) and tests/test_tape_exact_gpu.py, plus the restatement of cn_channel_sum_bf16's summation
order for tests/test_glue_kernels_exact_gpu.py.

A graph is DATA: a short list of steps ``(op, input names, output name(s), kwargs)``. `run_ref` interprets it in
float64 torch autograd on the CPU; the GPU module interprets the same list in engine ops. The ops:

    conv      y = conv2d(x, weight kw["w"]) ("same" padding, no bias); kw["out"] = (buffer, c0): written in place into
              channels [c0, c0 + Cout) of a buffer
    pool      adaptive_max_pool2d to kw["size"]
    cat       cat_channels(inputs, buf=kw.get("buf"))
    split     split_channels into kw["sizes"]; the outputs are the slice names
    join      join_channels(inputs, buffer kw["buf"])
    add       add(a, b)
    flip      the converter that leaves the current precision: to_bf16 on an fp32 Var, to_f32 on a bf16 one (the
              identity in float64)
    buffer    a fresh activation buffer with kw["C"] channels in the precision of Var kw["like"]
    spawn     run kw["steps"] on aliases kw["args"] of the inputs as a branch; the output names kw["result"]
    sync      join() the branch named by the input

Inputs, weights and upstream gradients are small integers (`ints` of conv_exact_worker), so every activation and every
gradient is an integer; while all of them stay within +-256 they are exact in bf16 as well as in fp32, whatever is
aliased, copied or accumulated in whatever order. `premise256` asserts that for every Var of a case, with the
accumulated gradient bounded by the sum of the absolute contributions of its uses (every partial sum of an accumulation
is then within the bound too).
"""
from __future__ import annotations

import itertools

import torch
import torch.nn.functional as F

from conv_exact_worker import ints, premise, term_bound

PLUMBING = ("cat", "add", "join")            # consumers that hand their gradient on through give_grad
KERNELS = ("conv1", "conv3", "pool", "flip")  # consumers that take grad_buffer()'s accumulate flag into a kernel
NO_USE = ("split", "spawn", "sync", "buffer")  # steps that are structure, not a use of their input


class Case:
    def __init__(self, name, B, HW, inputs, weights, steps, outs, no_dy=(), claims=()):
        self.name, self.B, self.H, self.W = name, B, HW[0], HW[1]
        self.inputs = {k: (v if isinstance(v, tuple) else (v, True)) for k, v in inputs.items()}  # name -> (C, req)
        self.weights = dict(weights)  # name -> (Cout, Cin, k)
        self.steps, self.outs, self.no_dy, self.claims = list(steps), tuple(outs), tuple(no_dy), tuple(claims)

    def __repr__(self):
        return self.name


def seed_of(case, what):
    return sum(ord(c) * (i + 1) for i, c in enumerate(case.name + "/" + what)) % 100003


def make_inputs(case):
    """name -> float64 [B, C, H, W] with integers in -2..2."""
    return {k: ints((case.B, c, case.H, case.W), -2, 2, seed_of(case, k)) for k, (c, _) in case.inputs.items()}


def make_weights(case):
    """name -> float64 [Cout, Cin, k, k] with entries in -1..1, sparse enough for sums over Cin * k * k taps to stay
    small (about 6 non-zero taps per output channel)."""
    out = {}
    for k, (co, ci, ks) in case.weights.items():
        out[k] = ints((co, ci, ks, ks), -1, 1, seed_of(case, k), zeros=max(0.0, 1.0 - 6.0 / (ci * ks * ks)))
    return out


def make_dys(case, outs):
    return {k: ints(tuple(outs[k].shape), -1, 1, seed_of(case, "d" + k), zeros=0.3) for k in case.outs
            if k not in case.no_dy}


def walk(steps, prefix=()):
    """(step id, step) of every step, branches included."""
    for i, st in enumerate(steps):
        yield prefix + (i,), st
        if st[0] == "spawn":
            yield from walk(st[3]["steps"], prefix + (i,))


def uses(case):
    """Every edge (step id, input position, Var name) at which an op reads a Var."""
    return [(sid, j, n) for sid, (op, ins, _, _) in walk(case.steps) if op not in NO_USE for j, n in enumerate(ins)]


def _canon(case):
    """Resolver of names to the Var they stand for: a branch's alias is its input, its output is its result."""
    alias = {}
    for _, (op, ins, out, kw) in walk(case.steps):
        if op == "spawn":
            alias.update(zip(kw["args"], ins))
            alias[out] = kw["result"]

    def res(n):
        return res(alias[n]) if n in alias else n

    return res


def live_steps(case):
    """Ids of the steps whose output reaches an output that receives a dy (the others have no gradient to hand on)."""
    res = _canon(case)
    flat = [(sid, st) for sid, st in walk(case.steps) if st[0] not in ("spawn", "sync", "buffer")]
    flat.sort(key=lambda e: e[0])  # forward order: a branch's steps (i, j) sort between steps i and i + 1
    live_names = {res(o) for o in case.outs if o not in case.no_dy}
    live = set()
    for sid, (op, ins, out, kw) in reversed(flat):
        outs_ = out if isinstance(out, tuple) else (out,)
        if any(res(o) in live_names for o in outs_):
            live.add(sid)
            live_names.update(res(n) for n in ins)
    return live


class RefRun:
    """Result of run_ref: outs, grads (inputs; None where autograd reaches none), wgrads, and for the premise every
    Var's value and the gradient contribution of every use."""


def run_ref(case, xs=None, ws=None, dys=None, cut=None):
    """The graph in float64 autograd. `cut` = (step id, input position): that one use reads a detached copy."""
    xs = make_inputs(case) if xs is None else xs
    ws = make_weights(case) if ws is None else ws
    env = {k: v.clone().requires_grad_(case.inputs[k][1]) for k, v in xs.items()}
    wv = {k: v.clone().requires_grad_(True) for k, v in ws.items()}
    edge = {}

    def use(sid, j, name):
        t = env[name]
        if cut == (sid, j):
            return t.detach()
        t = t * 1.0  # a node of its own: its .grad is this use's contribution
        if t.requires_grad:
            t.retain_grad()
        edge[(sid, j, name)] = t
        return t

    def run(steps, prefix):
        for i, (op, ins, out, kw) in enumerate(steps):
            sid = prefix + (i,)
            a = [use(sid, j, n) for j, n in enumerate(ins)] if op not in NO_USE else None
            if op == "conv":
                w = wv[kw["w"]]
                env[out] = F.conv2d(a[0], w, None, 1, w.shape[2] // 2)
            elif op == "pool":
                env[out] = F.adaptive_max_pool2d(a[0], kw["size"])
            elif op in ("cat", "join"):
                env[out] = torch.cat(a, 1)
            elif op == "add":
                env[out] = a[0] + a[1]
            elif op == "flip":
                env[out] = a[0]
            elif op == "split":
                for o, t in zip(out, torch.split(env[ins[0]], list(kw["sizes"]), 1)):
                    env[o] = t
            elif op == "spawn":
                for an, n in zip(kw["args"], ins):
                    env[an] = env[n]
                run(kw["steps"], sid)
                env[out] = env[kw["result"]]
            elif op in ("buffer", "sync"):
                pass
            else:
                raise ValueError(op)

    run(case.steps, ())
    r = RefRun()
    r.xs, r.ws = xs, ws
    r.outs = {k: env[k].detach() for k in case.outs}
    r.dys = make_dys(case, r.outs) if dys is None else dys
    loss = sum((env[k] * d).sum() for k, d in r.dys.items())
    if isinstance(loss, torch.Tensor) and loss.requires_grad:
        loss.backward()
    r.grads = {k: env[k].grad for k in xs}
    r.wgrads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in wv.items()}
    r.values = {k: v.detach() for k, v in env.items()}
    r.edge_grads = {k: t.grad for k, t in edge.items() if t.requires_grad}
    return r


def premise256(case, r=None):
    """Every activation, every gradient contribution and every accumulated gradient of the case is an integer within
    +-256 (exact in bf16 and fp32); the weight gradients' sums stay below 2^24 (`premise`)."""
    r = run_ref(case) if r is None else r
    worst = 0.0
    for k, v in r.values.items():
        assert torch.equal(v, v.round()), f"{case}: {k} is not integer"
        worst = max(worst, float(v.abs().max()))
    acc = {}
    for (sid, j, name), g in r.edge_grads.items():
        if g is None:
            continue
        assert torch.equal(g, g.round()), f"{case}: gradient into {name} at {sid} is not integer"
        acc[name] = acc.get(name, 0.0) + float(g.abs().max())
    for name, b in acc.items():
        worst = max(worst, b)
    assert worst <= 256, f"{case}: bf16 premise fails, a value or an accumulated gradient may reach {worst:.0f} > 256"
    w = torch.tensor(worst)
    premise(f"{case} weight gradients", term_bound(w, w, case.B * case.H * case.W))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

def _fanout(kinds, B, HW, tag):
    """h = conv1x1(x) read by the consumers `kinds`, in that forward order; every consumer's result is an output."""
    join = "join" in kinds
    weights = {"wpre": (8, 8, 1)}
    inputs = {"x": 8}
    steps, outs = [], []
    if join:
        steps += [("buffer", (), "jb", {"C": 16, "like": "x"}), ("conv", ("x",), "h", {"w": "wpre", "out": ("jb", 0)})]
    else:
        steps += [("conv", ("x",), "h", {"w": "wpre"})]
    for i, k in enumerate(kinds):
        o = f"o{i}"
        if k == "cat":
            inputs[f"z{i}"] = 8
            steps.append(("cat", ("h", f"z{i}"), o, {}))
        elif k == "add":
            inputs[f"z{i}"] = 8
            steps.append(("add", ("h", f"z{i}"), o, {}))
        elif k == "addb":
            inputs[f"z{i}"] = 8
            steps.append(("add", (f"z{i}", "h"), o, {}))
        elif k == "join":
            inputs[f"z{i}"] = 8
            weights[f"wj{i}"] = (8, 8, 1)
            steps += [("conv", (f"z{i}",), f"p{i}", {"w": f"wj{i}", "out": ("jb", 8)}),
                      ("join", ("h", f"p{i}"), o, {"buf": "jb"})]
        elif k in ("conv1", "conv3"):
            weights[f"w{i}"] = (8, 8, int(k[-1]))
            steps.append(("conv", ("h",), o, {"w": f"w{i}"}))
        elif k == "pool":
            steps.append(("pool", ("h",), o, {"size": (2, 3)}))
        elif k == "flip":
            steps.append(("flip", ("h",), o, {}))
        else:
            raise ValueError(k)
        outs.append(o)
    return Case(f"fanout{tag}-" + "-".join(kinds), B, HW, inputs, weights, steps, outs,
                claims=[("consumers", "h", tuple(kinds))])


def _fanout_cases():
    kinds = ("cat", "add", "addb", "join", "conv1", "conv3", "pool", "flip")
    cases = [_fanout((k,), 1 + 2 * (i % 2), (5, 7), "1") for i, k in enumerate(kinds)]
    pairs = [(a, b) for a in kinds for b in kinds if a != b and not {a, b} <= {"add", "addb"} and not {a, b} <= {"conv1", "conv3"}]
    pairs += [("cat", "cat"), ("conv3", "conv3"), ("add", "add"), ("pool", "pool"), ("flip", "flip")]
    cases += [_fanout(p, 1 + 2 * (i % 2), (5, 7) if i % 3 else (9, 9), "2") for i, p in enumerate(pairs)]
    for trio in (("cat", "conv3", "flip"), ("add", "pool", "join"), ("addb", "conv1", "cat")):
        cases += [_fanout(p, 1 + 2 * (i % 2), (5, 7), "3") for i, p in enumerate(itertools.permutations(trio))]
    return cases


def _named_cases():
    C = Case
    S3 = {"sizes": (8, 8, 8)}
    pre24 = [("conv", ("x",), "h", {"w": "wpre"}), ("split", ("h",), ("s0", "s1", "s2"), S3)]
    cases = [
        # ---- slices ----
        C("slices-all-used", 3, (5, 7), {"x": 8, "z": 8}, {"wpre": (24, 8, 1), "w0": (8, 8, 3)},
          pre24 + [("conv", ("s0",), "o0", {"w": "w0"}), ("pool", ("s1",), "o1", {"size": (2, 3)}),
                   ("add", ("s2", "z"), "o2", {})], ("o0", "o1", "o2"),
          claims=[("sliced", "h", 3, 3)]),
        C("slices-one-unused", 1, (9, 9), {"x": 8, "z": 8}, {"wpre": (24, 8, 1), "w0": (8, 8, 1)},
          pre24 + [("conv", ("s0",), "o0", {"w": "w0"}), ("cat", ("s2", "z"), "o2", {})], ("o0", "o2"),
          claims=[("sliced", "h", 3, 2)]),
        C("slices-one-unused-input", 3, (5, 7), {"x": 24, "z": 8}, {"w0": (8, 8, 3)},
          [("split", ("x",), ("s0", "s1", "s2"), S3), ("conv", ("s1",), "o0", {"w": "w0"}),
           ("add", ("z", "s2"), "o2", {})], ("o0", "o2"),
          claims=[("sliced", "x", 3, 2), ("consumers", "s2", ("addb",))]),  # a slice as add's second operand
        C("slices-added", 3, (5, 7), {"x": 8}, {"wpre": (24, 8, 1)},
          pre24 + [("add", ("s0", "s1"), "o0", {}), ("add", ("s2", "s2"), "o1", {}), ("add", ("s2", "s0"), "o2", {})],
          ("o0", "o1", "o2"), claims=[("sliced", "h", 3, 3), ("consumers", "s1", ("addb",)),
                                      ("consumers", "s2", ("add", "addb", "add")), ("consumers", "s0", ("add", "addb"))]),
        C("slices-none-used", 3, (5, 7), {"x": 24, "z": 8}, {"w0": (8, 8, 1)},
          [("split", ("x",), ("s0", "s1", "s2"), S3), ("conv", ("z",), "o0", {"w": "w0"})], ("o0",),
          claims=[("sliced", "x", 3, 0), ("no-grad", "x")]),
        C("slice-used-twice", 3, (5, 7), {"x": 8, "z": 8}, {"wpre": (24, 8, 1), "w0": (8, 8, 1)},
          pre24 + [("conv", ("s0",), "o0", {"w": "w0"}), ("add", ("s0", "z"), "o1", {}), ("cat", ("s1", "s1"), "o2", {}),
                   ("pool", ("s2",), "o3", {"size": (2, 3)}), ("flip", ("s2",), "o4", {})],
          ("o0", "o1", "o2", "o3", "o4"), claims=[("consumers", "s0", ("conv1", "add")), ("consumers", "s1", ("cat", "cat")),
                                                  ("consumers", "s2", ("pool", "flip"))]),
        C("parent-read-before-slices-kernel", 3, (5, 7), {"x": 8, "z": 8}, {"wpre": (24, 8, 1), "wp": (8, 24, 3)},
          [("conv", ("x",), "h", {"w": "wpre"}), ("conv", ("h",), "o0", {"w": "wp"}),
           ("split", ("h",), ("s0", "s1", "s2"), S3), ("add", ("s0", "z"), "o1", {}),
           ("pool", ("s2",), "o2", {"size": (2, 3)})], ("o0", "o1", "o2"),
          claims=[("order", "h", "conv3", "before"), ("sliced", "h", 3, 2)]),
        C("parent-read-after-slices-kernel", 1, (9, 9), {"x": 8, "z": 8}, {"wpre": (24, 8, 1), "wp": (8, 24, 3)},
          pre24 + [("add", ("s0", "z"), "o1", {}), ("pool", ("s2",), "o2", {"size": (3, 3)}),
                   ("conv", ("h",), "o0", {"w": "wp"})], ("o1", "o2", "o0"),
          claims=[("order", "h", "conv3", "after"), ("sliced", "h", 3, 2)]),
        C("parent-read-before-slices-plumbing", 3, (5, 7), {"x": 8, "z": 24, "y": 8}, {"wpre": (24, 8, 1), "w1": (8, 8, 3)},
          [("conv", ("x",), "h", {"w": "wpre"}), ("add", ("h", "z"), "o0", {}),
           ("split", ("h",), ("s0", "s1", "s2"), S3), ("conv", ("s1",), "o1", {"w": "w1"}),
           ("cat", ("y", "s2"), "o2", {})], ("o0", "o1", "o2"),
          claims=[("order", "h", "add", "before"), ("sliced", "h", 3, 2)]),
        C("parent-read-after-slices-plumbing", 3, (5, 7), {"x": 8, "z": 24, "y": 8}, {"wpre": (24, 8, 1), "w1": (8, 8, 3)},
          pre24 + [("conv", ("s1",), "o1", {"w": "w1"}), ("cat", ("y", "s2"), "o2", {}), ("add", ("h", "z"), "o0", {}),
                   ("cat", ("h", "y"), "o3", {})], ("o1", "o2", "o0", "o3"),
          claims=[("order", "h", "add", "after"), ("sliced", "h", 3, 2)]),
        C("slices-reordered", 3, (5, 7), {"x": 8}, {"wpre": (24, 8, 1), "w1": (8, 24, 1)},
          pre24 + [("cat", ("s2", "s0", "s1"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w1"})], ("o0", "o1"),
          claims=[("sliced", "h", 3, 3)]),
        C("slices-reordered-input", 1, (9, 9), {"x": 24}, {},
          [("split", ("x",), ("s0", "s1", "s2"), S3), ("cat", ("s1", "s2", "s0", "s1"), "o0", {})], ("o0",),
          claims=[("sliced", "x", 3, 3)]),
        # ---- cat_channels ----
        C("cat-fresh", 3, (5, 7), {"a": 8, "b": 16, "c": 8}, {"w": (8, 32, 3)},
          [("cat", ("a", "b", "c"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w"})], ("o0", "o1")),
        C("cat-fresh-b1", 1, (9, 9), {"a": 8, "b": 16}, {}, [("cat", ("a", "b"), "o0", {})], ("o0",)),
        C("cat-buf-in-place", 3, (5, 7), {"x": 8, "z": 8}, {"wa": (8, 8, 3), "wb": (16, 8, 1), "w": (8, 24, 1)},
          [("buffer", (), "cb", {"C": 24, "like": "x"}), ("conv", ("x",), "p0", {"w": "wa", "out": ("cb", 0)}),
           ("conv", ("z",), "p1", {"w": "wb", "out": ("cb", 8)}), ("cat", ("p0", "p1"), "y", {"buf": "cb"}),
           ("conv", ("y",), "o0", {"w": "w"})], ("y", "o0")),
        C("cat-buf-mixed", 3, (5, 7), {"x": 8, "z": 8, "q": 8}, {"wa": (8, 8, 3), "wb": (8, 8, 1), "w": (8, 32, 1)},
          [("buffer", (), "cb", {"C": 32, "like": "x"}), ("conv", ("x",), "p0", {"w": "wa", "out": ("cb", 0)}),
           ("conv", ("z",), "p1", {"w": "wb"}), ("conv", ("z",), "p3", {"w": "wb", "out": ("cb", 24)}),
           ("cat", ("p0", "p1", "q", "p3"), "y", {"buf": "cb"}), ("conv", ("y",), "o0", {"w": "w"})], ("y", "o0")),
        C("cat-buf-mixed-b1", 1, (9, 9), {"x": 8, "q": 16}, {"wa": (8, 8, 3)},
          [("buffer", (), "cb", {"C": 24, "like": "x"}), ("conv", ("x",), "p0", {"w": "wa", "out": ("cb", 16)}),
           ("cat", ("q", "p0"), "y", {"buf": "cb"})], ("y",)),
        C("cat-x-x", 3, (5, 7), {"x": 8}, {"wpre": (8, 8, 1), "w": (8, 16, 3)},
          [("conv", ("x",), "h", {"w": "wpre"}), ("cat", ("h", "h"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w"}),
           ("cat", ("x", "x", "x"), "o2", {})], ("o0", "o1", "o2"),
          claims=[("consumers", "h", ("cat", "cat")), ("consumers", "x", ("conv1", "cat", "cat", "cat"))]),
        # ---- add ----
        C("add-b-absent", 3, (5, 7), {"a": 8, "b": 8}, {"w": (8, 8, 3)},
          [("add", ("a", "b"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w"})], ("o0", "o1")),
        C("add-b-present", 3, (5, 7), {"a": 8, "b": 8}, {"w": (8, 8, 3)},
          [("add", ("a", "b"), "o0", {}), ("conv", ("b",), "o1", {"w": "w"}), ("cat", ("b", "a"), "o2", {})],
          ("o0", "o1", "o2"), claims=[("consumers", "b", ("addb", "conv3", "cat"))]),
        C("add-a-frozen", 3, (5, 7), {"a": (8, False), "b": 8}, {"w": (8, 8, 1)},
          [("add", ("a", "b"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w"}), ("add", ("a", "o1"), "o2", {})],
          ("o0", "o1", "o2"), claims=[("no-grad", "a")]),
        C("add-b-frozen", 1, (9, 9), {"a": 8, "b": (8, False)}, {"w": (8, 8, 1)},
          [("add", ("a", "b"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w"}), ("add", ("o1", "b"), "o2", {})],
          ("o0", "o1", "o2"), claims=[("no-grad", "b")]),
        C("add-x-x", 3, (5, 7), {"x": 8}, {"wpre": (8, 8, 1), "w": (8, 8, 3)},
          [("conv", ("x",), "h", {"w": "wpre"}), ("add", ("h", "h"), "o0", {}), ("conv", ("o0",), "o1", {"w": "w"}),
           ("add", ("x", "x"), "o2", {})], ("o0", "o1", "o2"),
          claims=[("consumers", "h", ("add", "addb")), ("consumers", "x", ("conv1", "add", "addb"))]),
        # ---- precision edges: flip -> ... -> flip -> ... -> flip, fan-out on both sides of each converter ----
        C("precision-chain-others-after", 3, (5, 7), {"x": 8, "z": 8},
          {"wx": (8, 8, 3), "wu": (8, 8, 1), "wv": (8, 8, 3), "wt": (8, 8, 1)},
          [("flip", ("x",), "u", {}), ("conv", ("x",), "o0", {"w": "wx"}),
           ("flip", ("u",), "v", {}), ("conv", ("u",), "o1", {"w": "wu"}), ("cat", ("u", "u"), "o5", {}),
           ("add", ("v", "z"), "w", {}), ("flip", ("w",), "t", {}), ("conv", ("v",), "o2", {"w": "wv"}),
           ("pool", ("w",), "o6", {"size": (2, 3)}),
           ("pool", ("t",), "o3", {"size": (2, 3)}), ("conv", ("t",), "o4", {"w": "wt"})],
          ("o0", "o1", "o2", "o3", "o4", "o5", "o6"),
          claims=[("consumers", "x", ("flip", "conv3")), ("consumers", "u", ("flip", "conv1", "cat", "cat")),
                  ("consumers", "v", ("add", "conv3")), ("consumers", "w", ("flip", "pool")),
                  ("consumers", "t", ("pool", "conv1"))]),
        C("precision-chain-others-before", 1, (9, 9), {"x": 8, "z": 8},
          {"wx": (8, 8, 3), "wu": (8, 8, 1), "wv": (8, 8, 3), "wt": (8, 8, 1)},
          [("conv", ("x",), "o0", {"w": "wx"}), ("flip", ("x",), "u", {}),
           ("conv", ("u",), "o1", {"w": "wu"}), ("flip", ("u",), "v", {}),
           ("conv", ("v",), "o2", {"w": "wv"}), ("add", ("z", "v"), "w", {}), ("pool", ("w",), "o6", {"size": (3, 3)}),
           ("flip", ("w",), "t", {}),
           ("pool", ("t",), "o3", {"size": (3, 3)}), ("conv", ("t",), "o4", {"w": "wt"})],
          ("o0", "o1", "o2", "o3", "o4", "o6"),
          claims=[("consumers", "x", ("conv3", "flip")), ("consumers", "u", ("conv1", "flip")),
                  ("consumers", "v", ("conv3", "addb")), ("consumers", "w", ("pool", "flip"))]),
        # ---- an output without dy ----
        C("output-without-dy", 3, (5, 7), {"x": 8, "z": 8}, {"wpre": (8, 8, 1), "w1": (8, 8, 3), "w2": (8, 8, 1)},
          [("conv", ("x",), "h", {"w": "wpre"}), ("conv", ("h",), "o0", {"w": "w1"}), ("conv", ("h",), "o1", {"w": "w2"}),
           ("cat", ("h", "z"), "o2", {}), ("add", ("h", "z"), "m", {}), ("pool", ("m",), "o3", {"size": (2, 3)}),
           ("add", ("z", "h"), "o4", {})], ("o0", "o1", "o2", "o3", "o4"), no_dy=("o1", "o2", "o3"),
          claims=[("consumers", "h", ("conv3", "conv1", "cat", "add", "addb"))]),
        # ---- spawn / join ----
        C("spawn-branch", 3, (5, 7), {"x": 8}, {"wpre": (8, 8, 1), "wm": (8, 8, 3), "wb1": (8, 8, 3), "wb2": (8, 8, 1)},
          [("conv", ("x",), "h", {"w": "wpre"}),
           ("spawn", ("h",), "r", {"args": ("ha",), "result": "b2",
                                   "steps": [("conv", ("ha",), "b1", {"w": "wb1"}), ("conv", ("b1",), "b2", {"w": "wb2"})]}),
           ("conv", ("h",), "m", {"w": "wm"}), ("sync", ("r",), None, {}), ("add", ("m", "r"), "o0", {})], ("o0",),
          claims=[("consumers", "h", ("conv3", "conv3")), ("branch", "r", 2)]),
        C("spawn-branch-input", 1, (9, 9), {"x": 8}, {"wm": (8, 8, 1), "wb1": (8, 8, 3)},
          [("conv", ("x",), "m", {"w": "wm"}),
           ("spawn", ("x",), "r", {"args": ("xa",), "result": "b2",
                                   "steps": [("conv", ("xa",), "b1", {"w": "wb1"}), ("pool", ("b1",), "b2", {"size": (3, 3)})]}),
           ("pool", ("m",), "mp", {"size": (3, 3)}), ("sync", ("r",), None, {}), ("cat", ("mp", "r"), "o0", {})], ("o0",),
          claims=[("consumers", "x", ("conv1", "conv3")), ("branch", "r", 2)]),
    ]
    return cases


CASES = _fanout_cases() + _named_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def consumers_of(case, name):
    """Kinds of the ops that read Var `name` (conv1 / conv3 / pool / flip / cat / join / add / addb, the second operand
    of an add), in forward order; the alias of a branch counts as the Var it stands for. A Var read twice by one op
    counts twice."""
    res = _canon(case)
    out = []
    for _, (op, ins, _, kw) in walk(case.steps):
        if op in NO_USE:
            continue
        kind = op + str(case.weights[kw["w"]][2]) if op == "conv" else op
        out += [kind + "b" if op == "add" and j == 1 else kind for j, n in enumerate(ins) if res(n) == name]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cn_channel_sum_bf16: the order of its fp32 sums, and the bound that follows from it
# ---------------------------------------------------------------------------------------------------------------------

def bbn_grid(P, C):
    """bbn_grid of cn_bnorm.hip: (blocks, rows per block, R thread rows)."""
    R = 256 // (C // 8)
    want = min(max(-(-P // (R * 8)), 1), 512)
    rows = -(-P // want)
    rows = -(-rows // R) * R
    return -(-P // rows), rows, R


def channel_sum_rows(C):
    """The P of the channel-sum tests: 1, R - 1, R, 2R + 1, 8R + 1 (the first P with two blocks) and, for C = 128,
    73,723 (512 blocks of 144 rows, the last one short: past the cap of 512 blocks, where the rows per block grow)."""
    R = 256 // (C // 8)
    ps = sorted({p for p in (1, R - 1, R, 2 * R + 1, 8 * R + 1) if p >= 1})
    return ps + ([73723] if C == 128 else [])


def channel_sum_depth(P, C):
    """D of the bound D * 2^-24 * sum|x| of cn_channel_sum_bf16, counted from cn_bsum_ticket_kernel: a thread sums
    m = rows / R pixels in pairs (one rounding for the pair, one for adding it to the running sum: no value passes more
    than m roundings, and for m >= 2 no more than m / 2 + 1), one thread per column then adds the R thread rows in turn
    (R), the block rows are combined in fp64 and the total is cast to fp32 once (1): bbn_depth of test_norm_gpu.py
    plus the cast. The chain is counted at m although it is at most m / 2 + 1 long, which more than covers the
    second-order terms of the product of (1 + 2^-24) factors and the fp64 sums of the block rows."""
    _, rows, R = bbn_grid(P, C)
    return rows // R + R + 1


def channel_sum_emulated(x, drop_last_row=False):
    """cn_bsum_ticket_kernel restated with sequential fp32 arithmetic: x [P, C] float32 (bf16-representable) ->
    float32 [C]. `drop_last_row`: a kernel that forgets the last pixel."""
    P, C = x.shape
    nblk, rows, R = bbn_grid(P, C)
    if drop_last_row:
        x = x[:P - 1]
    Pe = x.shape[0]
    tot = torch.zeros(C, dtype=torch.float64)
    for b in range(nblk):
        p0, p1 = b * rows, min(b * rows + rows, Pe)
        red = torch.zeros(R, C, dtype=torch.float32)
        p = p0
        while p + R < p1:  # rows p .. p+R-1 (one per thread row) paired with rows p+R .. p+2R-1
            na = min(R, p1 - p)
            nb = max(0, min(R, p1 - (p + R)))
            # a thread row r takes the pair only while p + r + R < p1; otherwise its single row is the tail
            pair = torch.zeros(R, C, dtype=torch.float32)
            pair[:nb] = x[p:p + nb] + x[p + R:p + R + nb]
            pair[nb:na] = x[p + nb:p + na]
            red = red + pair
            p += 2 * R
        if p < p1:
            na = min(R, p1 - p)
            red[:na] = red[:na] + x[p:p + na]
        s = torch.zeros(C, dtype=torch.float32)
        for r in range(R):
            s = s + red[r]
        tot += s.double()
    return tot.float()


def channel_sum_bound(x, P, C, old=None):
    """Per-channel bound of |out - float64 sum|: D u sum|x|, plus one rounding of |old| + |sum x| when accumulating."""
    u = 2.0 ** -24
    b = channel_sum_depth(P, C) * u * x.double().abs().sum(0)
    if old is not None:
        b = b + u * (old.double().abs() + x.double().sum(0).abs())
    return b
