"""Times every fp32 BatchNorm launch shape of one default TowerUNet step (hidden 32, batch 8 of 100 x 100 chips) alone,
forward and backward. The shapes are not a list kept here: one training step runs with the four BatchNorm entry points
hooked, and every distinct call (groups, shape, strides, alignment, summed or not, residual, shared dy, accumulate
flags) is replayed on buffers of its own. Kernel durations come from torch.profiler (one call at a time on one stream,
the operands rotating over several buffer sets so that no call finds its inputs in the caches); a call's time is the sum
of its kernels. MB: the bytes the call's kernels move (one launch: every operand once; two launches: x and dy once per
pass, dy once per pass and GROUP unless the kernels that loop the groups ran). Four single calls that a step may not
make (fixed_rows) are timed as well, with n/step 0. Ends with the sum over one step.

    python tools/bn_bench.py [out.txt] [reps] [label]      (CN_LIB_PATH selects the library build)"""
import ctypes
import statistics
import sys

import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from cultionet_amd import _lib  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
LABEL = sys.argv[3] if len(sys.argv) > 3 else _lib.LIB_PATH
NSET = 3
NAMES = ("cn_bn_act_fwd_f32", "cn_bn_act_bwd_f32", "cn_bn_act_group_fwd_f32", "cn_bn_act_group_bwd_f32")
dev = torch.device("cuda:0")


def ptrs(tab, G):
    return [tab[g] or 0 for g in range(G)] if tab is not None else [0] * G


def describe(name, a):
    """The hashable description of one call: everything its path and its traffic depend on."""
    al = lambda ps: all(p % 16 == 0 for p in ps)
    if name == "cn_bn_act_group_fwd_f32":
        G, (B, C, L) = a[0], a[14:17]
        return dict(kind="fwd", G=G, B=B, C=C, L=L, train=a[17], act=a[20], summed=a[21], res=a[7] is not None,
                    strides=(a[2], a[10], a[8]), aligned=al(ptrs(a[1], G) + ptrs(a[9], G) + [a[7] or 0]), single=0)
    if name == "cn_bn_act_group_bwd_f32":
        G, (B, C, L) = a[0], a[15:18]
        dys, dxs = ptrs(a[3], G), ptrs(a[9], G)
        return dict(kind="bwd", G=G, B=B, C=C, L=L, train=a[18], act=a[19], shared=G > 1 and len(set(dys)) == 1,
                    acc=tuple(a[11][g] for g in range(G)), null=tuple(p == 0 for p in dxs), strides=(a[2], a[4], a[10]),
                    aligned=al(ptrs(a[1], G) + dys + dxs), single=0)
    if name == "cn_bn_act_fwd_f32":
        B, C, L = a[13:16]
        return dict(kind="fwd", G=1, B=B, C=C, L=L, train=a[16], act=a[19], summed=0, res=a[6] is not None,
                    strides=(a[1], a[9], a[7]), aligned=al([a[0], a[8], a[6] or 0]), single=1)
    B, C, L = a[14:17]
    return dict(kind="bwd", G=1, B=B, C=C, L=L, train=a[17], act=a[18], shared=False, acc=(a[19],), null=(a[8] is None,),
                strides=(a[1], a[3], a[9]), aligned=al([a[0], a[2], a[8] or 0]), single=1)


def step_calls():
    """{description: calls per step} of one default training step (bench.py's TrainLeg configuration)."""
    from cultionet_amd import synthetic as O
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=32, dropout=0.0)
    model = lit.cultionet_model.mask_model
    model.load_state_dict(O.seeded_state_dict(model.state_dict()))
    lit = lit.to(dev).train()
    x, y, bdist = O.seeded_batch(8, seed=7)
    batch = Data(x=x.to(dev), y=y.to(dev), bdist=bdist.to(dev), lon=torch.zeros(8, device=dev),
                 lat=torch.zeros(8, device=dev))
    trainer = HipTrainer(lit, gradient_clip_val=1.0, precision="32-true")
    trainer.training_step(batch)
    seen = {}
    orig = _lib.call

    def hooked(name, *a):
        if name in NAMES:
            d = describe(name, a)
            key = tuple(sorted(d.items()))
            seen[key] = seen.get(key, 0) + 1
        return orig(name, *a)

    _lib.call = hooked
    try:
        trainer.training_step(batch)
        torch.cuda.synchronize()
    finally:
        _lib.call = orig
    del trainer, lit, batch
    torch.cuda.empty_cache()
    return seen


def tensor(B, C, L, stride, aligned, fill=None):
    """[B, C, L] view with batch stride `stride`; not aligned: one float past a 16-byte boundary."""
    stride = max(stride, C * L)
    flat = torch.empty(B * stride + 4, device=dev)
    if fill is None:
        flat.normal_()
    else:
        flat.fill_(fill)
    off = 0 if aligned else 1
    return flat[off:off + B * stride].view(B, stride)[:, :C * L].view(B, C, L)


def kernel_times(fn):
    """[(microseconds, kernel names)] per call of REPS calls of fn(i), after NSET warm-up calls."""
    for i in range(NSET):
        fn(i)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(REPS):
            fn(i)
            torch.cuda.synchronize()
    evs = sorted((ev for ev in prof.events() if ev.device_type.name == "CUDA" and "cn_" in ev.name),
                 key=lambda ev: ev.time_range.start)
    per = len(evs) // REPS  # every call launches the same kernels
    assert per >= 1 and per * REPS == len(evs), (len(evs), REPS)
    out = []
    for i in range(REPS):
        mine = evs[i * per:(i + 1) * per]
        dur = sum(ev.device_time if hasattr(ev, "device_time") else ev.cuda_time for ev in mine)
        out.append((dur, tuple(ev.name.split("(")[0].replace("void ", "") for ev in mine)))
    return out


def replay(d):
    G, B, C, L = d["G"], d["B"], d["C"], d["L"]
    s = torch.cuda.current_stream().cuda_stream
    tab = lambda ts: (ctypes.c_void_p * G)(*[t.data_ptr() if t is not None else None for t in ts])
    sx, s2, s3 = d["strides"]
    al = d["aligned"]
    X = B * C * L * 4  # bytes of one tensor
    gam = [torch.randn(C, device=dev) for _ in range(G)]
    bet = [torch.randn(C, device=dev) for _ in range(G)]
    rm = [torch.zeros(C, device=dev) for _ in range(G)]
    rv = [torch.ones(C, device=dev) for _ in range(G)]
    mean = [torch.zeros(C, device=dev) for _ in range(G)]
    rstd = [torch.ones(C, device=dev) for _ in range(G)]
    ws = torch.empty(G * _lib.query("cn_bn_workspace_doubles", C), dtype=torch.float64, device=dev)
    xs = [[tensor(B, C, L, sx, al) for _ in range(G)] for _ in range(NSET)]
    if d["kind"] == "fwd":
        ny = 1 if d["summed"] else G
        ys = [[tensor(B, C, L, s2, al, 0.0) for _ in range(ny)] for _ in range(NSET)]
        res = [tensor(B, C, L, s3, al) if d["res"] else None for _ in range(NSET)]

        def fn(i):
            k = i % NSET
            r = res[k]
            if d["single"]:
                _lib.call("cn_bn_act_fwd_f32", xs[k][0].data_ptr(), xs[k][0].stride(0), gam[0].data_ptr(),
                          bet[0].data_ptr(), rm[0].data_ptr(), rv[0].data_ptr(), r.data_ptr() if r is not None else None,
                          r.stride(0) if r is not None else 0, ys[k][0].data_ptr(), ys[k][0].stride(0),
                          mean[0].data_ptr(), rstd[0].data_ptr(), ws.data_ptr(), B, C, L, d["train"], 0.1, 1e-5, d["act"],
                          s)
            else:
                _lib.call("cn_bn_act_group_fwd_f32", G, tab(xs[k]), xs[k][0].stride(0), tab(gam), tab(bet), tab(rm),
                          tab(rv), r.data_ptr() if r is not None else None, r.stride(0) if r is not None else 0,
                          tab([ys[k][0 if d["summed"] else g] for g in range(G)]), ys[k][0].stride(0), tab(mean),
                          tab(rstd), ws.data_ptr(), B, C, L, d["train"], 0.1, 1e-5, d["act"], d["summed"], s)

        runs = kernel_times(fn)
        passes = len(runs[0][1]) if d["train"] else 1
        nbytes = X * (G * passes + ny + (1 if d["res"] else 0))
    else:
        ndy = 1 if d["shared"] else G
        dys = [[tensor(B, C, L, s2, al) for _ in range(ndy)] for _ in range(NSET)]
        dxs = [[None if d["null"][g] else tensor(B, C, L, s3, al, 0.0) for g in range(G)] for _ in range(NSET)]
        acc = (ctypes.c_int * G)(*d["acc"])
        dg = [torch.zeros(C, device=dev) for _ in range(G)]
        db = [torch.zeros(C, device=dev) for _ in range(G)]
        coef = torch.empty(2 * C, device=dev)
        live = [t for t in dxs[0] if t is not None]
        dxbs = live[0].stride(0) if live else 0

        def fn(i):
            k = i % NSET
            if d["single"]:
                _lib.call("cn_bn_act_bwd_f32", xs[k][0].data_ptr(), xs[k][0].stride(0), dys[k][0].data_ptr(),
                          dys[k][0].stride(0), mean[0].data_ptr(), rstd[0].data_ptr(), gam[0].data_ptr(),
                          bet[0].data_ptr(), dxs[k][0].data_ptr() if dxs[k][0] is not None else None, dxbs,
                          dg[0].data_ptr(), db[0].data_ptr(), coef.data_ptr(), ws.data_ptr(), B, C, L, d["train"],
                          d["act"], d["acc"][0], 1, s)
            else:
                _lib.call("cn_bn_act_group_bwd_f32", G, tab(xs[k]), xs[k][0].stride(0),
                          tab([dys[k][0 if d["shared"] else g] for g in range(G)]), dys[k][0].stride(0), tab(mean),
                          tab(rstd), tab(gam), tab(bet), tab(dxs[k]), dxbs, acc, tab(dg), tab(db), ws.data_ptr(), B, C, L,
                          d["train"], d["act"], 1, s)

        runs = kernel_times(fn)
        passes = len(runs[0][1])
        looped = passes == 1 or any("shared" in n for n in runs[0][1])
        dy_reads = (1 if looped and d["shared"] else G) * passes
        nout = sum(1 for g in range(G) if not d["null"][g])
        nacc = sum(1 for g in range(G) if not d["null"][g] and d["acc"][g])
        nbytes = X * (G * passes + dy_reads + nout + nacc)
    ts = [t for t, _ in runs]
    return statistics.median(ts), min(ts), max(ts), nbytes, runs[0][1]


def label(d):
    t = f"{d['kind']} {'one' if d['single'] else 'G' + str(d['G'])} B{d['B']} C{d['C']} L{d['L']}"
    if d["kind"] == "fwd":
        t += (" sum" if d["summed"] else "") + (" +res" if d["res"] else "")
    else:
        t += (" dy1" if d["shared"] else "") + (" acc" + "".join(str(v) for v in d["acc"]) if any(d["acc"]) else "") \
            + (" null" + "".join(str(int(v)) for v in d["null"]) if any(d["null"]) else "")
    return t + ("" if d["aligned"] and d["L"] % 4 == 0 else " dword") + ("" if d["train"] else " eval")


def fixed_rows():
    """Single calls on the two-pass kernels that a default step may not make (n/step 0 then: outside the step's sum):
    the BatchNorm3d view of the time reduction both ways, an eval forward and a backward of 32 channels at 100 x 100."""
    def fwd(C, L, train):
        return dict(kind="fwd", G=1, B=8, C=C, L=L, train=train, act=1, summed=0, res=False, strides=(C * L, C * L, 0),
                    aligned=True, single=1)

    def bwd(C, L):
        return dict(kind="bwd", G=1, B=8, C=C, L=L, train=1, act=1, shared=False, acc=(0,), null=(False,),
                    strides=(C * L, C * L, C * L), aligned=True, single=1)

    return [fwd(3, 120000, 1), bwd(3, 120000), fwd(32, 10000, 0), bwd(32, 10000)]


calls = step_calls()
for d in fixed_rows():
    calls.setdefault(tuple(sorted(d.items())), 0)
lines = [f"library: {LABEL}",
         f"{'call':<44}{'n/step':>7}{'launches':>9}{'median us':>11}{'min':>8}{'max':>8}{'MB':>8}{'GB/s':>8}  kernels"]
total = 0.0
order = sorted(calls.items(), key=lambda kv: (dict(kv[0])["kind"], -dict(kv[0])["B"] * dict(kv[0])["L"], dict(kv[0])["C"]))
for key, n in order:
    d = dict(key)
    med, lo, hi, nbytes, kernels = replay(d)
    total += n * med
    short = "+".join(k.replace("cn_bn_", "").replace("_kernel", "") for k in kernels)
    lines.append(f"{label(d):<44}{n:>7}{len(kernels):>9}{med:>11.1f}{lo:>8.1f}{hi:>8.1f}{nbytes / 1e6:>8.1f}"
                 f"{nbytes / med / 1e3:>8.0f}  {short}")
    torch.cuda.empty_cache()
lines.append(f"one step: {sum(calls.values())} calls, sum of medians {total:.1f} us")
text = "\n".join(lines)
print(text)
if OUT:
    with open(OUT, "a") as f:
        f.write(text + "\n\n")
