"""Times the fp32 neighborhood-attention and LayerNorm launches of one TowerUNet step (hidden 32, batch 8 of 100 x 100
chips) alone, per attention site, with the bytes each launch has to move and the bandwidth that gives; cn_bn_group_apply
on a tensor of the same size is the yardstick. Kernel durations come from torch.profiler (one launch at a time on one
stream, the operands rotating over several buffer sets so that no launch finds its inputs in the caches).

    python tools/na_ln_bench.py [out.txt] [reps]"""
import ctypes
import statistics
import sys

import torch
from torch.profiler import ProfilerActivity, profile

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from cultionet_amd import _lib  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else None
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 12
NSET = 3
B, C = 8, 128
SITES = {"a 100x100": (100, 100, 4, 2), "b 50x50": (50, 50, 4, 1), "c 25x25": (25, 25, 8, 1)}  # H, W, heads, dilation
dev = torch.device("cuda:0")
s = torch.cuda.current_stream().cuda_stream


def rnd(*shape):
    return torch.randn(*shape, device=dev)


def kernel_times(fn):
    """{kernel name: [durations in us]} of REPS calls of fn(i), after NSET warm-up calls."""
    for i in range(NSET):
        fn(i)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(REPS):
            fn(i)
            torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if ev.device_type.name == "CUDA" and "cn_" in ev.name:
            dur = ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            out.setdefault(ev.name.split("(")[0], []).append(dur)
    return out


rows = []


def record(site, fn, nbytes):
    """nbytes: {substring of the kernel name: bytes moved}."""
    for name, ts in sorted(kernel_times(fn).items()):
        key = next((k for k in nbytes if k in name), None)
        by = nbytes[key] if key else 0
        med = statistics.median(ts)
        rows.append((site, name.replace("void ", ""), len(ts), med, min(ts), max(ts), by / 1e6, by / med / 1e3 if med else 0.0))


for site, (H, W, heads, dil) in SITES.items():
    HW = H * W
    X = B * C * HW * 4  # bytes of one C-channel tensor
    D = C // heads
    A = B * heads * 9 * HW * 4
    qkv = [rnd(B, 3 * C, H, W) for _ in range(NSET)]
    x = [rnd(B, C, H, W) for _ in range(NSET)]
    dy = [rnd(B, C, H, W) for _ in range(NSET)]
    y = [torch.empty(B, C, H, W, device=dev) for _ in range(NSET)]
    attn = [torch.empty(B, heads, 9, H, W, device=dev) for _ in range(NSET)]
    dattn = [torch.empty(B, heads, 9, H, W, device=dev) for _ in range(NSET)]
    dqkv = [torch.empty(B, 3 * C, H, W, device=dev) for _ in range(NSET)]
    mu, rstd = torch.empty(B, HW, device=dev), torch.empty(B, HW, device=dev)
    w, bvec = rnd(C), rnd(C)
    dw, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    nws = _lib.query("cn_layernorm_c_workspace_floats", B, C, HW)
    ws = torch.empty(max(nws, 1), device=dev)

    def na_fwd(i):
        k = i % NSET
        _lib.call("cn_na2d_fwd_f32", qkv[k].data_ptr(), 3 * C * HW, y[k].data_ptr(), C * HW, attn[k].data_ptr(), B, C,
                  heads, H, W, 3, dil, 0.0, 0, None, s)

    def na_bwd(i):
        k = i % NSET
        _lib.call("cn_na2d_bwd_f32", qkv[k].data_ptr(), 3 * C * HW, dy[k].data_ptr(), C * HW, attn[k].data_ptr(),
                  dattn[k].data_ptr(), dqkv[k].data_ptr(), 3 * C * HW, B, C, heads, H, W, 3, dil, 0.0, 0, None, s)

    def ln_fwd(res):
        def fn(i):
            k = i % NSET
            _lib.call("cn_layernorm_c_fwd_f32", x[k].data_ptr(), C * HW, w.data_ptr(), bvec.data_ptr(),
                      dy[k].data_ptr() if res else None, C * HW if res else 0, y[k].data_ptr(), C * HW, mu.data_ptr(),
                      rstd.data_ptr(), B, C, HW, 1e-5, s)
        return fn

    def ln_bwd(acc):
        def fn(i):
            k = i % NSET
            _lib.call("cn_layernorm_c_bwd_f32", x[k].data_ptr(), C * HW, dy[k].data_ptr(), C * HW, w.data_ptr(),
                      mu.data_ptr(), rstd.data_ptr(), y[k].data_ptr(), C * HW, dw.data_ptr(), db.data_ptr(), B, C, HW, acc,
                      ws.data_ptr(), nws, s)
        return fn

    # eval-mode group BatchNorm of one group: the apply kernel alone, x -> y
    xs = [(ctypes.c_void_p * 1)(t.data_ptr()) for t in x]
    ys = [(ctypes.c_void_p * 1)(t.data_ptr()) for t in y]
    one = [(ctypes.c_void_p * 1)(t.data_ptr()) for t in (w, bvec, torch.zeros(C, device=dev), torch.ones(C, device=dev),
                                                           torch.empty(C, device=dev), torch.empty(C, device=dev))]
    bws = torch.empty(_lib.query("cn_bn_workspace_doubles", C), dtype=torch.float64, device=dev)

    def bn_apply(i):
        k = i % NSET
        _lib.call("cn_bn_act_group_fwd_f32", 1, xs[k], C * HW, one[0], one[1], one[2], one[3], None, 0, ys[k], C * HW,
                  one[4], one[5], bws.data_ptr(), B, C, HW, 0, 0.1, 1e-5, 0, 0, s)

    record(site, na_fwd, {"na2d": 4 * X + A})
    record(site, na_bwd, {"bwd_q": 4 * X + 2 * A, "bwd_kv": 4 * X + 2 * A})
    ln_fwd(False)(0)
    torch.cuda.synchronize()
    record(site + " no res", ln_fwd(False), {"ln_": 2 * X})
    record(site + " res", ln_fwd(True), {"ln_": 3 * X})
    record(site + " write", ln_bwd(0), {"ln_bwd": 3 * X, "finalize": nws * 4})
    record(site + " accum", ln_bwd(1), {"ln_bwd": 4 * X, "finalize": nws * 4})
    record(site, bn_apply, {"bn_group_apply": 2 * X})
    del qkv, x, dy, y, attn, dattn, dqkv
    torch.cuda.empty_cache()

lines = [f"{'site':<22}{'kernel':<46}{'n':>4}{'median us':>11}{'min':>9}{'max':>9}{'MB':>9}{'GB/s':>9}"]
for r in rows:
    lines.append(f"{r[0]:<22}{r[1][:44]:<46}{r[2]:>4}{r[3]:>11.1f}{r[4]:>9.1f}{r[5]:>9.1f}{r[6]:>9.1f}{r[7]:>9.0f}")
text = "\n".join(lines)
print(text)
if OUT:
    with open(OUT, "w") as f:
        f.write(text + "\n")
