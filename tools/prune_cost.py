#!/usr/bin/env python
"""What global magnitude pruning costs at the benchmarked fp32 point (hidden 32, batch 8, 100 x 100, 12 time steps).

    python tools/prune_cost.py [--out profiles/prune_cost.txt] [--iters 2000] [--repeats 7] [--steps 20]

Three measurements, all in one process on one build:
  * the two mask passes a step with a pruner adds (cn_mask_select_f32 in place over the flat gradient, then over the flat
    parameters) against the yardstick, cn_adamw_step_f32 over buffers of the same length (28 B per element; a mask pass
    moves 9 B per element, so by bytes the two together are 18 / 28 of it), and cn_grad_sumsq_f32 for scale;
  * the selection, cn_prune_magnitude_u8 (3 histogram + pick launches, tie count, scan, commit) at amount 0.3 on the
    model's own weights; every call starts from fresh flags, restored by a device copy of the byte array inside the
    window, which is timed alone and reported beside it;
  * the training step (HipTrainer.training_step, AdamW, norm clipping) without a pruner and with one at 30 % sparsity, two
    trainers alternating inside every repeat, host clock between two device synchronisations over ``--steps`` steps.
Kernel figures: the time between two HIP events around ``--iters`` back-to-back calls on one stream, divided by the
calls, alternated inside every repeat, after untimed warm-up calls; median (min-max) over the repeats. Back-to-back calls
over 42 MB buffers stay in the 256 MB last-level cache, the yardstick's included: the kernel figures are warm-cache
figures and their ratio is what they are for; what a step pays after a forward and backward pass is the third measurement."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIDDEN, BATCH, SIZE, AMOUNT = 32, 8, 100, 0.3


def _fmt(values, unit):
    return f"{statistics.median(values):9.2f} ({min(values):.2f}-{max(values):.2f}) {unit}"


def main():
    import cultionet_amd

    cultionet_amd.configure_runtime()
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/prune_cost.py measures on the GPU: no device found")
    from cultionet_amd import _lib
    from cultionet_amd import engine as E
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer
    from cultionet_amd.pruning import MagnitudePruner

    def lit():
        m = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=HIDDEN, dropout=0.0, lr_scheduler="StepLR",
                              steplr_step_size=1000)
        mm = m.cultionet_model.mask_model
        mm.load_state_dict(S.seeded_state_dict(mm.state_dict()))
        return m.to("cuda:0").train()

    plain_lit, pruned_lit = lit(), lit()
    plain = HipTrainer(plain_lit, steps_per_epoch=1)
    pruner = MagnitudePruner(pruned_lit)
    pruned = HipTrainer(pruned_lit, steps_per_epoch=1, pruner=pruner)
    store, n = pruned.store, pruned.store.numel
    x, y, bd = S.seeded_batch(BATCH, height=SIZE, width=SIZE, seed=3, with_mask=True)
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    for tr in (plain, pruned):
        for _ in range(3):
            tr.training_step(batch)
    weights = store.flat.clone()  # what the selection is timed on: the weights before this round zeroes 30 % of them
    k = pruned.prune(AMOUNT)
    torch.cuda.synchronize()
    lines = [f"global magnitude pruning at hidden {HIDDEN}, batch {BATCH}, {SIZE} x {SIZE}, fp32: {n} flat elements, "
             f"{pruner.total} prunable, {k} pruned (amount {AMOUNT}); {args.repeats} repeats, median (min-max)"]

    # ---- kernels over buffers of the store's length (copies: the trainers' state is not touched) ----
    s = E._stream()
    p, g, m, v = (store.flat.clone(), store.flat_grad.clone(), pruned.opt.exp_avg.clone(), pruned.opt.exp_avg_sq.clone())
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    flags = pruner.flags
    fresh = torch.where((flags & 2) != 0, torch.full_like(flags, 3), flags)
    work = fresh.clone()
    ws = torch.zeros_like(pruner._ws)
    kernels = {
        "mask gradient (cn_mask_select_f32, in place)":
            lambda: _lib.call("cn_mask_select_f32", g.data_ptr(), g.data_ptr(), flags.data_ptr(), n, s),
        "mask parameters (cn_mask_select_f32, in place)":
            lambda: _lib.call("cn_mask_select_f32", p.data_ptr(), p.data_ptr(), flags.data_ptr(), n, s),
        "cn_adamw_step_f32 (yardstick)":
            lambda: _lib.call("cn_adamw_step_f32", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0.0, 0.9, 0.98,
                              1e-4, 0.0, 10, 1.0, sumsq.data_ptr(), 1.0, s),
        "cn_grad_sumsq_f32":
            lambda: _lib.call("cn_grad_sumsq_f32", g.data_ptr(), n, sumsq.data_ptr(), s),
        "flags restore (device copy, 1 B per element)":
            lambda: work.copy_(fresh),
    }

    def select():
        work.copy_(fresh)
        _lib.call("cn_prune_magnitude_u8", weights.data_ptr(), work.data_ptr(), n, round(AMOUNT * pruner.total),
                  ws.data_ptr(), ws.numel(), s)

    kernels["selection + flags restore (cn_prune_magnitude_u8, 9 launches)"] = select

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    for fn in kernels.values():
        for _ in range(10):
            fn()
    times = {name: [] for name in kernels}
    for _ in range(args.repeats):
        for name, fn in kernels.items():
            times[name].append(window(fn))
    for name, vals in times.items():
        lines.append(f"{name:<68}{_fmt(vals, 'us')}")
    med = {name: statistics.median(vals) for name, vals in times.items()}
    names = list(kernels)
    both = med[names[0]] + med[names[1]]
    lines.append(f"two mask passes / cn_adamw_step_f32: {both / med[names[2]]:.3f} (by bytes 18 / 28 = 0.643; accepted up to 1)")
    lines.append(f"selection alone (median minus the restore): {med[names[5]] - med[names[4]]:.2f} us, once per epoch")

    # ---- the step with and without a pruner ----
    def steps(tr):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tr.training_step(batch)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    step_ms = {"without a pruner": [], "with a pruner": []}
    for _ in range(args.repeats):
        step_ms["without a pruner"].append(steps(plain))
        step_ms["with a pruner"].append(steps(pruned))
    for name, vals in step_ms.items():
        lines.append(f"{'training step ' + name:<68}{_fmt(vals, 'ms')}")
    assert pruner.count_alive() == pruner.alive
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
