"""Cost of the optimizer kernels and of gradient accumulation at hidden 32 / batch 8 fp32.

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/optimizer_cost.py      # kernel averages, one trace
    python tools/optimizer_cost.py --accumulate                                    # step time per micro-batch

Ten native steps with each optimizer of the reference's command line, in one process, so that cn_adamw_kernel (AdamW,
Adam) and the cn_optim_kernel instances (RAdam, SGD) land in the same trace. With --accumulate: the wall time of a
micro-batch with accumulate_grad_batches=4 against the plain step (device-synchronised, 40 micro-batches each).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _trainer(optimizer, **kw):
    from cultionet_amd import synthetic as S
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=32, dropout=0.0, optimizer=optimizer)
    m = lit.cultionet_model.mask_model
    m.load_state_dict(S.seeded_state_dict(m.state_dict()))
    return HipTrainer(lit.to("cuda:0").train(), **kw)


def main():
    import cultionet_amd

    cultionet_amd.configure_runtime()
    import torch

    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data

    ap = argparse.ArgumentParser()
    ap.add_argument("--accumulate", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    x, y, bd = S.seeded_batch(8, height=100, width=100, seed=3, with_mask=True)
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    if not args.accumulate:
        for name in ("AdamW", "Adam", "RAdam", "SGD"):
            tr = _trainer(name)
            for _ in range(args.steps):
                tr.training_step(batch)
            torch.cuda.synchronize()
            print(json.dumps({"optimizer": name, "steps": args.steps, "numel": tr.store.numel}))
        return
    out = {}
    for k in (1, 4):
        tr = _trainer("AdamW", accumulate_grad_batches=k)
        for _ in range(8):
            tr.training_step(batch)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(40):
            tr.training_step(batch)
        torch.cuda.synchronize()
        out[f"accumulate_{k}_ms_per_micro_batch"] = round((time.perf_counter() - t0) / 40 * 1e3, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
