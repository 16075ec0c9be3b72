"""Child process of tests/test_accum_ddp_gpu.py: one data-parallel rank of the native step with gradient accumulation.

    python tests/accum_ddp_worker.py RANK WORLD PORT OUTDIR HIDDEN B H W STEPS ACCUMULATE

Every rank drives cuda:0 over gloo (as tests/ddp_worker.py). Rank r > 0 starts from different random weights, so the
construction-time broadcast must make the replicas identical. Writes the final state, the losses of every micro-batch
and the number of collectives each micro-batch launched to OUTDIR/rank{r}.pt.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def micro_seed(rank, step, micro):
    return 7 + rank + 10 * micro + 100 * step


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    outdir = sys.argv[4]
    hidden, B, H, W, steps, accumulate = (int(v) for v in sys.argv[5:11])
    import torch
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.ddp import GradientAllReduce
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    dev = "cuda:0"
    torch.manual_seed(1234 + rank)
    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=hidden, dropout=0.0)
    model = lit.cultionet_model.mask_model
    if rank == 0:
        model.load_state_dict(S.seeded_state_dict(model.state_dict()))
    lit = lit.to(dev).train()
    comm = GradientAllReduce(world_size=world, bucket_mb=float(os.environ.get("CN_DDP_BUCKET_MB", "0.05")))
    launched = [0]
    launch = comm._launch

    def counting(*args, **kw):
        launched[0] += 1
        return launch(*args, **kw)

    comm._launch = counting
    trainer = HipTrainer(lit, gradient_clip_val=1.0, comm=comm, accumulate_grad_batches=accumulate)
    losses, collectives, step_counts = [], [], []
    for k in range(steps):
        for j in range(accumulate):
            x, y, bdist = S.seeded_batch(B, height=H, width=W, seed=micro_seed(rank, k, j), with_mask=True)
            before = launched[0]
            losses.append(trainer.training_step(Data(x=x.to(dev), y=y.to(dev), bdist=bdist.to(dev))).clone())
            collectives.append(launched[0] - before)
            step_counts.append(trainer.step_count)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.save({"state": sd, "losses": [float(v.item()) for v in losses], "collectives": collectives,
                "step_counts": step_counts, "buckets": len(comm._plan)}, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
