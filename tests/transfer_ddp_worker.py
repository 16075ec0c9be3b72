"""Child process of tests/test_transfer_ddp_gpu.py: one data-parallel rank of the native step with frozen parameters.

    python tests/transfer_ddp_worker.py RANK WORLD PORT OUTDIR HIDDEN B H W STEPS

Every rank drives cuda:0 over gloo (as tests/ddp_worker.py). The mask model is frozen as CultionetLitTransferModel's
finetune="fc" freezes it: only the ``final_*`` heads train. Rank r > 0 starts from different random weights, so the
construction-time broadcast must make the replicas identical. Writes the final state, the losses, the bucket plan and
the store layout (offsets, sizes, trainable mask, in store order) to OUTDIR/rank{r}.pt.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    outdir = sys.argv[4]
    hidden, B, H, W, steps = (int(v) for v in sys.argv[5:10])
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
    for n, p in model.named_parameters():
        p.requires_grad_(n.startswith("final_"))
    lit = lit.to(dev).train()
    comm = GradientAllReduce(world_size=world, bucket_mb=float(os.environ.get("CN_DDP_BUCKET_MB", "0.01")))
    trainer = HipTrainer(lit, gradient_clip_val=1.0, comm=comm)
    losses = []
    for k in range(steps):
        x, y, bdist = S.seeded_batch(B, height=H, width=W, seed=7 + rank + 100 * k, with_mask=True)
        losses.append(trainer.training_step(Data(x=x.to(dev), y=y.to(dev), bdist=bdist.to(dev))).clone())
    torch.cuda.synchronize()
    store = trainer.store
    name_of = {id(p): n for n, p in model.named_parameters()}
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.save({"state": sd, "losses": [float(v.item()) for v in losses], "plan": list(comm._plan),
                "buckets_last_step": comm.buckets_last_step, "offsets": list(store.offsets),
                "sizes": [p.numel() for p in store.params], "mask": list(store.trainable_mask()),
                "names": [name_of[id(p)] for p in store.params], "numel": store.numel},
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
