"""Two data-parallel ranks of the native step with frozen parameters (finetune="fc": only the heads train), against two
single-process shards of the same step: their gradients averaged, clip_grad_norm_(1.0) over the trainable parameters,
AdamW -- what torch DDP computes for the reference's transfer model. The bucket plan must never cover a frozen range."""
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN, B, H, W, WORLD, STEPS = 8, 2, 28, 28, 2, 2


def _run_ranks(outdir):
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["GLOO_SOCKET_IFNAME"] = "lo"
    os.makedirs(outdir, exist_ok=True)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "transfer_ddp_worker.py"), str(r), str(WORLD),
                               str(port), str(outdir), str(HIDDEN), str(B), str(H), str(W), str(STEPS)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(WORLD)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("the two ranks timed out")
        outs.append(out.decode(errors="replace"))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return [torch.load(os.path.join(outdir, f"rank{r}.pt"), weights_only=False) for r in range(WORLD)]


def _shard_trainers():
    from cultionet_amd import synthetic as S
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    trainers = []
    for _ in range(WORLD):
        lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=HIDDEN, dropout=0.0)
        model = lit.cultionet_model.mask_model
        model.load_state_dict(S.seeded_state_dict(model.state_dict()))
        for n, p in model.named_parameters():
            p.requires_grad_(n.startswith("final_"))
        trainers.append(HipTrainer(lit.to("cuda:0").train(), gradient_clip_val=1.0))
    return trainers


def test_two_ranks_with_frozen_parameters_match_averaged_shards(tmp_path):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data

    got = _run_ranks(tmp_path)
    # no bucket covers a frozen range; together they cover exactly the trainable slices
    lay = got[0]
    frozen, trainable = set(), set()
    for o, n, t in zip(lay["offsets"], lay["sizes"], lay["mask"]):
        (trainable if t else frozen).update(range(o, o + (n + 3) // 4 * 4))
    assert frozen and trainable
    covered = set()
    for lo, hi, _ in lay["plan"]:
        assert not (set(range(lo, hi)) & frozen), (lo, hi)
        covered.update(range(lo, hi))
    assert covered == trainable
    assert all(g["buckets_last_step"] == len(g["plan"]) for g in got)

    # the reference: two shards from the same weights, averaged gradients, clip over the trainable ones, AdamW
    trainers = _shard_trainers()
    model0 = trainers[0].model
    names = dict(model0.named_parameters())
    train_names = [n for n, p in names.items() if p.requires_grad]
    p_ref = {n: names[n].detach().double().cpu().clone() for n in train_names}
    frozen0 = {n: p.detach().cpu().clone() for n, p in names.items() if not p.requires_grad}
    m = {n: torch.zeros_like(v) for n, v in p_ref.items()}
    v = {n: torch.zeros_like(t) for n, t in p_ref.items()}
    lr, wd, eps, b1, b2 = 0.01, 1e-3, 1e-4, 0.9, 0.98
    ref_losses = [[] for _ in range(WORLD)]
    for k in range(STEPS):
        grads = []
        for r, tr in enumerate(trainers):
            x, y, bd = S.seeded_batch(B, height=H, width=W, seed=7 + r + 100 * k, with_mask=True)
            ref_losses[r].append(float(tr.forward_backward(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())).item()))
            mp = dict(tr.model.named_parameters())
            grads.append({n: tr.store.grad_of(mp[n]).double().cpu() for n in train_names})
        g = {n: sum(gr[n] for gr in grads) / WORLD for n in train_names}
        norm = math.sqrt(sum(float((t ** 2).sum()) for t in g.values()))
        coef = min(1.0, 1.0 / (norm + 1e-6))
        step = k + 1
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        for n in train_names:
            gi = g[n] * coef
            p_ref[n] = p_ref[n] * (1.0 - lr * wd)
            m[n] = b1 * m[n] + (1.0 - b1) * gi
            v[n] = b2 * v[n] + (1.0 - b2) * gi * gi
            p_ref[n] = p_ref[n] - (lr / bc1) * m[n] / (v[n].sqrt() / math.sqrt(bc2) + eps)
        with torch.no_grad():  # both shards continue from the reference's weights (refreshed through the version counters)
            for tr in trainers:
                mp = dict(tr.model.named_parameters())
                for n in train_names:
                    mp[n].copy_(p_ref[n].float())

    for r in range(WORLD):
        assert max(abs(a - b) for a, b in zip(got[r]["losses"], ref_losses[r])) <= 1e-5, (got[r]["losses"], ref_losses[r])
    for n in names:
        assert torch.equal(got[0]["state"][n], got[1]["state"][n]), n  # replicas bitwise identical
    for n, t in frozen0.items():
        assert torch.equal(got[0]["state"][n], t), n  # frozen: rank 0's initial weights, on both ranks
    worst = 0.0
    for n in train_names:
        d = float((got[0]["state"][n].double() - p_ref[n]).abs().max())
        worst = max(worst, d)
        assert d <= 5e-5, (n, d)
    print(f"trainable parameters: max |rank - averaged shards| = {worst:.2e} over {len(train_names)} tensors")
