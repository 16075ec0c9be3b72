"""Two data-parallel ranks of the native step with accumulate_grad_batches=2, against the four single-process
micro-gradients of every optimizer step averaged, clipped (clip_grad_norm_ 1.0) and stepped with AdamW -- what torch DDP
under Lightning computes. Only the last micro-batch of a group communicates (Lightning's no_sync for the others).
Tolerances and process handling of tests/test_transfer_ddp_gpu.py."""
import os
import socket
import subprocess
import sys

import pytest
import torch

import optim_ref as R
from accum_ddp_worker import micro_seed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIDDEN, B, H, W, WORLD, STEPS, ACCUMULATE = 8, 2, 28, 28, 2, 2, 2


def _run_ranks(outdir):
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["GLOO_SOCKET_IFNAME"] = "lo"
    os.makedirs(outdir, exist_ok=True)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "accum_ddp_worker.py"), str(r), str(WORLD),
                               str(port), str(outdir), str(HIDDEN), str(B), str(H), str(W), str(STEPS), str(ACCUMULATE)],
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


def test_two_ranks_accumulating_match_averaged_micro_gradients(tmp_path):
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel, HipTrainer

    got = _run_ranks(tmp_path)
    for g in got:
        # one set of bucket collectives per optimizer step, launched by the group's last micro-batch
        assert g["buckets"] >= 1 and g["collectives"] == [0, g["buckets"]] * STEPS, g["collectives"]
        assert g["step_counts"] == [k + (j == ACCUMULATE - 1) for k in range(STEPS) for j in range(ACCUMULATE)]

    lit = CultionetLitModel(in_channels=3, in_time=12, hidden_channels=HIDDEN, dropout=0.0)
    model = lit.cultionet_model.mask_model
    model.load_state_dict(S.seeded_state_dict(model.state_dict()))
    tr = HipTrainer(lit.to("cuda:0").train(), gradient_clip_val=1.0)
    names = dict(model.named_parameters())
    p_ref = {n: p.detach().double().cpu().clone() for n, p in names.items()}
    m = {n: torch.zeros_like(t) for n, t in p_ref.items()}
    v = {n: torch.zeros_like(t) for n, t in p_ref.items()}
    lr, wd, eps, b1 = 0.01, 1e-3, 1e-4, 0.9
    ref_losses = [[] for _ in range(WORLD)]
    for k in range(STEPS):
        grads = []
        for r in range(WORLD):
            for j in range(ACCUMULATE):
                x, y, bd = S.seeded_batch(B, height=H, width=W, seed=micro_seed(r, k, j), with_mask=True)
                ref_losses[r].append(float(tr.forward_backward(Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())).item()))
                grads.append({n: tr.store.grad_of(p).double().cpu() for n, p in names.items()})
        g = {n: sum(gr[n] for gr in grads) / len(grads) for n in names}
        norm = float(torch.sqrt(sum((t ** 2).sum() for t in g.values())))
        coef = R.clip_coef(norm, 1.0)
        for n in names:
            p_ref[n], m[n], v[n] = R.step("AdamW", p_ref[n], g[n] * coef, m[n], v[n], lr, b1, eps, wd, k + 1)
        with torch.no_grad():  # continue from the reference's weights (refreshed through the version counters)
            for n, p in names.items():
                p.copy_(p_ref[n].float())

    for r in range(WORLD):
        assert max(abs(a - b) for a, b in zip(got[r]["losses"], ref_losses[r])) <= 1e-5, (got[r]["losses"], ref_losses[r])
    worst = 0.0
    for n in names:
        assert torch.equal(got[0]["state"][n], got[1]["state"][n]), n  # replicas bitwise identical
        d = float((got[0]["state"][n].double() - p_ref[n]).abs().max())
        worst = max(worst, d)
        assert d <= 5e-5, (n, d)
    print(f"parameters: max |rank - averaged micro-gradients| = {worst:.2e} (bound 5e-5) over {len(names)} tensors")
