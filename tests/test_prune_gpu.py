"""Global magnitude pruning on the device (csrc/cn_prune.hip, cultionet_amd.pruning): the selection and the masked copy
against tests/prune_ref.py for exact equality, the masked optimizer step against torch.nn.utils.prune + torch.optim.AdamW,
and HipTrainer / NativePruning end to end at hidden 8, batch 2, 28 x 28 (the shapes of tests/test_optim_train_gpu.py)."""
import copy
import types

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils import prune

import prune_ref as R
from test_loss_optim_gpu import F32_EPS, GRAD_REL
from test_optim_train_gpu import CONSTANT, KW, TOL, _batches, _torch_side

pytestmark = pytest.mark.gpu

CHUNK = 2048  # CN_PRUNE_CHUNK: flat elements per chunk of the ordered tie-break


# ---- kernel level: a synthetic store -----------------------------------------------------------------------------------

class _Leaf(nn.Module):
    def __init__(self, nw, nb, extra=0):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(nw))
        if nb:
            self.bias = nn.Parameter(torch.zeros(nb))
        if extra:
            self.gamma = nn.Parameter(torch.zeros(extra))  # not named weight / bias: never pruned


class _Synthetic(nn.Module):
    """~3e5 elements in odd-sized tensors: slices start at offsets that are no multiple of 32, padding exists, four
    tensors are longer than a chunk, and a histogram pass takes several blocks (65536 elements each)."""

    SIZES = [(5, 3, 0), (70001, 33, 1), (1, 0, 0), (100003, 7, 1001), (4097, 1, 0), (130001, 129, 3)]

    def __init__(self):
        super().__init__()
        self.leaves = nn.ModuleList([_Leaf(*s) for s in self.SIZES])


@pytest.fixture(scope="module")
def synthetic():
    from cultionet_amd import engine as E
    from cultionet_amd.pruning import MagnitudePruner

    net = _Synthetic().to("cuda:0")
    store = E.ParamStore(net)
    pruner = MagnitudePruner(net, store=store)
    flags0 = pruner.flags.cpu().numpy().copy()
    assert store.numel > 4 * 65536 and pruner.total == sum(w + b for w, b, _ in _Synthetic.SIZES)
    assert int((flags0 == 0).sum()) > 1005 and any(o % 32 for o in store.offsets)  # gamma + padding
    return store, pruner, flags0


def _bits(n, gen, lo, hi):
    return gen.integers(lo, hi, size=n, dtype=np.uint32)


def _values(kind, n, flags0):
    """float32 [n] for the whole flat buffer, padding and non-prunable elements included (tiny values there: they would
    be the first to go if they took part)."""
    gen = np.random.default_rng(sum(map(ord, kind)))
    sign = (gen.integers(0, 2, size=n, dtype=np.uint32) << np.uint32(31))
    if kind == "normal":
        v = gen.standard_normal(n).astype(np.float32) * np.float32(0.02)
    elif kind == "one_exponent":  # [1, 2): the first pass lands in eight adjacent bins
        v = (_bits(n, gen, 0x3F800000, 0x40000000)).view(np.float32)
    elif kind == "denormals_and_zeros":
        b = _bits(n, gen, 1, 0x00800000)
        b[gen.random(n) < 0.3] = 0
        v = (b | sign).view(np.float32)
    elif kind == "negative":
        v = -np.abs(gen.standard_normal(n).astype(np.float32)) - np.float32(1e-3)
    elif kind == "tie_block":  # 7000 entries at the 0.3 quantile, 5000 of them adjacent: across two chunk boundaries
        v = gen.standard_normal(n).astype(np.float32)
        q = np.float32(np.quantile(np.abs(v[flags0 == 3]), 0.3))
        start = 3 * CHUNK - 1234
        v[start:start + 5000] = q
        outside = np.nonzero(flags0 == 3)[0]
        scattered = gen.choice(outside[(outside < start) | (outside >= start + 5000)], 2000, replace=False)
        v[scattered] = np.where(gen.random(2000) < 0.5, q, -q)
    elif kind == "all_equal":
        v = (np.full(n, 0x3FC00000, dtype=np.uint32) | sign).view(np.float32)  # +-1.5
    else:
        raise KeyError(kind)
    v = v.copy()
    v[flags0 != 3] = np.float32(1e-30) if kind != "denormals_and_zeros" else np.float32(0.0)
    return v


def _rounds(store, pruner, flags0, flat0, ks):
    """Run ``ks`` through MagnitudePruner.prune on fresh flags; after every round the device flags and the flat buffer
    equal the restated rule's, byte for byte. ``ks`` entries: an int, a float, or a callable of the alive count."""
    flat_ref, flags_ref = flat0.copy(), flags0.copy()
    store.flat.copy_(torch.from_numpy(flat0))
    pruner.flags.copy_(torch.from_numpy(flags0))
    pruner.alive = pruner.total
    seen = []
    for amount in ks:
        if callable(amount):
            amount = amount(pruner.alive)
        alive = int((flags_ref == 3).sum())
        k = R.round_count(amount, alive)
        version = store.version
        assert pruner.prune(amount) == k and pruner.alive == alive - k
        assert store.version == version + (1 if k else 0)
        flags_ref = R.prune_round(flat_ref, flags_ref, k)
        flat_ref = R.masked(flat_ref, flags_ref)
        torch.cuda.synchronize()
        got_flags, got_flat = pruner.flags.cpu().numpy(), store.flat.cpu().numpy()
        assert (got_flags == flags_ref).all(), (amount, int((got_flags != flags_ref).sum()))
        assert (got_flat.view(np.uint32) == flat_ref.view(np.uint32)).all(), amount
        keep = flags0 != 3  # padding and non-prunable elements: flags and values as they were
        assert (got_flags[keep] == flags0[keep]).all() and (got_flat[keep].view(np.uint32) == flat0[keep].view(np.uint32)).all()
        assert pruner.count_alive() == pruner.alive and abs(pruner.sparsity(sync=True) - pruner.sparsity()) == 0.0
        seen.append(got_flags)
    return seen


KINDS = ["normal", "one_exponent", "denormals_and_zeros", "negative", "tie_block", "all_equal"]


@pytest.mark.parametrize("kind", KINDS)
def test_selection_equals_the_restated_rule(synthetic, kind):
    store, pruner, flags0 = synthetic
    flat0 = _values(kind, store.numel, flags0)
    if kind == "tie_block":  # the first float round's threshold falls inside the block of equal values
        key = R.keys(flat0[flags0 == 3])
        q = R.keys(flat0[3 * CHUNK:3 * CHUNK + 1])[0]
        k1 = round(0.3 * pruner.total)
        assert int((key < q).sum()) < k1 < int((key <= q).sum()) and int((key == q).sum()) >= 7000
    # 0, 1, three float rounds, then all but one of what is left, then the last one
    chain = [0, 1, 0.3, 0.3, 0.3, lambda alive: alive - 1, 1]
    first = _rounds(store, pruner, flags0, flat0, chain)
    assert pruner.alive == 0 and (first[-1][flags0 == 3] == R.PRUNABLE).all()
    again = _rounds(store, pruner, flags0, flat0, chain)
    assert all((a == b).all() for a, b in zip(first, again))  # two runs: byte-identical flags
    _rounds(store, pruner, flags0, flat0, [lambda alive: alive - 1])
    _rounds(store, pruner, flags0, flat0, [lambda alive: alive])
    _rounds(store, pruner, flags0, flat0, [1.0])
    with pytest.raises(ValueError):
        pruner.prune(1)  # nothing left


@pytest.mark.parametrize("n", [1, 3, 2049, 3 * 65536 + 4 * 500 + 1])  # n % 4 = 1 or 3: tail only; one chunk + 1; three blocks
def test_selection_on_a_bare_buffer_of_any_length(n):
    """cn_prune_magnitude_u8 as the C ABI takes it: n no multiple of 4 (the one-element-per-thread tail of the histogram
    pass, a last chunk of one element), random flags of all four kinds, values drawn from 64 levels so that every round
    ends in ties."""
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    gen = np.random.default_rng(n)
    flags = gen.integers(0, 4, size=n, dtype=np.uint8)
    flags[-1] = 3  # the last element takes part
    w = (gen.integers(0, 64, size=n) / 64.0).astype(np.float32) * np.where(gen.random(n) < 0.5, -1, 1).astype(np.float32)
    wd, fd = torch.from_numpy(w).cuda(), torch.from_numpy(flags).cuda()
    words = _lib.query("cn_prune_workspace_words", n)
    ws = torch.zeros(words, dtype=torch.int32, device="cuda")
    ref = flags.copy()
    while int((ref == 3).sum()):
        alive = int((ref == 3).sum())
        k = max(1, round(0.4 * alive))
        _lib.call("cn_prune_magnitude_u8", wd.data_ptr(), fd.data_ptr(), n, k, ws.data_ptr(), words, E._stream())
        ref = R.prune_round(w, ref, k)
        assert (fd.cpu().numpy() == ref).all(), (n, alive, k)
    assert (wd.cpu().numpy().view(np.uint32) == w.view(np.uint32)).all()  # the weights are only read


def test_selection_refuses_bad_arguments(synthetic):
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    store, pruner, _ = synthetic
    lib, s = _lib.load(), E._stream()
    w, f, ws, n = store.flat.data_ptr(), pruner.flags.data_ptr(), pruner._ws.data_ptr(), store.numel
    words = pruner._ws.numel()
    assert words == _lib.query("cn_prune_workspace_words", n) == 8 + 2048 + (n + CHUNK - 1) // CHUNK
    assert lib.cn_prune_magnitude_u8(w, f, n, 0, ws, words, s) == -1          # k = 0 is the host's no-op
    assert lib.cn_prune_magnitude_u8(w, f, n, n + 1, ws, words, s) == -1
    assert lib.cn_prune_magnitude_u8(w, f, n, 1, ws, words - 1, s) == -1      # workspace too small
    assert lib.cn_prune_magnitude_u8(w + 4, f, n - 4, 1, ws, words, s) == -1  # w not 16-byte aligned
    assert lib.cn_prune_magnitude_u8(w, f + 1, n - 4, 1, ws, words, s) == -1  # flags not 4-byte aligned
    assert lib.cn_prune_magnitude_u8(w, f, 1 << 31, 1, ws, words, s) == -1
    assert lib.cn_mask_select_f32(w + 4, w, f, n - 4, s) == -1
    assert lib.cn_prune_reset_f32(w, w, f, n, s) == -1
    assert lib.cn_prune_count_u32(f + 2, n - 4, ws, s) == -1


@pytest.mark.parametrize("n", [3, 10007, 4096 * 1024 + 4 * 300 + 2])  # tail only; odd; past the 4096-block grid cap
def test_mask_select_and_reset_are_exact(n):
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    gen = np.random.default_rng(n)
    flags = gen.integers(0, 4, size=n, dtype=np.uint8)
    src = gen.standard_normal(n).astype(np.float32)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1e-42], dtype=np.float32)
    where = gen.random(n) < 0.2
    src[where] = special[gen.integers(0, special.size, size=int(where.sum()))]
    own = gen.standard_normal(n).astype(np.float32)
    own[gen.random(n) < 0.1] = np.nan
    assert np.isnan(src[(flags & 3) == 2]).any() or n < 100  # a pruned NaN is among the inputs
    fd, sd = torch.from_numpy(flags).cuda(), torch.from_numpy(src).cuda()
    want = R.masked(src, flags).view(np.uint32)
    s = E._stream()
    out = torch.from_numpy(own).cuda()
    _lib.call("cn_mask_select_f32", out.data_ptr(), sd.data_ptr(), fd.data_ptr(), n, s)  # out of place
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert (sd.cpu().numpy().view(np.uint32) == src.view(np.uint32)).all()
    inplace = sd.clone()
    _lib.call("cn_mask_select_f32", inplace.data_ptr(), inplace.data_ptr(), fd.data_ptr(), n, s)
    assert (inplace.cpu().numpy().view(np.uint32) == want).all()
    # lottery-ticket reset: prunable ? (alive ? snapshot : +0.0) : own
    p = torch.from_numpy(own).cuda()
    _lib.call("cn_prune_reset_f32", p.data_ptr(), sd.data_ptr(), fd.data_ptr(), n, s)
    reset = np.where((flags & 2) != 0, np.where((flags & 1) != 0, src.view(np.uint32), np.uint32(0)), own.view(np.uint32))
    assert (p.cpu().numpy().view(np.uint32) == reset).all()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.call("cn_prune_count_u32", fd.data_ptr(), n, count.data_ptr(), s)
    assert int(count.item()) == int(((flags & 3) == 3).sum())


# ---- against torch.nn.utils.prune + torch.optim.AdamW + clip_grad_norm_ -------------------------------------------------

class _Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 7, 3)
        self.bn = nn.BatchNorm2d(7)
        self.seq = nn.Sequential(nn.Linear(7, 33), nn.ReLU(), nn.Linear(33, 5, bias=False))
        self.gate = _Leaf(9, 0, extra=1)


def test_masked_step_matches_torch_prune_and_adamw():
    """Three AdamW steps with norm clipping on hand-written gradients, a prune of 30 % after the first. The torch side runs
    in float64 on the CPU: prune.global_unstructured re-parametrises it, its gradients reach ``*_orig`` through autograd
    (loss = sum of effective parameter * G), clip_grad_norm_ sees them masked. At the prune the torch side takes the
    native weights (widened), so both select on the same values and torch's unspecified tie order never matters (|w|
    distinct, asserted). Kept entries: the bound of tests/test_loss_optim_gpu.py as it stands (GRAD_REL of the step's
    max|dp| plus two ulps of p) against the torch trajectory; pruned entries exactly zero; opt.sumsq: that file's 1e-12."""
    from cultionet_amd import engine as E
    from cultionet_amd.optim import NativeOptimizer
    from cultionet_amd.pruning import MagnitudePruner, prunable_parameters

    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731  (torch gets the values the kernel receives)
    hyper = dict(lr=f32(0.01), betas=(f32(0.9), f32(0.98)), eps=f32(1e-4), weight_decay=f32(1e-3))
    torch.manual_seed(21)
    ref = _Small().double()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn_like(p).float().double() * 0.05)
    net = copy.deepcopy(ref).float().to("cuda:0")
    store = E.ParamStore(net)
    pruner = MagnitudePruner(net, store=store)
    opt = NativeOptimizer(list(net.parameters()), store, "AdamW", **hyper)
    opt.pruner = pruner
    names = [n for n, _ in net.named_parameters()]
    gen = torch.Generator().manual_seed(22)
    grads = [{n: torch.randn(p.shape, generator=gen) * 0.5 for n, p in net.named_parameters()} for _ in range(3)]
    pairs = [(ref.get_submodule(m), n) for m, n, _ in prunable_parameters(ref)]
    ref_opt = torch.optim.AdamW(ref.parameters(), **hyper)  # (pruning keeps the Parameter objects, renamed *_orig)
    all_on = tuple(True for _ in store.params)

    def effective(name):  # the tensor a forward of the torch model reads, recomputed by torch's own pre-hooks
        mod_name, _, leaf = name.rpartition(".")
        mod = ref.get_submodule(mod_name)
        for hook in mod._forward_pre_hooks.values():
            hook(mod, None)
        return getattr(mod, leaf)

    for step in range(3):
        ref_opt.zero_grad(set_to_none=True)
        sum((effective(n) * grads[step][n].double()).sum() for n in names).backward()
        kept_sq = sum(float((p.grad ** 2).sum()) for p in ref.parameters())
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 1.0)
        before = {n: effective(n).detach().clone() for n in names}
        ref_opt.step()
        store.zero_grad()
        for n, p in net.named_parameters():
            store.grad_of(p).copy_(grads[step][n])
        opt.step_flat(store.flat_grad.data_ptr(), all_on, hyper["lr"], *hyper["betas"], hyper["eps"],
                      hyper["weight_decay"], 1.0, 1.0, "norm")
        torch.cuda.synchronize()
        assert abs(float(opt.sumsq.item()) - kept_sq) <= 1e-12 * kept_sq, (step, float(opt.sumsq.item()), kept_sq)
        worst = 0.0
        for n, p in net.named_parameters():
            want, got = effective(n).detach(), p.detach().cpu().double()
            keep = pruner.keep_mask(p).cpu()
            assert keep.shape == p.shape and (got[~keep] == 0).all() and (want[~keep] == 0).all(), n
            dp = float((want - before[n]).abs().max())
            err = float(((got - want).abs() - 2 * F32_EPS * want.abs()).clamp(min=0).max())
            worst = max(worst, err / (GRAD_REL * dp))
            assert err <= GRAD_REL * dp, (step, n, err, dp)
        print(f"masked AdamW step {step + 1}: worst err/bound {worst:.3f}")
        if step == 0:
            with torch.no_grad():  # both sides select on the same values
                for (n, p), q in zip(net.named_parameters(), ref.parameters()):
                    q.copy_(p.detach().cpu().double())
            mags = torch.cat([getattr(m, n).detach().abs().flatten() for m, n in pairs])
            assert mags.unique().numel() == mags.numel()
            prune.global_unstructured(pairs, pruning_method=prune.L1Unstructured, amount=0.3)
            assert pruner.prune(0.3) == round(0.3 * mags.numel())
            torch.cuda.synchronize()
            for n, p in net.named_parameters():
                mod_name, _, leaf = n.rpartition(".")
                mask = getattr(ref.get_submodule(mod_name), leaf + "_mask", None)
                keep = pruner.keep_mask(p).cpu()
                assert keep.all() if mask is None else torch.equal(keep, mask != 0), n
            assert pruner.count_alive() == pruner.alive == mags.numel() - round(0.3 * mags.numel())


# ---- end to end: HipTrainer ---------------------------------------------------------------------------------------------

def _lit():
    from cultionet_amd import synthetic as S
    from cultionet_amd.lightning import CultionetLitModel

    lit = CultionetLitModel(**KW, optimizer="AdamW", **CONSTANT)
    mm = lit.cultionet_model.mask_model
    mm.load_state_dict(S.seeded_state_dict(mm.state_dict()))
    return lit.to("cuda:0").train()


def _pruned(pruner):
    return (pruner.flags & 3) == 2


def _mask_holds(trainer, what):
    torch.cuda.synchronize()
    pr = trainer.pruner
    flat_bits = trainer.store.flat.view(torch.int32)
    assert int((flat_bits[_pruned(pr)] != 0).sum()) == 0, what  # exactly +0.0
    assert pr.count_alive() == pr.alive, what


def _pruned_run(precision, replay, batches):
    """Two steps, prune(0.5), three steps; the mask holds after every step. Returns (lit, trainer, flat before the prune)."""
    from cultionet_amd.lightning import HipTrainer
    from cultionet_amd.pruning import MagnitudePruner

    lit = _lit()
    trainer = HipTrainer(lit, precision=precision, replay=replay, steps_per_epoch=1, pruner=MagnitudePruner(lit))
    pr = trainer.pruner
    assert pr.store is trainer.store and pr.alive == pr.total and pr.sparsity() == 0.0
    for k in range(2):
        trainer.training_step(batches[k % 3])
        _mask_holds(trainer, f"step {k + 1}")
    at_prune = trainer.store.flat.clone()
    assert trainer.prune(0.5) == round(0.5 * pr.total)
    assert pr.alive == pr.total - round(0.5 * pr.total) and abs(pr.sparsity() - 0.5) < 1e-6
    _mask_holds(trainer, "prune")
    for k in range(2, 5):
        trainer.training_step(batches[k % 3])
        _mask_holds(trainer, f"step {k + 1}")
    if replay:
        assert trainer._plan is not None  # steps 3.. ran from (or recorded) the plan
    return lit, trainer, at_prune


@pytest.mark.parametrize("precision", ["32-true", "bf16-mixed"])
def test_trainer_keeps_the_mask_and_replay_follows_eager(precision):
    """HipTrainer(pruner=...) eager and under replay=True. The first three steps of both runs are eager, so at the prune
    they differ by the summation order of float atomics alone; an entry can then be pruned in one run and kept in the
    other only if its magnitude is within the trajectory tolerance of the threshold. So: wherever the masks agree the
    parameters agree within the bounds of tests/test_optim_train_gpu.py (fp32: TOL relative to max(1, max|p|); bf16:
    0.05 absolute), and wherever they differ, | |w| - threshold | at the prune is within twice that tolerance. The
    number of such entries is capped by what the eager run itself holds that close to the threshold at the prune --
    within TOL in fp32, within 1e-3 in bf16 (the loss bound that file gives the bf16 trajectory; 0.05 would span every
    weight) -- and by 1 % of the prunable entries: a selection that ignored the magnitudes would differ at half."""
    from cultionet_amd import synthetic as S
    from cultionet_amd.data import Data
    from cultionet_amd.lightning import CultionetLitModel

    batches = _batches(3)
    lit_e, eager, w_e = _pruned_run(precision, False, batches)
    lit_r, replayed, _ = _pruned_run(precision, True, batches)
    pe, pr_ = _pruned(eager.pruner), _pruned(replayed.pruner)
    prunable = (eager.pruner.flags & 2) != 0
    assert int(pe.sum()) == int(pr_.sum()) == round(0.5 * eager.pruner.total)
    fe, fr = eager.store.flat, replayed.store.flat
    tol = TOL * max(1.0, float(fe.abs().max())) if precision == "32-true" else 0.05
    agree = pe == pr_
    err = float((fe - fr)[agree].abs().max())
    threshold = float(w_e[pe].abs().max())
    off = float((w_e[~agree].abs() - threshold).abs().max()) if int((~agree).sum()) else 0.0
    print(f"pruned run {precision}: replay-vs-eager err/tol {err / tol:.3f}, masks differ at {int((~agree).sum())} entries "
          f"(|w| - threshold there: {off:.3e}), threshold {threshold:.3e}")
    assert err <= tol and off <= 2 * tol
    near = tol if precision == "32-true" else 1e-3
    band = int(((w_e.abs() - threshold).abs()[prunable] <= near).sum())
    assert int((~agree).sum()) <= min(band, eager.pruner.total // 100), (int((~agree).sum()), band)
    assert int((pe & ~prunable).sum()) == 0
    # a second model loaded with the masked weights gives the same eval forward, bit for bit: the packs hold the masked values
    fresh = CultionetLitModel(**KW, optimizer="AdamW", **CONSTANT).to("cuda:0")
    fresh.load_state_dict(copy.deepcopy(lit_e.state_dict()))
    fresh.hip_precision = lit_e.hip_precision = precision
    x, y, bd = S.seeded_batch(2, height=28, width=28, seed=99)
    batch = Data(x=x.cuda(), y=y.cuda(), bdist=bd.cuda())
    with torch.no_grad():
        a, b = lit_e.eval()(batch), fresh.eval()(batch)
    for key in ("distance", "edge", "crop"):
        assert torch.equal(a[key], b[key]), key


def test_trainer_without_a_pruner_launches_what_it_did(monkeypatch):
    from cultionet_amd import _lib
    from cultionet_amd.lightning import HipTrainer
    from cultionet_amd.pruning import MagnitudePruner

    bt = _batches(1)[0]
    seen, call = [], _lib.call
    for with_pruner in (False, True):
        lit = _lit()
        trainer = HipTrainer(lit, steps_per_epoch=1, pruner=MagnitudePruner(lit) if with_pruner else None)
        assert trainer.opt.pruner is trainer.pruner and (trainer.pruner is not None) == with_pruner
        assert ("pruner" in trainer.state_dict()) == with_pruner
        trainer.forward_backward(bt)
        names = []
        monkeypatch.setattr(_lib, "call", lambda name, *a, _n=names: (_n.append(name), call(name, *a))[1])
        trainer.optimizer_step()
        monkeypatch.undo()
        seen.append(names)
    assert seen[0] == ["cn_grad_sumsq_f32", "cn_adamw_step_f32"]
    assert seen[1] == ["cn_mask_select_f32", "cn_grad_sumsq_f32", "cn_adamw_step_f32", "cn_mask_select_f32"]
    with pytest.raises(RuntimeError, match="without a pruner"):
        HipTrainer(_lit()).prune(0.1)


def test_state_dict_round_trip_continues_the_run():
    """Two steps, prune, one step, state_dict(); two more steps -> A. A fresh model and trainer loaded from the module's
    and the trainer's state at that point, the same two steps -> B. The same flags, pruned entries exactly zero in both,
    parameters within TOL of tests/test_optim_train_gpu.py (the gradient atomics are not ordered: two runs of A differ)."""
    from cultionet_amd.lightning import HipTrainer
    from cultionet_amd.pruning import MagnitudePruner

    batches = _batches(3)
    lit_a = _lit()
    tr_a = HipTrainer(lit_a, steps_per_epoch=1, pruner=MagnitudePruner(lit_a, lottery_ticket=True))
    for k in range(2):
        tr_a.training_step(batches[k])
    tr_a.prune(0.4)
    tr_a.training_step(batches[2])
    torch.cuda.synchronize()
    module_sd, sd = copy.deepcopy(lit_a.state_dict()), tr_a.state_dict()
    assert set(sd) == {"optimizer", "step_count", "micro", "param_steps", "pruner"}
    assert set(sd["pruner"]) == {"flags", "alive", "total", "snapshot"} and sd["pruner"]["alive"] == tr_a.pruner.alive
    for k in range(2):
        tr_a.training_step(batches[k])
    _mask_holds(tr_a, "A")

    lit_b = _lit()
    lit_b.load_state_dict(module_sd)
    tr_b = HipTrainer(lit_b, steps_per_epoch=1, pruner=MagnitudePruner(lit_b, lottery_ticket=True))
    ptrs = (tr_b.pruner.flags.data_ptr(), tr_b.pruner.snapshot.data_ptr())
    tr_b.load_state_dict(sd)
    assert ptrs == (tr_b.pruner.flags.data_ptr(), tr_b.pruner.snapshot.data_ptr())  # written in place
    assert tr_b.pruner.alive == sd["pruner"]["alive"] and tr_b.step_count == 3
    assert torch.equal(tr_b.pruner.snapshot.cpu(), sd["pruner"]["snapshot"])
    for k in range(2):
        tr_b.training_step(batches[k])
    _mask_holds(tr_b, "B")
    assert torch.equal(tr_a.pruner.flags, tr_b.pruner.flags)
    fa, fb = tr_a.store.flat, tr_b.store.flat
    err, bound = float((fa - fb).abs().max()), TOL * max(1.0, float(fa.abs().max()))
    print(f"pruned resume: err/tol {err / bound:.3f}")
    assert err <= bound
    with pytest.raises(RuntimeError, match="pruner"):
        HipTrainer(_lit(), steps_per_epoch=1).load_state_dict(sd)
    with pytest.raises(ValueError, match="lottery_ticket"):
        MagnitudePruner(lit_b).load_state_dict(sd["pruner"])


def test_prune_inside_an_accumulation_group_raises():
    from cultionet_amd.lightning import HipTrainer
    from cultionet_amd.pruning import MagnitudePruner

    lit = _lit()
    trainer = HipTrainer(lit, accumulate_grad_batches=2, steps_per_epoch=1, pruner=MagnitudePruner(lit))
    bt = _batches(1)[0]
    trainer.training_step(bt)
    with pytest.raises(RuntimeError, match="accumulated"):
        trainer.prune(0.5)
    assert trainer.pruner.alive == trainer.pruner.total
    trainer.training_step(bt)  # the group is complete: the optimizer stepped
    assert trainer.prune(0.5) > 0
    with pytest.raises(ValueError, match="ParamStore"):
        HipTrainer(_lit(), pruner=trainer.pruner)


def test_lottery_ticket_resets_survivors_to_the_snapshot():
    from cultionet_amd.lightning import HipTrainer
    from cultionet_amd.pruning import MagnitudePruner

    lit = _lit()
    pruner = MagnitudePruner(lit, lottery_ticket=True)
    assert not MagnitudePruner(lit).lottery_ticket and pruner.lottery_ticket
    trainer = HipTrainer(lit, steps_per_epoch=1, pruner=pruner)
    initial = trainer.store.flat.clone()
    batches = _batches(2)
    for bt in batches:
        trainer.training_step(bt)
    trained = trainer.store.flat.clone()
    assert float((trained - initial).abs().max()) > 0
    version = trainer.store.version
    trainer.prune(0.5)
    torch.cuda.synchronize()
    assert trainer.store.version == version + 1
    flat, flags = trainer.store.flat.view(torch.int32), pruner.flags
    alive, pruned, other = flags == 3, flags == 2, (flags & 2) == 0
    assert int(alive.sum()) == pruner.alive and int(pruned.sum()) == pruner.total - pruner.alive
    assert torch.equal(flat[alive], initial.view(torch.int32)[alive])   # survivors: the snapshot, bit for bit
    assert int((flat[pruned] != 0).sum()) == 0
    assert torch.equal(flat[other], trained.view(torch.int32)[other])   # gamma scalars (and padding): as trained
    # the selection ran on the trained magnitudes: every pruned one is at most every surviving one
    assert float(trained[pruned].abs().max()) <= float(trained[alive].abs().min())
    trainer.training_step(batches[0])
    _mask_holds(trainer, "step after the reset")


# ---- the callback on the drop-in route --------------------------------------------------------------------------------------

def test_native_pruning_callback_on_the_dropin_route():
    from cultionet_amd.optim import NativeOptimizer
    from cultionet_amd.pruning import NativePruning

    lit = _lit()
    off = NativePruning(0.5)
    with pytest.raises(RuntimeError, match="native_optimizer"):
        off.setup(types.SimpleNamespace(optimizers=[]), lit, "fit")
    lit.native_optimizer = True
    opt = _torch_side(lit, 100)[0]
    assert isinstance(opt, NativeOptimizer) and opt.pruner is None
    loop = types.SimpleNamespace(optimizers=[opt])
    cb = NativePruning(0.5)
    assert cb.lottery_ticket
    with pytest.raises(RuntimeError, match="NativeOptimizer"):
        NativePruning(0.5).on_fit_start(types.SimpleNamespace(optimizers=[]), lit)
    cb.setup(loop, lit, "fit")
    cb.on_fit_start(loop, lit)
    pruner = cb.pruner
    assert opt.pruner is pruner and pruner.store is opt.store and pruner.lottery_ticket
    initial = opt.store.flat.clone()
    batches = _batches(2)

    def step(bt):  # what lightning.Trainer runs per batch (tools/dropin_step.py)
        opt.zero_grad(set_to_none=True)
        lit.training_step(bt).backward()
        lit.configure_gradient_clipping(opt, 1.0, "norm")
        opt.step()
        torch.cuda.synchronize()
        assert opt.in_place
        assert int((opt.store.flat.view(torch.int32)[_pruned(pruner)] != 0).sum()) == 0
        assert pruner.count_alive() == pruner.alive

    for bt in batches:
        step(bt)
    cb.on_train_epoch_end(loop, lit)
    torch.cuda.synchronize()
    assert pruner.alive == pruner.total - round(0.5 * pruner.total)
    alive = pruner.flags == 3
    assert torch.equal(opt.store.flat.view(torch.int32)[alive], initial.view(torch.int32)[alive])
    before = opt.store.flat.clone()
    for bt in batches:
        step(bt)
    assert float((opt.store.flat - before)[alive].abs().max()) > 0  # the survivors train on
    # what Lightning checkpoints and restores: state_dict() -> load_state_dict() before on_fit_start of a new callback
    state = cb.state_dict()
    assert NativePruning(0.5).state_dict() == {} and set(state) == {"pruner"}
    fresh = NativePruning(0.5)
    fresh.load_state_dict(state)
    assert fresh.pruner is None
    fresh.on_fit_start(loop, lit)
    assert opt.pruner is fresh.pruner and fresh.pruner is not pruner
    assert torch.equal(fresh.pruner.flags, pruner.flags) and fresh.pruner.alive == pruner.alive
    assert torch.equal(fresh.pruner.snapshot, pruner.snapshot)
    unbound = types.SimpleNamespace(optimizers=[NativeOptimizer(list(lit.cultionet_model.parameters()), None, "AdamW")])
    with pytest.raises(RuntimeError, match="without a ParamStore"):
        NativePruning(0.5).on_fit_start(unbound, lit)
