"""CPU reference and yardstick for the BatchNorm state of the whole model (tests/test_state_ref.py checks it on the CPU,
tests/test_model_state_gpu.py holds the HIP engine to it).

Reference: oracle.towerunet_oracle.TowerUNet with the key-seeded weights, in float64, train mode, under no_grad, fed the
seeded batch sequence. Parameters never move, so a layer's batch statistic b_k at step k does not depend on its running
buffers and the whole trajectory r_0 .. r_n of every buffer follows r_k = (1 - m) r_{k-1} + m b_k. The mutants below are
restated from that recorded trajectory in float64 (b_k = (r_k - (1 - m) r_{k-1}) / m), which is exact to ~1e-15.

Compared quantity, per element: ratio = |got - ref64| / S with S = |m64| + sqrt(v64) for running_mean and S = v64 for
running_var, both from that channel's float64 buffers after the steps. No floor, no per-tensor maximum.
"""
import contextlib
import functools

import torch

MOMENTUM = 0.1  # torch's default, which the reference never changes
U = 2.0 ** -24

CONFIGS = {
    "default": {},
    "sca": {"attention_weights": "spatial_channel"},
    "res": {"res_block_type": "res", "attention_weights": None},
    "bnfirst": {"batchnorm_first": True},
    "dil3": {"dilations": [1, 3]},
    "poolmax": {"pool_by_max": True},
}

MUTANTS = ("skipped", "twice", "momentum", "biased", "swapped")


def batch_sequence(n, B=2, H=28, W=28, seed0=50, with_mask=True, same=False):
    """The seeded batches of tests/test_replay_train_gpu.py: seeds 50, 51, 52, 50, ... (``same``: seed0 every step)."""
    from oracle import towerunet_oracle as O

    three = [O.seeded_batch(B, height=H, width=W, seed=seed0 + k, with_mask=with_mask) for k in range(1 if same else 3)]
    return [three[i % len(three)] for i in range(n)]


def is_stat(key):
    return key.endswith("running_mean") or key.endswith("running_var")


def snapshot(model):
    """Every BatchNorm buffer (running_mean, running_var, num_batches_tracked) as float64 / int64 CPU copies."""
    out = {}
    for k, v in model.state_dict().items():
        if is_stat(k):
            out[k] = v.detach().double().cpu().clone()
        elif k.endswith("num_batches_tracked"):
            out[k] = v.detach().cpu().clone()
    return out


def _frozen(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _trajectory(kwf, mode, n, B, H, W, same, hidden):
    from oracle import towerunet_oracle as O

    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kwf}
    ref = O.TowerUNet(3, 12, hidden_channels=hidden, **kw)
    ref.load_state_dict(O.seeded_state_dict(ref.state_dict()))
    if mode == "f64":
        ref = ref.double()
    ref.train()
    counts = {}

    def hook(name):
        def fn(mod, inp, out):
            counts[name] = inp[0].numel() // inp[0].shape[1]
        return fn

    for name, m in ref.named_modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            assert m.momentum == MOMENTUM
            m.register_forward_hook(hook(name))
    traj = [snapshot(ref)]
    cast = torch.autocast("cpu", dtype=torch.bfloat16) if mode == "bf16" else contextlib.nullcontext()
    with torch.no_grad(), cast:
        for x, _, _ in batch_sequence(n, B, H, W, same=same):
            ref(x.double() if mode == "f64" else x)
            traj.append(snapshot(ref))
    return traj, counts


def trajectory(kw=None, mode="f64", n=3, B=2, H=28, W=28, same=False, hidden=8):
    """(buffers after 0 .. n train-mode forwards, elements per channel of every BatchNorm layer) of the oracle in
    ``mode``: "f64" (the reference), "f32", or "bf16" (fp32 weights under torch.autocast("cpu", bfloat16)). Cached: the
    returned tensors are shared between tests and must not be written."""
    return _trajectory(_frozen(kw or {}), mode, n, B, H, W, same, hidden)


def ratios(got, ref):
    """Per element |got - ref64| / S for every running_mean / running_var of ``ref`` (see the module docstring)."""
    out = {}
    for k, r in ref.items():
        if k.endswith("running_mean"):
            v = ref[k[:-len("running_mean")] + "running_var"]
            out[k] = (got[k].double().cpu() - r).abs() / (r.abs() + v.sqrt())
        elif k.endswith("running_var"):
            out[k] = (got[k].double().cpu() - r).abs() / r
    return out


def worst(rat):
    return max(float(v.max()) for v in rat.values())


def pair_of(key):
    """The same buffer of the other branch of a grouped ResidualAConv pair (res_modules.0 <-> res_modules.1), or None."""
    for a, b in ((".res_modules.0.", ".res_modules.1."), (".res_modules.1.", ".res_modules.0.")):
        if a in key:
            return key.replace(a, b)
    return None


def mutant(name, traj, counts):
    """Final buffers of the oracle with one fault in its running update (float64, from the recorded trajectory)."""
    m = MOMENTUM
    last, prev = traj[-1], traj[-2]
    out = {k: v.clone() for k, v in last.items()}
    steps = len(traj) - 1
    for k in last:
        if not is_stat(k):
            out[k] = last[k] + {"skipped": -1, "twice": 1}.get(name, 0)
            continue
        layer = k.rsplit(".", 1)[0]
        b = [(traj[i][k] - (1 - m) * traj[i - 1][k]) / m for i in range(1, steps + 1)]
        if name == "skipped":
            out[k] = prev[k].clone()
        elif name == "twice":
            out[k] = (1 - m) * last[k] + m * b[-1]
        elif name == "momentum":
            r = traj[0][k]
            for bk in b:
                r = (1 - 0.11) * r + 0.11 * bk
            out[k] = r
        elif name == "biased" and k.endswith("running_var"):
            n = counts[layer]
            r = traj[0][k]
            for bk in b:
                r = (1 - m) * r + m * bk * (n - 1) / n
            out[k] = r
        elif name == "swapped" and pair_of(k) in last:
            out[k] = last[pair_of(k)].clone()
    return out


def affected(name, ref):
    """The buffer tensors a mutant moves: all of them, the variances only (biased), the grouped pairs only (swapped)."""
    keys = [k for k in ref if is_stat(k)]
    if name == "biased":
        return [k for k in keys if k.endswith("running_var")]
    if name == "swapped":
        return [k for k in keys if pair_of(k) in ref]
    return keys


def recurrence_residual(r0, r1, r2, c=16.0, m=MOMENTUM):
    """Identical batches, frozen parameters: r2 = (2 - m) r1 - (1 - m) r0 whatever the batch statistic is. Returns
    (|residual|, bound) per element with bound = c * u * (|r0| + 2 |r1| + |r2|)."""
    r0, r1, r2 = (t.double().cpu() for t in (r0, r1, r2))
    return (r2 - (2 - m) * r1 + (1 - m) * r0).abs(), c * U * (r0.abs() + 2 * r1.abs() + r2.abs())


# The bounds tests/test_model_state_gpu.py asserts (measured on the MI355X; see that module's docstring) and
# tests/test_state_ref.py checks the mutants against.
F32_BOUND = 3.85e-6  # 4 x 9.617e-7, the worst fp32 ratio over all cases (pool_by_max; the fp32 oracle itself: 9.49e-7)
BF16_K = 16.4        # 2 x 8.22, the worst per-tensor quotient of HIP bf16 to the autocast oracle (res, a 3-channel head)
BF16_MODEL = 2.0     # and no tensor further from float64 than twice the autocast oracle's worst element anywhere


def bf16_tensor_bounds(r16):
    """Per buffer tensor, the bound on max ratio(HIP bf16) from the autocast oracle's own ratios ``r16``: K times that
    tensor's worst element. The quotient is noisy where the autocast oracle happens to be close to float64 in a
    3-element tensor, and K is sized by the noisiest; in the few tensors where the autocast oracle is itself far off,
    K times its error exceeds what a skipped step moves. So a tensor is also held to BF16_MODEL times the autocast
    oracle's worst element over the whole model (the reference's own error, with the factor two K carries as well)."""
    cap = BF16_MODEL * worst(r16)
    return {k: min(BF16_K * float(v.max()), cap) for k, v in r16.items()}
