"""The yardstick of tests/state_ref.py, checked on the CPU: how far the oracle itself is from float64 in fp32 and
under bf16 autocast, and that every mutant of the running update is flagged, per buffer tensor, under the bounds that
tests/test_model_state_gpu.py asserts (state_ref.F32_BOUND, state_ref.BF16_K).

Measured, seeds 50..52 with mask, three steps, hidden 8, B=2, 28x28 (worst ratio over all 2580 elements; 1524 for res):
  config    fp32      autocast bf16 (worst, median of the per-tensor worst)
  default   5.38e-7   7.03e-3  5.94e-4
  sca       5.34e-7   7.03e-3  6.55e-4
  res       2.81e-7   4.28e-3  4.57e-4
  bnfirst   4.58e-7   6.75e-3  6.33e-4
  dil3      5.92e-7   5.60e-3  5.74e-4
  poolmax   9.49e-7   2.18e-2  9.09e-4
Mutants, worst element of the least affected tensor (default configuration): skipped 1.57e-2, twice 1.41e-2, momentum
0.11 4.15e-3, swapped pair 1.43e-1 (1.04e-1 with batchnorm_first); biased variance 1.25e-4 or more on every
BatchNorm2d layer (n = 1568 or fewer elements per channel) but only 3.70e-6 and 5.73e-6 on the two BatchNorm3d layers
of the PreTimeReduction (n = 12544 and 15680, and a batch variance that is small beside the seeded running variance).
Skipped / twice against K = 16.4 times the autocast oracle's own error of the same tensor: flagged in all but 8 of
the 1292 tensor-cases -- one 3-channel head of the default model (quotient 15.9) and four tensors of the pool_by_max
model where the autocast oracle is itself 6e-3 .. 2e-2 off (quotients 11.2 .. 16.0). The second bf16 bound (twice the
autocast oracle's worst element over the model, state_ref.bf16_tensor_bounds) flags those: with both, every tensor of
every configuration is flagged, by a factor of 1.11 at the least (default, twice) and 1.56 for pool_by_max. These
figures move by a few per cent with the host's bf16 kernels.
"""
import statistics

import pytest
import torch

import state_ref as S

NAMES = list(S.CONFIGS)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_fp32_and_autocast_against_float64(name):
    kw = S.CONFIGS[name]
    t64, counts = S.trajectory(kw)
    ref = t64[-1]
    assert len(counts) * 2 == sum(1 for k in ref if S.is_stat(k))  # every BatchNorm layer ran, and has both buffers
    for k, v in ref.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 3, k
    r32 = S.ratios(S.trajectory(kw, "f32")[0][-1], ref)
    r16 = S.ratios(S.trajectory(kw, "bf16")[0][-1], ref)
    per16 = [float(v.max()) for v in r16.values()]
    print(f"{name}: fp32 worst {S.worst(r32):.3e}; autocast worst {max(per16):.3e}, median of per-tensor worst "
          f"{statistics.median(per16):.3e}, least {min(per16):.3e}")
    # the bound the GPU is held to must lie above what fp32 arithmetic itself gives on the same network
    assert S.worst(r32) <= S.F32_BOUND, (S.worst(r32), S.F32_BOUND)
    assert S.F32_BOUND <= 1e-5
    # the bf16 check divides by these: a tensor the autocast oracle reproduces exactly would make it vacuous or unfair
    assert min(per16) > 0.0


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mut", S.MUTANTS)
def test_mutant_is_flagged_in_every_tensor_under_the_fp32_bound(name, mut):
    kw = S.CONFIGS[name]
    t64, counts = S.trajectory(kw)
    ref = t64[-1]
    keys = S.affected(mut, ref)
    if mut == "swapped" and name == "res":
        assert not keys  # ResidualConv has no grouped pair
        return
    assert keys
    rat = S.ratios(S.mutant(mut, t64, counts), ref)
    least = min((float(rat[k].max()), k) for k in keys)
    allv = torch.cat([rat[k].flatten() for k in keys])
    print(f"{name} {mut}: least affected tensor {least[1]} worst element {least[0]:.3e}; "
          f"{float((allv < 1e-4).float().mean()):.4f} of the elements move by less than 1e-4")
    missed = [(k, float(rat[k].max())) for k in keys if not float(rat[k].max()) > S.F32_BOUND]
    if mut == "biased":
        # n / (n - 1) moves a variance by 0.1 / n of the batch variance per step. Every BatchNorm2d layer has n <= 1568
        # here and is flagged. The two BatchNorm3d layers of the PreTimeReduction see n = 12544 and 15680 elements per
        # channel and a batch variance well below their seeded running variance: 3.70e-6 and 5.73e-6, at the bound
        # itself. Part 2 does not claim the factor for these two; tests/test_pretime_exact_gpu.py and the BatchNorm3d
        # cases of tests/test_norm_gpu.py hold it at the kernels.
        layer = lambda k: k.rsplit(".", 1)[0]
        small = [k for k in keys if counts[layer(k)] <= 1568]
        assert sorted(set(keys) - set(small)) == ["pre_unet.conv3.seq.1.running_var", "pre_unet.conv5.seq.1.running_var"]
        assert min(float(rat[k].max()) for k in small) > 30 * S.F32_BOUND
        missed = [(k, v) for k, v in missed if k in small]
    assert not missed, missed
    if mut in ("skipped", "twice"):
        for k, v in ref.items():
            if k.endswith("num_batches_tracked"):
                assert int(S.mutant(mut, t64, counts)[k]) != int(v)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mut", ["skipped", "twice"])
def test_skipped_and_doubled_step_are_flagged_in_every_tensor_under_the_bf16_bound(name, mut):
    kw = S.CONFIGS[name]
    t64, counts = S.trajectory(kw)
    ref = t64[-1]
    r16 = S.ratios(S.trajectory(kw, "bf16")[0][-1], ref)
    rat = S.ratios(S.mutant(mut, t64, counts), ref)
    q = min((float(rat[k].max()) / float(r16[k].max()), k) for k in rat)
    bounds = S.bf16_tensor_bounds(r16)
    margin = min((float(rat[k].max()) / bounds[k], k) for k in rat)
    print(f"{name} {mut}: least mutant / autocast quotient {q[0]:.2f} at {q[1]} (K = {S.BF16_K}); least mutant / bound "
          f"{margin[0]:.2f} at {margin[1]}")
    missed = [(k, float(rat[k].max()), bounds[k]) for k in rat if not float(rat[k].max()) > bounds[k]]
    assert not missed, missed


def test_large_plane_case_flags_skipped_and_doubled_steps():
    """The 100x100, two-step case of the GPU test (planes 100, 50, 25, 13)."""
    t64, counts = S.trajectory({}, n=2, H=100, W=100)
    ref = t64[-1]
    r32 = S.ratios(S.trajectory({}, "f32", n=2, H=100, W=100)[0][-1], ref)
    r16 = S.ratios(S.trajectory({}, "bf16", n=2, H=100, W=100)[0][-1], ref)
    assert S.worst(r32) <= S.F32_BOUND
    for mut in ("skipped", "twice"):
        rat = S.ratios(S.mutant(mut, t64, counts), ref)
        assert min(float(v.max()) for v in rat.values()) > S.F32_BOUND
        bounds = S.bf16_tensor_bounds(r16)
        assert all(float(rat[k].max()) > bounds[k] for k in rat)


def test_recurrence_holds_for_the_oracle_and_not_for_its_mutants():
    """Same batch every step: r2 = (2 - m) r1 - (1 - m) r0 per element. The seeded buffers are random, so r1 != r0 almost
    everywhere; a doubled update or a momentum of 0.11 leaves about a hundred to thousands of times the bound in every tensor."""
    traj, counts = S.trajectory({}, n=3, same=True)
    moved = total = 0
    least = (float("inf"), "", "")
    for k in traj[0]:
        if not S.is_stat(k):
            continue
        r0, r1, r2 = traj[0][k], traj[1][k], traj[2][k]
        res, bound = S.recurrence_residual(r0, r1, r2)
        assert bool((res <= bound).all()), k
        moved += int((r1 != r0).sum())
        total += r0.numel()
        m = S.MOMENTUM
        b = (r1 - (1 - m) * r0) / m
        twice = (1 - m) * ((1 - m) * r1 + m * b) + m * b  # step two applied twice
        res, bound = S.recurrence_residual(r0, r1, twice)
        least = min(least, (float((res / bound).max()), "twice", k))
        other = (1 - 0.11) * ((1 - 0.11) * r0 + 0.11 * b) + 0.11 * b
        res, bound = S.recurrence_residual(r0, (1 - 0.11) * r0 + 0.11 * b, other)
        least = min(least, (float((res / bound).max()), "momentum 0.11", k))
    print(f"least flagged tensor: residual / bound {least[0]:.1f} ({least[1]}, {least[2]})")
    assert least[0] > 1.0, least  # flagged in every tensor, by either fault (measured: 96.6 times the bound at the least)
    assert moved >= 0.99 * total, (moved, total)
