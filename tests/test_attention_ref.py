"""Pins tests/attention_ref.py on the CPU: the mask restatement against Python integers, the NA2D reference against
scalar loops, and the bounds from both sides -- an fp32 evaluation of the same operation stays inside them at every
shape tests/test_attention_gpu.py uses, and each of six plausible kernel mistakes, applied to the float64 reference
only, leaves them; then the two seed-free checks of the engine's masks against a backward of another step word. Run
with -s to read the ratios."""
import random
from unittest import mock

import numpy as np
import pytest
import torch

import attention_ref as R
from oracle import na2d_ref as N

M = R.MASK64


def _py_splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_splitmix64_and_step_word_match_python_integers():
    rng = random.Random(7)
    seeds = [rng.getrandbits(64) for _ in range(3000)] + [0, 1, M, M - 1, 1 << 63, (1 << 63) - 1]
    idx = [rng.getrandbits(rng.choice([8, 20, 40, 64])) for _ in seeds]
    steps = [rng.getrandbits(64) for _ in seeds]
    steps[:4] = [0, 1, (1 << 63) + 5, M]
    wraps = sum(1 for s, i in zip(seeds, idx) if s + i > M)
    assert wraps > 100 and any(st >= 1 << 63 for st in steps)
    got = R.splitmix64(np.array(seeds, dtype=np.uint64))
    assert [int(v) for v in got] == [_py_splitmix64(s) for s in seeds]
    with np.errstate(over="ignore"):
        got = R.splitmix64(np.array(seeds, dtype=np.uint64) + np.array(idx, dtype=np.uint64))
    assert [int(v) for v in got] == [_py_splitmix64((s + i) & M) for s, i in zip(seeds, idx)]
    for s, st in list(zip(seeds, steps))[:200]:
        assert int(R.step_seed(s, st)[0]) == (s + st * R.STEP_MULT) & M
        assert int(R.step_seed(s, None)[0]) == s
    got = R.step_seed(np.array(seeds, dtype=np.uint64), np.array(steps, dtype=np.uint64))
    assert [int(v) for v in got] == [(s + st * R.STEP_MULT) & M for s, st in zip(seeds, steps)]
    # no step pointer is its own case: a step word of 0 gives the same seed, any other word does not
    assert int(R.step_seed(5, 0)[0]) == 5 and int(R.step_seed(5, 1)[0]) == (5 + R.STEP_MULT) & M
    # the whole decision, wrapping seed + counter past 2^64, element by element
    seed, p = M - 1000, 0.3
    index = R.na2d_index(1, 2, 5, 7)
    k = R.kept(index, p, seed, (1 << 63) + 5)
    s2 = (seed + ((1 << 63) + 5) * R.STEP_MULT) & M
    want = [_py_splitmix64((s2 + int(i)) & M) >= R.threshold(p) for i in index.reshape(-1)]
    assert k.reshape(-1).tolist() == want
    assert 0.55 < np.mean(want) < 0.85


def test_na2d_index_is_a_bijection_on_a_non_square_plane():
    B, heads, H, W = 2, 3, 5, 7
    idx = R.na2d_index(B, heads, H, W)
    assert idx.shape == (B, heads, H, W, 9)
    assert sorted(int(i) for i in idx.reshape(-1)) == list(range(B * heads * 9 * H * W))
    # ((bh * 9 + t) * HW + y * W + x), spelled out at one element
    assert int(idx[1, 2, 3, 4, 5]) == ((1 * heads + 2) * 9 + 5) * H * W + 3 * W + 4


def test_dropout_index_maps():
    B, C, L = 2, 3, 5
    e = R.dropout_index(B, C, L, False)
    assert sorted(int(i) for i in e.reshape(-1)) == list(range(B * C * L)) and int(e[1, 2, 3]) == (1 * C + 2) * L + 3
    cw = R.dropout_index(B, C, L, True)
    assert (cw == np.arange(B * C, dtype=np.uint64).reshape(B, C, 1)).all() and cw.shape == (B, C, L)
    k = R.dropout_keep(B, C, L, 0.5, 99, None, channelwise=True)
    assert (k == k[:, :, :1]).all()


def test_p_zero_keeps_everything():
    assert R.threshold(0.0) == 0
    assert R.kept(R.na2d_index(2, 2, 4, 5), 0.0, 1234, 7).all()
    assert (R.na2d_keep(2, 2, 4, 5, 0.0, 1234) == 1.0).all()
    assert (R.dropout_keep(2, 3, 10, 0.0, 5, None, True) == 1.0).all()


def test_threshold_comes_from_the_float32_value_of_p():
    t32, t64 = R.threshold(0.1), R.threshold(0.1, single=False)
    assert t32 != t64
    assert t32 == int(float(np.float32(0.1)) * 2.0 ** 64) and t64 == int(0.1 * 2.0 ** 64)
    assert R.threshold(0.5) == 1 << 63
    assert R.threshold(float(np.nextafter(np.float32(1), np.float32(0)))) < M
    assert R.keep_scale(0.5) == 2.0 and R.keep_scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))


def test_reference_with_a_mask_against_scalar_loops():
    """out and dv of na2d_reference (gathers + autograd) against loops over queries, taps and channels."""
    case = (1, 2, 3, 7, 6, 2)
    B, heads, D, H, W, dil = case
    C = heads * D
    qkv, dout = R.na2d_inputs(case, seed=3)
    keep = R.na2d_keep(B, heads, H, W, 0.4, 77, 3)
    ref = R.na2d_reference(qkv, dout, heads, dil, keep=keep)
    x, g = qkv.double(), dout.double()
    out = torch.zeros(B, C, H, W, dtype=torch.float64)
    dv = torch.zeros(B, C, H, W, dtype=torch.float64)
    for h in range(heads):
        q, k, v = (x[0, w * C + h * D: w * C + (h + 1) * D] for w in range(3))
        for y in range(H):
            for xx in range(W):
                sy, sx = N.window_start(y, H, 3, dil), N.window_start(xx, W, 3, dil)
                keys = [(sy + i * dil, sx + j * dil) for i in range(3) for j in range(3)]
                lg = torch.stack([(q[:, y, xx] * k[:, ky, kx]).sum() * D ** -0.5 for ky, kx in keys])
                pr = torch.softmax(lg, 0)
                assert torch.allclose(pr, ref["attn"][0, h, :, y, xx], rtol=1e-12, atol=0)
                for t, (ky, kx) in enumerate(keys):
                    w_ = pr[t] * keep[0, h, y, xx, t]
                    out[0, h * D:(h + 1) * D, y, xx] += w_ * v[:, ky, kx]
                    dv[0, h * D:(h + 1) * D, ky, kx] += w_ * g[0, h * D:(h + 1) * D, y, xx]
    assert torch.allclose(out, ref["out"], rtol=1e-12, atol=1e-14)
    assert torch.allclose(dv, ref["dqkv"][:, 2 * C:], rtol=1e-12, atol=1e-14)
    # the key-side mutation hook with the true mask is the identity
    same = R.na2d_reference(qkv, dout, heads, dil, keep=keep, keep_kv=keep)
    assert torch.allclose(same["dqkv"], ref["dqkv"], rtol=1e-12, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------------------

def _all_configs():
    """(id, case, bf16, keep spec or None, qk scale, zero q): every configuration tests/test_attention_gpu.py runs."""
    out = []
    for name, case in R.NA_CASES.items():
        out.append((f"f32-{name}", case, False, None, 1.0, False))
    for name in R.BF16_NA_CASES:
        out.append((f"bf16-{name}", R.NA_CASES[name], True, None, 1.0, False))
    for bf in (False, True):
        tag = "bf16" if bf else "f32"
        out.append((f"{tag}-logits60", R.NA_CASES["d8"], bf, None, 4.5, False))
        out.append((f"{tag}-q0", R.NA_CASES["d8"], bf, None, 1.0, True))
        for p in (0.1, 0.5, 0.9):
            out.append((f"{tag}-drop{p}", R.DROP_CASE, bf, (p, M - 1000, 1), 1.0, False))
    return out


CONFIGS = _all_configs()


def _inputs(case, bf16, qk_scale, zero_q, seed=0):
    qkv, dout = R.na2d_inputs(case, seed=seed, bf16=bf16, qk_scale=qk_scale)
    if zero_q:
        qkv[:, :case[1] * case[2]] = 0
    return qkv, dout


def _ratios(got, ref, bnd, tag):
    return max(R.worst_ratio(got[n], ref[n], bnd[n], f"{tag} {n}")[0] for n in ("out", "attn", "dattn", "dqkv"))


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_fp32_evaluation_stays_inside_the_bound(cfg):
    tag, case, bf16, drop, qk_scale, zero_q = cfg
    B, heads, D, H, W, dil = case
    qkv, dout = _inputs(case, bf16, qk_scale, zero_q)
    keep = R.na2d_keep(B, heads, H, W, drop[0], drop[1], drop[2]) if drop else None
    ref = R.na2d_reference(qkv, dout, heads, dil, keep=keep)
    bnd = R.na2d_bounds(qkv, dout, heads, dil, ref, keep=keep, bf16=bf16)
    f32 = R.na2d_reference(qkv, dout, heads, dil, keep=keep, dtype=torch.float32)
    if qk_scale > 1:
        assert float(ref["attn"].max()) > 0.999999 and float(N.na2d_qk(*[
            t * s for t, s in zip(R.split_heads(qkv.double(), heads)[:2], (D ** -0.5, 1.0))], 3, dil).abs().max()) > 55
    if bf16:
        f32["out"], f32["dqkv"] = f32["out"].bfloat16(), f32["dqkv"].bfloat16()
    assert _ratios(f32, ref, bnd, tag) <= 1.0


def _always_else_window_start(i, length, kernel_size, dilation):
    """oracle.na2d_ref.window_start without the `imodd < b` test: the last rows always take its second branch."""
    n = kernel_size // 2
    if dilation <= 1:
        return max(i - n, 0) + ((length - i - n - 1) if (i + n >= length) else 0)
    ni = i - n * dilation
    if ni < 0:
        return i % dilation
    if i + n * dilation >= length:
        return (length // dilation) * dilation + i % dilation - kernel_size * dilation
    return ni


MUTATIONS = ["window_branch", "transposed_taps", "scale_1_over_D", "key_pixel_in_mask", "keep_factor_1", "step_ignored"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutated_reference_leaves_the_bound(mutation):
    p, seed, step = 0.5, M - 1000, 1
    drop = mutation in ("key_pixel_in_mask", "keep_factor_1", "step_ignored")
    case = R.DROP_CASE if drop else R.NA_CASES["d8"]  # d8: W = 10 = 3 * 3 + 1, so column 9 has imodd 0 < b = 1
    B, heads, D, H, W, dil = case
    qkv, dout = R.na2d_inputs(case)
    keep = R.na2d_keep(B, heads, H, W, p, seed, step) if drop else None
    ref = R.na2d_reference(qkv, dout, heads, dil, keep=keep)
    bnd = R.na2d_bounds(qkv, dout, heads, dil, ref, keep=keep)
    if mutation == "window_branch":
        with mock.patch.object(N, "window_start", _always_else_window_start):
            mut = R.na2d_reference(qkv, dout, heads, dil)
    elif mutation == "transposed_taps":
        mut = R.na2d_reference(qkv, dout, heads, dil, transpose_taps=True)
    elif mutation == "scale_1_over_D":
        mut = R.na2d_reference(qkv, dout, heads, dil, scale=1.0 / D)
    elif mutation == "key_pixel_in_mask":
        mut = R.na2d_reference(qkv, dout, heads, dil, keep=keep, keep_kv=R.keep_at_key_pixel(keep, dil))
    elif mutation == "keep_factor_1":
        mut = R.na2d_reference(qkv, dout, heads, dil, keep=R.na2d_keep(B, heads, H, W, p, seed, step, factor=1.0))
    else:
        mut = R.na2d_reference(qkv, dout, heads, dil, keep=R.na2d_keep(B, heads, H, W, p, seed, None))
    assert _ratios(mut, ref, bnd, mutation) > 1.0
    if mutation == "key_pixel_in_mask":  # only dv moves: the other tensors are those of the true mask
        C = heads * D
        assert torch.equal(mut["out"], ref["out"]) and torch.equal(mut["dqkv"][:, :2 * C], ref["dqkv"][:, :2 * C])
        assert R.worst_ratio(mut["dqkv"][:, 2 * C:], ref["dqkv"][:, 2 * C:], bnd["dqkv"][:, 2 * C:], "dv")[0] > 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the engine tests' two checks of "the backward redraws the forward's mask", against a backward of another step word
# ---------------------------------------------------------------------------------------------------------------------

WRONG_STEPS = list(range(2, 22))  # the forward draws with step word 1


def _stored(t, bf16):
    return t.bfloat16().double() if bf16 else t.float().double()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_identity_slack_against_a_mask_of_another_step(bf16):
    """sum(dy * out) = sum(dv * v) with na2d_identity_slack, as tests/test_attention_gpu.py asserts it of the engine. The
    true mask stays inside the slack in both precisions. With dv drawn from the mask of another step word, the fp32 slack
    is left for every one of twenty words. The bf16 slack is not: it is a sum of worst-case half ulps over every
    element and most wrong words stay inside it (the count is printed), so the identity alone cannot vouch for the bf16
    path; test_mask_probe_tells_a_mask_of_another_step shows the check that does."""
    case, p, seed = R.DROP_CASE, 0.3, 20240607
    B, heads, D, H, W, dil = case
    C = heads * D
    qkv, dout = R.na2d_inputs(case, bf16=bf16)
    keep = R.na2d_keep(B, heads, H, W, p, seed, 1)
    slack = R.na2d_identity_slack(qkv, dout, heads, dil, p, bf16)
    v, dy = qkv[:, 2 * C:].double(), dout.double()

    def diff(keep_kv):
        r = R.na2d_reference(qkv, dout, heads, dil, keep=keep, keep_kv=keep_kv, dtype=torch.float32)
        return abs(float((dy * _stored(r["out"], bf16)).sum()) - float((_stored(r["dqkv"][:, 2 * C:], bf16) * v).sum()))

    right = diff(keep)
    wrong = [diff(R.na2d_keep(B, heads, H, W, p, seed, s)) for s in WRONG_STEPS]
    left = sum(1 for d in wrong if d > slack)
    print(f"identity {'bf16' if bf16 else 'f32'}: slack {slack:.4f}, true mask {right:.4f}, masks of {len(wrong)} other "
          f"step words {min(wrong):.4f} .. {max(wrong):.4f}, {left} of them leave the slack")
    assert right <= slack
    if not bf16:
        assert left == len(wrong)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_mask_probe_tells_a_mask_of_another_step(bf16):
    """The probe reads the forward's and the backward's kept taps exactly: equal to the restated mask at the probe's
    queries and to each other for the true mask, different for a backward of any other step word, in both precisions."""
    case, p, seed = R.DROP_CASE, 0.3, 20240607
    B, heads, D, H, W, dil = case
    C = heads * D
    qkv, dout, queries = R.mask_probe(case)
    assert torch.equal(qkv, qkv.bfloat16().float()) and torch.equal(dout, dout.bfloat16().float())
    keep = R.na2d_keep(B, heads, H, W, p, seed, 1)
    want = torch.stack([torch.stack([keep[b, h, queries[b][h][0], queries[b][h][1]] != 0 for h in range(heads)])
                        for b in range(B)])
    assert len({q for row in queries for q in row}) == B * heads and 0 < int(want.sum()) < want.numel()

    def taps(keep_kv):
        r = R.na2d_reference(qkv, dout, heads, dil, keep=keep, keep_kv=keep_kv, dtype=torch.float32)
        return R.probe_taps(case, p, _stored(r["out"], bf16), _stored(r["dqkv"][:, 2 * C:], bf16))

    fwd, bwd = taps(keep)
    assert torch.equal(fwd, want) and torch.equal(bwd, want)
    for s in WRONG_STEPS:
        fwd, bwd = taps(R.na2d_keep(B, heads, H, W, p, seed, s))
        assert torch.equal(fwd, want) and not torch.equal(bwd, want)
    # a forward that drew another mask shows as well
    other = R.na2d_keep(B, heads, H, W, p, seed, 2)
    r = R.na2d_reference(qkv, dout, heads, dil, keep=other, keep_kv=keep, dtype=torch.float32)
    fwd, bwd = R.probe_taps(case, p, _stored(r["out"], bf16), _stored(r["dqkv"][:, 2 * C:], bf16))
    assert torch.equal(bwd, want) and not torch.equal(fwd, want)
