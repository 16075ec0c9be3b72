"""float64 references and per-element error bounds for the neighborhood-attention kernels (cn_na2d.hip, the NA2D part of
cn_bops.hip) and the dropout kernels (cn_dropout_f32, cn_dropout_bf16), with the counter-based dropout masks restated
outside the kernels. A plain module: no GPU, no test; tests/test_attention_ref.py pins it, tests/test_attention_gpu.py
holds the kernels to it.

Masks. An element of counter i is KEPT when splitmix64(seed' + i) >= thresh (64-bit wrap-around sums), where
  thresh = floor(double(float32(p)) * 2^64), saturating at 2^64 - 1 (0 for p <= 0: everything is kept);
  seed'  = seed when the launch has no step pointer, else seed + step * 0xD1B54A32D192ED03 mod 2^64;
  i      = ((bh * 9 + t) * HW + pixel) for tap t of the QUERY `pixel` of plane bh = b * heads + h in NA2D,
           (b * C + c) * L + l for elementwise dropout, b * C + c for channelwise (Dropout2d) dropout.
A kept value is multiplied by the fp32 number 1 / (1 - p) the launchers compute: keep_scale(p) = fl(1 / fl(1 - p)).

NA2D (K = 3, head dimension D, scale = D^-1/2; q, k, v the channel blocks of one qkv tensor; g = dOut):
  l_t = scale * sum_d q_d k_td    P = softmax_t(l)    P~_t = P_t * keep_t    out_d = sum_t P~_t v_td
  dP~_t = keep_t * sum_d g_d v_td    dS_t = P_t (dP~_t - sum_s P_s dP~_s)
  dq_d = scale * sum_t dS_t k_td;  for a key pixel, over the (query, t) pairs whose tap t is that pixel (at most 25):
  dk_d = scale * sum dS_t[query] q_d[query],  dv_d = sum P~_t[query] g_d[query].
The kernels save P (undropped) as `attn` and dS as `dattn`; the reference returns both.

Bounds. u = 2^-24, c = 16 roundings for an element's own chain (the house constant of tests/test_norm_gpu.py; the
softmax chain has 13: exp 2, a nine-term denominator 8, reciprocal, product, keep factor). A serial fp32 sum of n
products is off by at most n * u * sum|terms|, whatever its order; first-order propagation of every input error:
  e_t    = (D + c) u scale sum_d |q_d||k_td|                      logit (the rounding of l_t - max is part of c)
  dP_t   = P_t (2 max_t e_t + c u) + T                            the error of the maximum cancels in the quotient
  dP~_t  = keep_t dP_t
  out_d  : sum_t |v_td| dP~_t + (9 + c) u sum_t P~_t |v_td| + T
  ddP~_t = keep_t (D + c) u sum_d |g_d||v_td|  (+ c u |dP~_t| when a keep factor multiplies it)
  ddot   = sum_t (dP_t |dP~_t| + P_t ddP~_t) + (9 + c) u sum_t P_t |dP~_t|
  ddS_t  = dP_t |dP~_t - dot| + P_t (ddP~_t + ddot) + c u P_t (|dP~_t| + |dot|) + T
  dq_d   : scale (sum_t ddS_t |k_td| + (9 + c) u sum_t |dS_t||k_td|) + T
  dk_d   : scale (sum ddS_t |q_d| + (25 + c) u sum |dS_t||q_d|) + T          sums over the key's (query, t) pairs
  dv_d   : sum dP~_t |g_d| + (25 + c) u sum P~_t |g_d| + T
T = 2^-126 is the fp32 underflow threshold: below it a result may be flushed to zero or lose bits (softmax tails at
logits of +-60), an absolute error no relative term covers. There is no max|ref| and no other floor: an element whose
inputs are all zero has bound T, and an output that must be exactly zero is asserted to be so by the tests.
bf16: the reference runs on the bf16-rounded operands (exact in fp32), the kernels accumulate in fp32, so the forms are
unchanged; `out` and `dqkv` are stored as bf16 and get half a bf16 ulp (half_ulp16) added, `attn` / `dattn` stay fp32.

Dropout: y = x * keep; against x * keep_scale(p) in float64 a kept value is one fp32 rounding off (u |y|), one more
(u |dest + y|) when it is accumulated into a destination, plus half a bf16 ulp when stored as bf16.

Engine masks, whose seed the tests do not know: na2d_identity_slack bounds sum(dy * out) - sum(dv * v), and mask_probe /
probe_taps read the taps a forward and its backward kept exactly from their outputs.
"""
import numpy as np
import torch

from oracle import na2d_ref as N

U = 2.0 ** -24
C_CHAIN = 16.0
TINY = 2.0 ** -126
MASK64 = (1 << 64) - 1
STEP_MULT = 0xD1B54A32D192ED03
KEY_DEPTH = 25  # queries whose 3x3 window can hold one key pixel: 5 per axis

# NA2D cases shared by the CPU and the GPU tests: name -> (B, heads, D, H, W, dilation). Window rule: H = 3 * dil
# (d2, d8), len % dil != 0 with rows on both sides of `imodd < b` (W of d2, d8, d16; both axes of d32, r6), len % dil == 0
# (H of d16, r24), H != W everywhere, dilations 1 / 2 / 3. Launch geometry of the fp32 kernels (256 pixels per block,
# blocks dealt in eights): planes under 256 pixels and 17 x 19 = 323 (d4, r6: two blocks per plane); block totals 6
# (d4), 4 (d8, r6), 2 (d16, d32, r12), 1 (d64, r24): the tail of the last eight returns early; 8 (d2) has no tail.
# Head dimensions: every compiled one, and run-time 3 (one ragged sweep of the key pass), 6, 12 (8 + a ragged 4), 24.
NA_CASES = {
    "d2": (2, 4, 2, 6, 7, 2),
    "d4": (1, 3, 4, 17, 19, 1),
    "d8": (2, 2, 8, 9, 10, 3),
    "d16": (1, 2, 16, 8, 11, 2),
    "d32": (1, 2, 32, 11, 13, 3),
    "d64": (1, 1, 64, 7, 9, 1),
    "r3": (2, 3, 3, 7, 6, 2),
    "r6": (1, 2, 6, 17, 19, 3),
    "r12": (1, 2, 12, 9, 8, 1),
    "r24": (1, 1, 24, 6, 10, 2),
}
BF16_NA_CASES = ("d4", "d8", "d16", "d32", "d64")
DROP_CASE = (2, 2, 8, 7, 10, 2)  # attention dropout: two blocks of bf16 lanes, W % dil == 0, H % dil != 0


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------

def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


def splitmix64(z):
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def step_seed(seed, step=None):
    """The seed a launch hashes with: `seed` itself without a step pointer (step None), else seed + step * STEP_MULT."""
    s = _u64(seed)
    if step is None:
        return s
    with np.errstate(over="ignore"):
        return s + _u64(step) * np.uint64(STEP_MULT)


def threshold(p, single=True):
    """Keep threshold of drop probability p. single: from the float32 value of p, as the launchers take it."""
    pv = float(np.float32(p)) if single else float(p)
    if not pv > 0.0:
        return 0
    t = pv * 18446744073709551616.0
    return MASK64 if t >= 18446744073709551615.0 else int(t)


def keep_scale(p):
    """The fp32 factor of a kept value, 1 / (1 - p) evaluated in float32."""
    one = np.float32(1.0)
    return float(one / (one - np.float32(p)))


def kept(index, p, seed, step=None):
    """bool array: which counters are kept."""
    with np.errstate(over="ignore"):
        h = splitmix64(step_seed(seed, step) + _u64(index).reshape(-1)).reshape(np.shape(index))
    return h >= np.uint64(threshold(p))


def na2d_index(B, heads, H, W):
    """[B, heads, H, W, 9] counters of the attention taps."""
    HW = H * W
    bh = np.arange(B * heads, dtype=np.uint64).reshape(B, heads, 1, 1)
    t = np.arange(9, dtype=np.uint64).reshape(1, 1, 9, 1)
    pix = np.arange(HW, dtype=np.uint64).reshape(1, 1, 1, HW)
    idx = (bh * np.uint64(9) + t) * np.uint64(HW) + pix  # [B, heads, 9, HW]
    return np.ascontiguousarray(idx.reshape(B, heads, 9, H, W).transpose(0, 1, 3, 4, 2))


def na2d_keep(B, heads, H, W, p, seed, step=None, factor=None):
    """[B, heads, H, W, 9] float64: 0 for a dropped tap, 1 / (1 - p) (`factor` overrides it) for a kept one."""
    k = kept(na2d_index(B, heads, H, W), p, seed, step)
    return torch.from_numpy(k.astype(np.float64)) * (keep_scale(p) if factor is None else factor)


def dropout_index(B, C, L, channelwise):
    plane = np.arange(B * C, dtype=np.uint64).reshape(B, C, 1)
    if channelwise:
        return np.broadcast_to(plane, (B, C, L)).copy()
    return plane * np.uint64(L) + np.arange(L, dtype=np.uint64).reshape(1, 1, L)


def dropout_keep(B, C, L, p, seed, step=None, channelwise=False):
    """[B, C, L] float64: 0 or 1 / (1 - p)."""
    k = kept(dropout_index(B, C, L, channelwise), p, seed, step)
    return torch.from_numpy(k.astype(np.float64)) * keep_scale(p)


# ---------------------------------------------------------------------------------------------------------------------
# NA2D reference
# ---------------------------------------------------------------------------------------------------------------------

def split_heads(x, heads):
    """qkv [B, 3C, H, W] (channel = which * C + head * D + d) -> q, k, v as [B, heads, H, W, D]."""
    B, C3, H, W = x.shape
    t = x.reshape(B, 3, heads, C3 // 3 // heads, H, W).permute(1, 0, 2, 4, 5, 3)
    return t[0], t[1], t[2]


def _heads(x, heads):
    """[B, C, H, W] -> [B, heads, H, W, D]."""
    B, C, H, W = x.shape
    return x.reshape(B, heads, C // heads, H, W).permute(0, 1, 3, 4, 2)


def _planes(t):
    """[B, heads, H, W, D] -> [B, heads * D, H, W]."""
    B, h, H, W, D = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(B, h * D, H, W)


def _taps_first(t):
    """[B, heads, H, W, 9] -> the kernels' [B, heads, 9, H, W]."""
    return t.permute(0, 1, 4, 2, 3).contiguous()


def key_pixels(H, W, dil):
    """[H, W, 9] flat pixel of tap t of every query."""
    ih, iw = N.window_index(H, 3, dil), N.window_index(W, 3, dil)
    return (ih[:, None, :, None] * W + iw[None, :, None, :]).reshape(H, W, 9)


def keep_at_key_pixel(keep, dil):
    """The mutation "key pixel in the mask index": tap t of a query takes the decision of counter (bh, t, its KEY pixel)."""
    B, h, H, W, _ = keep.shape
    flat = keep.permute(0, 1, 4, 2, 3).reshape(B, h, 9, H * W)
    kp = key_pixels(H, W, dil).reshape(H * W, 9).t()  # [9, HW]
    g = torch.gather(flat, 3, kp[None, None].expand(B, h, 9, H * W))
    return g.reshape(B, h, 9, H, W).permute(0, 1, 3, 4, 2)


def scatter_to_keys(a, b, dil):
    """[B, heads, H, W, D]: for every key pixel, sum of a[query, t] * b[query, d] over the (query, t) whose tap t is that
    pixel -- the adjoint of na2d_av in v."""
    v0 = torch.zeros_like(b, requires_grad=True)
    (r,) = torch.autograd.grad((N.na2d_av(a, v0, 3, dil) * b).sum(), v0)
    return r


def na2d_reference(qkv, dout, heads, dil, keep=None, dtype=torch.float64, scale=None, transpose_taps=False,
                   keep_kv=None):
    """qkv [B, 3C, H, W], dout [B, C, H, W] -> out [B, C, H, W], attn / dattn [B, heads, 9, H, W], dqkv [B, 3C, H, W].
    keep: [B, heads, H, W, 9] factors on the probabilities. The last three arguments are mutations for the tests of the
    bounds: another scale, transposed taps after the logits, another keep tensor in the key-side sum dv."""
    x = qkv.detach().to(dtype).clone().requires_grad_(True)
    q, k, v = split_heads(x, heads)
    D = q.shape[-1]
    scale = D ** -0.5 if scale is None else scale
    logits = N.na2d_qk(q * scale, k, 3, dil)
    if transpose_taps:
        logits = logits.reshape(*logits.shape[:-1], 3, 3).transpose(-1, -2).reshape(logits.shape)
    P = logits.softmax(dim=-1)
    Pd = P if keep is None else P * keep.to(dtype)
    out = _planes(N.na2d_av(Pd, v, 3, dil))
    g = dout.detach().to(dtype)
    dx, dS = torch.autograd.grad((out * g).sum(), [x, logits])
    if keep_kv is not None:
        dv = _planes(scatter_to_keys(P.detach() * keep_kv.to(dtype), _heads(g, heads), dil))
        C = g.shape[1]
        dx = torch.cat([dx[:, :2 * C], dv], dim=1)
    return {"out": out.detach(), "attn": _taps_first(P.detach()), "dattn": _taps_first(dS), "dqkv": dx}


def half_ulp16(y, slack):
    """Half a bf16 ulp of the stored value, which lies within |y| + slack (tests/test_norm_gpu.py _half_ulp16); zero
    where that is zero."""
    mag = y.abs() + slack
    _, e = torch.frexp(mag)
    return torch.where(mag == 0, torch.zeros_like(mag), torch.ldexp(torch.ones_like(mag), e - 9))


def na2d_bounds(qkv, dout, heads, dil, ref, keep=None, bf16=False, c=C_CHAIN):
    """Per-element bounds (module docstring) in the layouts of `ref` (a float64 na2d_reference result). "mag_out" and
    "mag_dv" are sum P~|v| and sum P~|g|: what |out| and |dv| cannot exceed."""
    x = qkv.detach().double()
    q, k, v = split_heads(x, heads)
    g = _heads(dout.detach().double(), heads)
    D = q.shape[-1]
    scale = D ** -0.5
    P = ref["attn"].permute(0, 1, 3, 4, 2)
    dS = ref["dattn"].permute(0, 1, 3, 4, 2)
    kp = torch.ones_like(P) if keep is None else keep.double()
    e = (D + c) * U * scale * N.na2d_qk(q.abs(), k.abs(), 3, dil)
    dP = P * (2 * e.max(dim=-1, keepdim=True).values + c * U) + TINY
    Pt, dPt = P * kp, kp * dP
    mag_out = N.na2d_av(Pt, v.abs(), 3, dil)
    b_out = N.na2d_av(dPt, v.abs(), 3, dil) + (9 + c) * U * mag_out + TINY
    gp = kp * N.na2d_qk(g, v, 3, dil)  # dP~
    dgp = kp * (D + c) * U * N.na2d_qk(g.abs(), v.abs(), 3, dil)
    if keep is not None:
        dgp = dgp + c * U * gp.abs()
    dot = (P * gp).sum(-1, keepdim=True)
    ddot = (dP * gp.abs() + P * dgp).sum(-1, keepdim=True) + (9 + c) * U * (P * gp.abs()).sum(-1, keepdim=True)
    ddS = dP * (gp - dot).abs() + P * (dgp + ddot) + c * U * P * (gp.abs() + dot.abs()) + TINY
    b_dq = scale * (N.na2d_av(ddS, k.abs(), 3, dil) + (9 + c) * U * N.na2d_av(dS.abs(), k.abs(), 3, dil)) + TINY
    b_dk = scale * (scatter_to_keys(ddS, q.abs(), dil)
                    + (KEY_DEPTH + c) * U * scatter_to_keys(dS.abs(), q.abs(), dil)) + TINY
    mag_dv = scatter_to_keys(Pt, g.abs(), dil)
    b_dv = scatter_to_keys(dPt, g.abs(), dil) + (KEY_DEPTH + c) * U * mag_dv + TINY
    b_out = _planes(b_out)
    b_dqkv = torch.cat([_planes(b_dq), _planes(b_dk), _planes(b_dv)], dim=1)
    if bf16:
        b_out = b_out + half_ulp16(ref["out"], b_out)
        b_dqkv = b_dqkv + half_ulp16(ref["dqkv"], b_dqkv)
    return {"out": b_out, "attn": _taps_first(dP), "dattn": _taps_first(ddS), "dqkv": b_dqkv,
            "mag_out": _planes(mag_out), "mag_dv": _planes(mag_dv)}


def na2d_inputs(case, seed=0, bf16=False, qk_scale=1.0):
    """qkv [B, 3C, H, W] and dout [B, C, H, W] (float32 on the CPU; bf16: rounded to bf16) of an NA_CASES-style tuple."""
    B, heads, D, H, W, _ = case
    C = heads * D
    gen = torch.Generator().manual_seed(1000 + seed)
    qkv = torch.randn(B, 3 * C, H, W, generator=gen)
    qkv[:, :2 * C] *= qk_scale
    dout = torch.randn(B, C, H, W, generator=gen)
    if bf16:
        qkv, dout = qkv.bfloat16().float(), dout.bfloat16().float()
    return qkv, dout


def na2d_identity_slack(qkv, dout, heads, dil, p, bf16):
    """Slack of sum(dy * out) = sum(dv * v) under an unknown mask of drop probability p: the bounds of `out` and of dv
    with every tap kept (each term of the bounds grows with the keep factor), weighted by |dy| and |v| and summed. It is
    a sum of worst cases over every element, so it grows with the element count N while the mismatch of two independent
    masks grows with sqrt(N): with the bf16 half ulps in it, it is too wide to tell one mask from another
    (tests/test_attention_ref.py measures that), which is what the mask probe below is for."""
    B, C3, H, W = qkv.shape
    C = C3 // 3
    ref = na2d_reference(qkv, dout, heads, dil)
    full = torch.full((B, heads, H, W, 9), keep_scale(p), dtype=torch.float64)
    bnd = na2d_bounds(qkv, dout, heads, dil, ref, keep=full)
    b_out, b_dv = bnd["out"], bnd["dqkv"][:, 2 * C:]
    if bf16:
        b_out = b_out + half_ulp16(bnd["mag_out"], b_out)
        b_dv = b_dv + half_ulp16(bnd["mag_dv"], b_dv)
    return float((dout.double().abs() * b_out).sum() + (qkv[:, 2 * C:].double().abs() * b_dv).sum())


# ---------------------------------------------------------------------------------------------------------------------
# mask probe: inputs from which the forward's mask and the backward's mask can each be read exactly, without the seed
# ---------------------------------------------------------------------------------------------------------------------

def _probe_queries(B, heads, H, W):
    """One query (y, x) per (b, head): the corners and interior pixels in turn, so that clamped windows take part."""
    spots = [(0, 0), (H // 2, W // 2), (H - 1, W - 1), (H // 3, W - 2), (H - 1, 0), (1, W // 3)]
    return [[spots[(b * heads + h) % len(spots)] for h in range(heads)] for b in range(B)]


def mask_probe(case):
    """qkv, dout, queries. q = 0, so all nine probabilities are 1/9. For the query Q of plane (b, head), the value at
    the key pixel of tap t holds 2^t in channel 0 (t < 5) or 2^(t - 5) in channel 1 (t >= 5) of the head and 0
    elsewhere, so out[Q] in those two channels spells which taps the FORWARD kept; dout is 1 in every channel of the head
    at Q and 0 elsewhere, so dv at the key pixel of tap t is keep_t / 9 where the BACKWARD kept the tap and exactly 0
    where it did not. Every value is exact in bf16, and a bf16 output resolves the five-bit codes (for p <= 0.5 the
    largest value, 31 * keep / 9, is under 8, where half a bf16 ulp is 2^-6: a tenth of a code step)."""
    B, heads, D, H, W, dil = case
    assert D >= 2
    C = heads * D
    qkv = torch.zeros(B, 3 * C, H, W)
    qkv[:, C:2 * C] = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(77)).bfloat16().float()
    dout = torch.zeros(B, C, H, W)
    queries = _probe_queries(B, heads, H, W)
    kp = key_pixels(H, W, dil)
    for b in range(B):
        for h in range(heads):
            y, x = queries[b][h]
            dout[b, h * D:(h + 1) * D, y, x] = 1.0
            for t in range(9):
                ky, kx = divmod(int(kp[y, x, t]), W)
                qkv[b, 2 * C + h * D + (0 if t < 5 else 1), ky, kx] = 2.0 ** (t if t < 5 else t - 5)
    return qkv, dout, queries


def probe_taps(case, p, out, dv):
    """(forward, backward): bool [B, heads, 9] kept taps of the probe's queries, read from `out` and from dv (the last
    third of dqkv). Asserts that both are readable: integer codes forward; backward every channel of a key pixel zero
    or non-zero together, and dv exactly zero off the window."""
    B, heads, D, H, W, dil = case
    queries = _probe_queries(B, heads, H, W)
    kp = key_pixels(H, W, dil)
    s = keep_scale(p)
    out, dv = out.double(), dv.double()
    fwd = torch.zeros(B, heads, 9, dtype=torch.bool)
    bwd = torch.zeros(B, heads, 9, dtype=torch.bool)
    for b in range(B):
        for h in range(heads):
            y, x = queries[b][h]
            codes = out[b, h * D:h * D + 2, y, x] * 9.0 / s
            ints = codes.round()
            assert float((codes - ints).abs().max()) < 0.2 and 0 <= int(ints[0]) < 32 and 0 <= int(ints[1]) < 16, codes
            assert bool((out[b, h * D + 2:(h + 1) * D, y, x] == 0).all())
            plane = dv[b, h * D:(h + 1) * D].reshape(D, H * W)
            off = torch.ones(H * W, dtype=torch.bool)
            for t in range(9):
                fwd[b, h, t] = bool((int(ints[0 if t < 5 else 1]) >> (t if t < 5 else t - 5)) & 1)
                col = plane[:, int(kp[y, x, t])]
                assert bool((col != 0).all()) or bool((col == 0).all()), col
                assert bool(((col - s / 9.0).abs() < 0.01 * s).all()) or bool((col == 0).all()), col
                bwd[b, h, t] = bool((col != 0).all())
                off[int(kp[y, x, t])] = False
            assert bool((plane[:, off] == 0).all()), "dv is not zero off the query's window"
    return fwd, bwd


def worst_ratio(got, ref, bound, what):
    """Largest err / bound over the elements (printed); an exact element counts 0 whatever its bound."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst err/bound {worst:.3f}")
    return worst, err, ratio


def within(got, ref, bound, what):
    worst, err, ratio = worst_ratio(got, ref, bound, what)
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        got = got.detach().double().cpu()
        raise AssertionError(f"{what}: err {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e} at flat "
                             f"index {i} (got {float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r})")
    return worst
