"""float64 restatement of the fused PreTimeReduction family (cultionet_amd/csrc/cn_pretime.hip) with a per-element error
bound for every quantity its C ABI produces. A plain module: no GPU, no test; tests/test_pretime_ref.py pins it to the
oracle module, tests/test_pretime_exact_gpu.py holds the kernels to it.

The chain, per branch k in {3, 5} (Tp = T - k + 1, P = B HW pixels, cnt3 = P Tp, x [B, C, T, HW]):
  h[cp, tp]  = sum_{c, dt} wa[cp, c, dt] x[c, tp + dt]                           Conv3d (k, 1, 1)
  xh = (h - m3) rho3,  z = g3 xh + b3,  a = SiLU(z)                              BatchNorm3d over (B, Tp, HW)
  r[o]       = sum_{cp, tp} wb[o, cp, tp] a[cp, tp]                              Conv3d (Tp, 1, 1)
  rh = (r - m2) rho2,  v = g2 rh + b2,  s = SiLU(v)                              BatchNorm2d over (B, HW)
  uu = s_3 + s_5,  mL = mean_o uu,  rL = (mean_o (uu - mL)^2 + epsL)^-1/2,  uhat = (uu - mL) rL,  y = gL uhat + bL
Training: m, rho from the batch (biased variance, rho = (var + eps)^-1/2), running <- (1 - mom) running + mom (mean,
var cnt / (cnt - 1)). Inference / training = 0: m, rho from the running statistics, which stay as they are.
Backward (dy given; k2 = k3 = 1 in training, 0 with training = 0):
  gj = dy gL,  s1 = mean_o gj,  s2 = mean_o gj uhat,  du = rL (gj - s1 - uhat s2),  dgL = sum_p dy uhat,  dbL = sum_p dy
  dv = du SiLU'(v),  db2 = sum_p dv,  dg2 = sum_p dv rh,  dr = g2 rho2 (dv - k2 (db2 / P) - k2 rh (dg2 / P))
  dwb[o, cp, tp] = sum_p dr[o] a[cp, tp],  da[cp, tp] = sum_o wb[o, cp, tp] dr[o],  dz = da SiLU'(z)
  db3 = sum dz,  dg3 = sum dz xh,  dh = g3 rho3 (dz - k3 (db3 / cnt3) - k3 xh (dg3 / cnt3))
  dwa[cp, c, dt] = sum_{p, tp} dh[cp, tp] x[c, tp + dt]
and every gradient is ADDED to what its buffer held.

Bounds. u = 2^-24; c = 16 roundings for an element's own chain, the house constant of tests/test_norm_gpu.py. The longest
chain of one stage here is the activation: fused multiply-add of the normalisation (1, with the rounded offset -m rho: 2
more), affine (1), product by -log2(e) (1), v_exp_f32 (1 ulp = 2), add (1), v_rcp_f32 (1 ulp = 2), product (1): 11, and
SiLU' adds three more. The rounding of the exp2 ARGUMENT is relative |z| u in the exponential, so an activation
carries (c + |z|) u |a| of its own. A serial fp32 sum of n terms is off by at most n u sum|terms| whatever its order.
Every stage carries (value, bound); the bound is the stage's own term plus the inherited bounds to first order:
  h      (C k + 2) u sum|wa||x|                              two FMA chains of C k / 2 and their sum
  m      D u (|m| + s) + mean(e_h) + u |m|                   s = sqrt(var); the ticket and the finish are fp64 (+ 0)
  var    dv = 3 D u (m^2 + var) + 2 mean(|h - m| e_h)        E[h^2] - m^2 cancels that much
  rho    2 u rho + ((max(var - dv, 0) + eps)^-1/2 - rho)     exact, not first order: var of a few pixels can be ~dv
  xh     c u rho (|h| + |m|) + rho (e_h + dm) + |h - m| e_rho
  z      c u (|g xh| + |b|) + |g| e_xh;     a: (c + |z|) u |a| + 1.1 e_z        (max |SiLU'| = 1.0998)
  r      (C Tp + c) u sum|wb||a| + sum|wb| e_a               the MFMA chain of one accumulator walks every entry
  LayerNorm over Cout with D_L = 16 MT + 1 (a lane's accumulator registers, then the other half-wave): the mean carries
         mean(e_uu) + D_L u mean|uu|, the two-pass variance 2 mean(|d| e_d) + (D_L + 2) u var, uhat and y as xh and z.
  SiLU'  (c + |z|) u s (1 + |z| (1 - s)) + e_z / 2           (max |SiLU''| = 1/2)
  sums over pixels: sum(e_terms) + (D + c) u sum|terms|; means of them divide both and add u |mean|
  products and the two BatchNorm backward forms: the product rule on |factors| and their bounds, + c u of the terms
  running statistics: c u (|old| + mom |new|) + mom (dm or dv cnt / (cnt - 1))
  gradients: + u |initial + gradient| for the final add; bf16 y: + half a bf16 ulp at |y| + bound.
Eval-mode rho = 1 / sqrtf(rv + eps) is c u rho off, the running mean is exact.

D, the serial length of the fp32 chain behind each sum over pixels, read from cn_pretime.hip (tiles = the pixel tiles of
128 a persistent block walks: ceil(ceil(P / 128) / maxb), maxb = 512 for the generic kernel and for PASS 3 / 4 / 5 of
the register variant, 1008 for its PASS 0 / 1 / 2, 768 for the C = 4 output pass; ns = ceil(Tp / 2) wave steps of a row;
TREE = 6 for the DPP / butterfly wave stage (pt_half_sum + row_bcast, pt_hsum16: 5 or 6 additions on a term's path);
tiles more for the ds_add_f32 of a wave's LDS accumulator, once per tile; WAVES = 3 for the four waves' rows; the
two-level ticket sums in double: + 0; + 2 for the roundings of the summed product itself):
  BatchNorm3d statistics (PASS 0), dg3 / db3 (PASS 4):  ns + TREE + tiles + WAVES + 2     a lane sums its row's steps first
  BatchNorm2d statistics (PASS 1), dg2 / db2 / dgL / dbL (PASS 3):  TREE + tiles + WAVES + 2
  dwb (PASS 4): 32 tiles + WAVES + 2     the MFMA accumulator takes a wave's 32 pixels per tile, tile after tile
  dwa (PASS 5): ns tiles + TREE + tiles + WAVES + 2     the register variant keeps its sums in registers across tiles
None of these constants is fitted to a GPU result.

`mut` names one deliberate defect (MUTATIONS) for tests/test_pretime_ref.py: the mutated VALUES must leave the bounds of
the unmutated reference."""
import functools
import math

import torch

U = 2.0 ** -24
C_CHAIN = 16.0
L_SILU = 1.1
L_DSILU = 0.5
TREE = 6
WAVES = 3
PXB = 128
BR = (3, 5)
BN_EPS, BN_MOM, LN_EPS = 1e-5, 0.1, 1e-5

MUTATIONS = ("tap5", "odd_tail", "biased", "eps_outside", "c_swap", "dsilu_sigmoid", "ln_cp", "swap_wb", "overwrite",
             "eval_keeps_means")
STAT_NAMES = [f"{n}_{k}" for k in BR for n in ("mean3", "rstd3", "mean2", "rstd2")]
RUN_NAMES = [f"{n}_{k}" for k in BR for n in ("rm3", "rv3", "rm2", "rv2")]
GRAD_NAMES = [f"{n}_{k}" for k in BR for n in ("dwa", "dwb", "dg3", "db3", "dg2", "db2")] + ["dgL", "dbL"]
# the groups the summary reports a worst ratio for
GROUPS = {"stats": STAT_NAMES, "running": RUN_NAMES, "dwa": ["dwa_3", "dwa_5"], "dwb": ["dwb_3", "dwb_5"],
          "bn_grads": [f"{n}_{k}" for k in BR for n in ("dg3", "db3", "dg2", "db2")], "ln_grads": ["dgL", "dbL"]}


def ceil32(v):
    return (v + 31) & ~31


def is_reg(PASS, C, T, Cout, generic=False):
    """pt_reg of cn_pretime.hip (generic: CN_PRETIME_REG=0, or a batch stride beyond 32-bit byte offsets)."""
    if generic or Cout > 32:
        return False
    return (C == 3 and T == 12) or (PASS == 2 and C == 4 and T == 25)


def tiles(P, PASS, C, T, Cout, generic=False):
    """Pixel tiles one persistent block walks (pt_launch: equal shares have the same ceiling)."""
    ntb = -(-P // PXB)
    if not is_reg(PASS, C, T, Cout, generic):
        maxb = 512
    elif PASS >= 3:
        maxb = 512
    else:
        maxb = 768 if C == 4 else 1008
    return -(-ntb // maxb)


def depths(P, C, T, Cout, k, generic=False):
    ns = (T - k + 2) // 2
    t = [tiles(P, ps, C, T, Cout, generic) for ps in range(6)]
    return {"bn3": ns + TREE + t[0] + WAVES + 2, "bn2": TREE + t[1] + WAVES + 2, "p3": TREE + t[3] + WAVES + 2,
            "bn3b": ns + TREE + t[4] + WAVES + 2, "dwb": 32 * t[4] + WAVES + 2,
            "dwa": ns * t[5] + TREE + t[5] + WAVES + 2}


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def silu(x):
    return x * sigmoid(x)


def dsilu(x):
    s = sigmoid(x)
    return s * (1.0 + x * (1.0 - s))


def half_ulp16(y, slack):
    mag = y.abs() + slack
    _, e = torch.frexp(mag)
    return torch.where(mag == 0, torch.zeros_like(mag), torch.ldexp(torch.ones_like(mag), e - 9))


def _e_dsilu(z, ez):
    s = sigmoid(z)
    return (C_CHAIN + z.abs()) * U * s * (1.0 + z.abs() * (1.0 - s)) + L_DSILU * ez


def _psum(val, err, dims, D):
    return val.sum(dims), err.sum(dims) + (D + C_CHAIN) * U * val.abs().sum(dims)


def _bcast(v, nd):
    return v.reshape((1, -1) + (1,) * (nd - 2))


def _norm(h, eh, p, tag, training, eps, mom, D, mut, out):
    """BatchNorm of h [B, ch, ...] over every other axis -> (xh, e_xh, rho, e_rho); statistics into `out`."""
    nd = h.dim()
    dims = (0,) + tuple(range(2, nd))
    cnt = h.numel() // h.shape[1]
    rm, rv = p["rm" + tag].double(), p["rv" + tag].double()
    k = p["k"]
    if training:
        m = h.mean(dims)
        d = h - _bcast(m, nd)
        var = (d * d).mean(dims)
        s = var.sqrt()
        dm = D * U * (m.abs() + s) + eh.mean(dims)
        dv = 3 * D * U * (m * m + var) + 2 * (d.abs() * eh).mean(dims)
        rho = 1.0 / (var.sqrt() + eps) if mut == "eps_outside" else 1.0 / (var + eps).sqrt()
        e_rho = 2 * U * rho + (1.0 / ((var - dv).clamp_min(0) + eps).sqrt() - 1.0 / (var + eps).sqrt())
        unb = var if (mut == "biased" or cnt <= 1) else var * cnt / (cnt - 1.0)
        f = 1.0 if cnt <= 1 else cnt / (cnt - 1.0)
        out[f"mean{tag}_{k}"] = (m, dm + U * m.abs())
        out[f"rstd{tag}_{k}"] = (rho, e_rho)
        out[f"rm{tag}_{k}"] = ((1 - mom) * rm + mom * m, C_CHAIN * U * (rm.abs() + mom * m.abs()) + mom * dm)
        out[f"rv{tag}_{k}"] = ((1 - mom) * rv + mom * unb, C_CHAIN * U * (rv.abs() + mom * var * f) + mom * dv * f)
        dm = dm + U * m.abs()
    else:
        m, dm = rm, torch.zeros_like(rm)
        rho = 1.0 / (rv.sqrt() + eps) if mut == "eps_outside" else 1.0 / (rv + eps).sqrt()
        e_rho = C_CHAIN * U * rho
        d = h - _bcast(m, nd)
        out[f"rm{tag}_{k}"] = (rm, torch.zeros_like(rm))
        out[f"rv{tag}_{k}"] = (rv, torch.zeros_like(rv))
    rb, eb, mb = _bcast(rho, nd), _bcast(e_rho, nd), _bcast(m, nd)
    xh = d * rb
    e_xh = C_CHAIN * U * rb * (h.abs() + mb.abs()) + rb * (eh + _bcast(dm, nd)) + d.abs() * eb
    return xh, e_xh, rho, e_rho


def _affine_silu(xh, e_xh, g, b):
    nd = xh.dim()
    g, b = _bcast(g.double(), nd), _bcast(b.double(), nd)
    z = g * xh + b
    ez = C_CHAIN * U * ((g * xh).abs() + b.abs()) + g.abs() * e_xh
    a = silu(z)
    ea = (C_CHAIN + z.abs()) * U * a.abs() + L_SILU * ez
    return z, ez, a, ea


def _bn_back(dv, e_dv, xh, e_xh, g, rho, e_rho, dims, cnt, D, keep, mut):
    """Parameter sums and the input gradient of one BatchNorm: (dgamma, dbeta, dr), each (value, bound)."""
    nd = dv.dim()
    db, e_db = _psum(dv, e_dv, dims, D)
    t = dv * xh
    dg, e_dg = _psum(t, e_dv * xh.abs() + dv.abs() * e_xh + U * t.abs(), dims, D)
    if keep:
        c0, c1 = db / cnt, dg / cnt
        e0, e1 = e_db / cnt + U * c0.abs(), e_dg / cnt + U * c1.abs()
    else:
        c0, c1, e0, e1 = torch.zeros_like(db), torch.zeros_like(dg), torch.zeros_like(db), torch.zeros_like(dg)
    c0b, c1b, e0b, e1b = _bcast(c0, nd), _bcast(c1, nd), _bcast(e0, nd), _bcast(e1, nd)
    q_true = dv - c0b - xh * c1b
    e_q = e_dv + e0b + e_xh * c1b.abs() + xh.abs() * e1b + C_CHAIN * U * (dv.abs() + c0b.abs() + (xh * c1b).abs())
    q = dv - c1b - xh * c0b if mut == "c_swap" else q_true
    gb, rb, eb = _bcast(g.double(), nd), _bcast(rho, nd), _bcast(e_rho, nd)
    dr = gb * rb * q
    e_dr = gb.abs() * (rb * e_q + q_true.abs() * eb) + C_CHAIN * U * (gb * rb * q_true).abs()
    return (dg, e_dg), (db, e_db), (dr, e_dr)


def reference(x, prm, dy=None, training=True, mut=None, grads0=None, bf16=False, generic=False,
              eps=(BN_EPS, BN_EPS, LN_EPS), mom=(BN_MOM, BN_MOM)):
    """x [B, C, T, HW]; prm {"br": [branch dicts of wa, wb, g3, b3, rm3, rv3, g2, b2, rm2, rv2], "gL", "bL"}; dy
    [B, Cout, HW] or None (forward only). Returns {name: (float64 value, float64 bound)} for y, STAT_NAMES (training
    forward), RUN_NAMES and, with dy, GRAD_NAMES (`grads0`: what the gradient buffers held, default zero)."""
    x = x.double()
    B, C, T, L = x.shape
    P = B * L
    Cout = prm["gL"].numel()
    out, saved = {}, []
    uu, e_uu = 0.0, 0.0
    for bi, k in enumerate(BR):
        p = dict(prm["br"][bi], k=k)
        D = depths(P, C, T, Cout, k, generic)
        Tp = T - k + 1
        wa, wb = p["wa"].double(), p["wb"].double()
        win = x.unfold(2, k, 1)  # [B, C, Tp, L, k]
        kk = k - 1 if (mut == "tap5" and k == 5) else k
        h = torch.einsum("ocd,bctld->botl", wa[..., :kk], win[..., :kk])
        eh = (C * k + 2) * U * torch.einsum("ocd,bctld->botl", wa.abs(), win.abs())
        xh, e_xh, rho3, e_rho3 = _norm(h, eh, p, "3", training, eps[0], mom[0], D["bn3"], mut, out)
        z, ez, a, ea = _affine_silu(xh, e_xh, p["g3"], p["b3"])
        wbm = wb
        if mut == "odd_tail" and Tp % 2 == 1:
            wbm = wb.clone()
            wbm[:, C - 1, Tp - 1] = 0
        if mut == "swap_wb":
            other = prm["br"][1 - bi]["wb"].double()
            n = min(Tp, other.shape[2])
            wbm = wb.clone()
            wbm[1] = 0
            wbm[1, :, :n] = other[1, :, :n]
        r = torch.einsum("oct,bctl->bol", wbm, a)
        er = (C * Tp + C_CHAIN) * U * torch.einsum("oct,bctl->bol", wb.abs(), a.abs()) + \
            torch.einsum("oct,bctl->bol", wb.abs(), ea)
        rh, e_rh, rho2, e_rho2 = _norm(r, er, p, "2", training, eps[1], mom[1], D["bn2"], mut, out)
        v, ev, s, es = _affine_silu(rh, e_rh, p["g2"], p["b2"])
        uu, e_uu = uu + s, e_uu + es
        saved.append((p, D, xh, e_xh, rho3, e_rho3, z, ez, a, ea, rh, e_rh, rho2, e_rho2, v, ev))
    e_uu = e_uu + U * uu.abs()
    # LayerNorm over Cout
    gL, bL = prm["gL"].double()[None, :, None], prm["bL"].double()[None, :, None]
    NL = ceil32(Cout) if mut == "ln_cp" else Cout
    DL = 16 * (2 if Cout > 32 else 1) + 1
    mL = uu.sum(1, keepdim=True) / NL
    e_mL = e_uu.mean(1, keepdim=True) + DL * U * uu.abs().mean(1, keepdim=True)
    d = uu - mL
    d_true = uu - uu.mean(1, keepdim=True)
    e_d = e_uu + e_mL + U * d_true.abs()
    varL = (d * d).sum(1, keepdim=True) / NL
    varL_true = (d_true * d_true).mean(1, keepdim=True)
    e_varL = 2 * (d_true.abs() * e_d).mean(1, keepdim=True) + (DL + 2) * U * varL_true
    rL = 1.0 / (varL + eps[2]).sqrt()
    rL_true = 1.0 / (varL_true + eps[2]).sqrt()
    e_rL = C_CHAIN * U * rL_true + (1.0 / ((varL_true - e_varL).clamp_min(0) + eps[2]).sqrt() - rL_true)
    uhat = d * rL
    uhat_true = d_true * rL_true
    e_uhat = rL_true * e_d + d_true.abs() * e_rL + C_CHAIN * U * uhat_true.abs()
    y = gL * uhat + bL
    e_y = C_CHAIN * U * ((gL * uhat_true).abs() + bL.abs()) + gL.abs() * e_uhat
    if bf16:
        e_y = e_y + half_ulp16(gL * uhat_true + bL, e_y)
    out["y"] = (y, e_y)
    if dy is None:
        return out

    dy = dy.double()
    D3 = saved[0][1]["p3"]
    gj = dy * gL
    e_gj = U * gj.abs()
    s1 = gj.sum(1, keepdim=True) / NL
    e_s1 = e_gj.mean(1, keepdim=True) + DL * U * gj.abs().mean(1, keepdim=True)
    s2 = (gj * uhat).sum(1, keepdim=True) / NL
    e_s2 = (e_gj * uhat.abs() + gj.abs() * e_uhat).mean(1, keepdim=True) + (DL + 2) * U * (gj * uhat).abs().mean(1, keepdim=True)
    t = gj - s1 - uhat * s2
    e_t = e_gj + e_s1 + e_uhat * s2.abs() + uhat.abs() * e_s2 + C_CHAIN * U * (gj.abs() + s1.abs() + (uhat * s2).abs())
    du = rL * t
    e_du = rL * e_t + t.abs() * e_rL + C_CHAIN * U * du.abs()
    g = {}
    g["dgL"] = _psum(dy * uhat, dy.abs() * e_uhat + U * (dy * uhat).abs(), (0, 2), D3)
    g["dbL"] = _psum(dy, torch.zeros_like(dy), (0, 2), D3)
    keep = training or mut == "eval_keeps_means"
    for bi, k in enumerate(BR):
        p, D, xh, e_xh, rho3, e_rho3, z, ez, a, ea, rh, e_rh, rho2, e_rho2, v, ev = saved[bi]
        wb = p["wb"].double()
        Tp = T - k + 1
        sg = sigmoid(v) if mut == "dsilu_sigmoid" else dsilu(v)
        dv = du * sg
        e_dv = e_du * dsilu(v).abs() + du.abs() * _e_dsilu(v, ev) + U * (du * dsilu(v)).abs()
        g[f"dg2_{k}"], g[f"db2_{k}"], (dr, e_dr) = _bn_back(dv, e_dv, rh, e_rh, p["g2"], rho2, e_rho2, (0, 2), P,
                                                           D["p3"], keep, mut)
        tw = torch.einsum("bol,bctl->oct", dr, a)
        e_tw = torch.einsum("bol,bctl->oct", e_dr, a.abs()) + torch.einsum("bol,bctl->oct", dr.abs(), ea) + \
            (D["dwb"] + C_CHAIN) * U * torch.einsum("bol,bctl->oct", dr.abs(), a.abs())
        g[f"dwb_{k}"] = (tw, e_tw)
        da = torch.einsum("oct,bol->bctl", wb, dr)
        e_da = torch.einsum("oct,bol->bctl", wb.abs(), e_dr) + \
            (ceil32(Cout) + C_CHAIN) * U * torch.einsum("oct,bol->bctl", wb.abs(), dr.abs())
        sgz = sigmoid(z) if mut == "dsilu_sigmoid" else dsilu(z)
        dz = da * sgz
        e_dz = e_da * dsilu(z).abs() + da.abs() * _e_dsilu(z, ez) + U * (da * dsilu(z)).abs()
        g[f"dg3_{k}"], g[f"db3_{k}"], (dh, e_dh) = _bn_back(dz, e_dz, xh, e_xh, p["g3"], rho3, e_rho3, (0, 2, 3),
                                                           P * Tp, D["bn3b"], keep, mut)
        win = x.unfold(2, k, 1)
        ta = torch.einsum("botl,bctld->ocd", dh, win)
        e_ta = torch.einsum("botl,bctld->ocd", e_dh, win.abs()) + \
            (D["dwa"] + C_CHAIN) * U * torch.einsum("botl,bctld->ocd", dh.abs(), win.abs())
        g[f"dwa_{k}"] = (ta, e_ta)
    for n in GRAD_NAMES:
        val, err = g[n]
        g0 = torch.zeros_like(val) if grads0 is None else grads0[n].double().reshape(val.shape)
        tot = val + g0
        out[n] = (val if mut == "overwrite" else tot, err + U * tot.abs())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# problems shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------

def make_problem(B, C, T, HW, Cout, seed=0, bf16=False):
    """Deterministic inputs: weights and dy of order 1, input channel 0 with a mean of 2 (the E[h^2] - m^2 cancellation
    of the statistics is live), the last first-convolution row scaled by 0.05 and the first second-convolution row by 0.02
    with running variances to match (standard deviations of 0.04 - 0.08, where eps inside or outside the root matters), dy
    with a per-channel offset of order 1 (sums over many pixels then grow like P, as their bounds do, instead of
    cancelling like sqrt(P)), non-trivial affine parameters and running statistics. Everything fp32 (dy rounded to
    bf16 first when bf16)."""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(B, C, T, HW)
    x[:, 0] += 2.0
    prm = {"br": []}
    for k in BR:
        Tp = T - k + 1
        prm["br"].append({
            "wa": rn(C, C, k) / math.sqrt(C * k) * 1.5, "wb": rn(Cout, C, Tp) / math.sqrt(C * Tp) * 2.0,
            "g3": 1 + 0.3 * rn(C), "b3": 0.3 * rn(C), "rm3": 0.5 * rn(C), "rv3": 0.5 + torch.rand(C, generator=g),
            "g2": 1 + 0.3 * rn(Cout), "b2": 0.3 * rn(Cout), "rm2": 0.5 * rn(Cout),
            "rv2": 0.5 + torch.rand(Cout, generator=g)})
    for p in prm["br"]:  # one low-variance channel per BatchNorm: there eps inside or outside the square root differs
        p["wa"][C - 1] *= 0.05
        p["rv3"][C - 1] = 0.004
        p["wb"][0] *= 0.02
        p["rv2"][0] = 0.002
    prm["gL"], prm["bL"] = 1 + 0.3 * rn(Cout), 0.3 * rn(Cout)
    dy = rn(B, Cout, HW) + 1.5 * rn(Cout)[None, :, None]
    if bf16:
        dy = dy.to(torch.bfloat16).float()
    shapes = {}
    for k, p in zip(BR, prm["br"]):
        for n, s in (("dwa", p["wa"]), ("dwb", p["wb"]), ("dg3", p["g3"]), ("db3", p["b3"]), ("dg2", p["g2"]), ("db2", p["b2"])):
            shapes[f"{n}_{k}"] = tuple(s.shape)
    shapes["dgL"], shapes["dbL"] = (Cout,), (Cout,)
    g0 = {n: rn(*shapes[n]) for n in GRAD_NAMES}
    return x, prm, dy, g0


@functools.lru_cache(maxsize=8)
def problem(B, C, T, HW, Cout, kind=0, training=True, backward=True, accumulate=False, generic=False, seed=0):
    """(x, prm, dy, grads0 or None, reference dict) of one configuration; shared, never modified."""
    x, prm, dy, g0 = make_problem(B, C, T, HW, Cout, seed, bf16=kind == 1)
    g0 = g0 if accumulate else None
    ref = reference(x, prm, dy if backward else None, training=training, grads0=g0, bf16=kind == 1, generic=generic)
    return x, prm, dy, g0, ref


def to_oracle(prm, C, T, dtype=torch.float64):
    """The oracle module holding prm (a fresh module: its running statistics are updated by a training forward)."""
    from oracle import towerunet_oracle as O

    Cout = prm["gL"].numel()
    mod = O.PreTimeReduction(C, T, Cout).to(dtype)
    with torch.no_grad():
        for conv, p in zip((mod.conv3, mod.conv5), prm["br"]):
            s = conv.seq
            s[0].weight.copy_(p["wa"][..., None, None])
            s[3].weight.copy_(p["wb"][..., None, None])
            for bn, t in ((s[1], "3"), (s[5], "2")):
                bn.weight.copy_(p["g" + t]); bn.bias.copy_(p["b" + t])
                bn.running_mean.copy_(p["rm" + t]); bn.running_var.copy_(p["rv" + t])
                bn.eps, bn.momentum = BN_EPS, BN_MOM
        ln = mod.layer_norm[1]
        ln.weight.copy_(prm["gL"]); ln.bias.copy_(prm["bL"])
        ln.eps = LN_EPS
    return mod


def oracle_tensors(mod):
    """{name: tensor} of the oracle module's gradients (after backward) and running statistics, in the ABI's names."""
    out = {}
    for k, conv in zip(BR, (mod.conv3, mod.conv5)):
        s = conv.seq
        pairs = (("dwa", s[0].weight), ("dwb", s[3].weight), ("dg3", s[1].weight), ("db3", s[1].bias),
                 ("dg2", s[5].weight), ("db2", s[5].bias))
        for n, t in pairs:
            if t.grad is not None:
                out[f"{n}_{k}"] = t.grad.detach().reshape(t.shape[:3] if t.dim() == 5 else t.shape)
        out[f"rm3_{k}"], out[f"rv3_{k}"] = s[1].running_mean.detach(), s[1].running_var.detach()
        out[f"rm2_{k}"], out[f"rv2_{k}"] = s[5].running_mean.detach(), s[5].running_var.detach()
    ln = mod.layer_norm[1]
    if ln.weight.grad is not None:
        out["dgL"], out["dbL"] = ln.weight.grad.detach(), ln.bias.grad.detach()
    return out


def worst_ratio(got, ref, bound, what):
    got = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return worst, err, ratio


def within(got, ref_pair, what, record=None, group=None):
    ref, bound = ref_pair
    worst, err, ratio = worst_ratio(got, ref, bound, what)
    print(f"{what}: worst err/bound {worst:.3f}")
    if record is not None:
        record[group or what] = max(record.get(group or what, 0.0), worst)
    if not worst <= 1.0:
        i = int(ratio.flatten().argmax())
        got = got.detach().double().cpu()
        raise AssertionError(f"{what}: err {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i]):.3e} at flat "
                             f"index {i} (got {float(got.flatten()[i])!r}, ref {float(ref.flatten()[i])!r})")
    return worst


def group_of(name, kind=0):
    if name == "y":
        return "y bf16" if kind else "y fp32"
    for g, names in GROUPS.items():
        if name in names:
            return g
    raise KeyError(name)


# configurations of tests/test_pretime_exact_gpu.py (B, C, T, HW, Cout, kind); the CPU tests walk the same list
CUBES = {"c5t6": (5, 6), "c8t5": (8, 5), "c6t8": (6, 8), "c4t12": (4, 12), "c4t25": (4, 25), "c3t12": (3, 12)}
COUTS = (8, 24, 32)
# (C, T) = (4, 25) is the NE = 3 cube, but no shape with 65 <= C (T - 2) <= 96 fits the gradient pass: PASS 4 keeps
# a[entry][pixel] and dr per wave, wB and the x tile in LDS -- 250 KB at (4, 25), 215 KB or more at every other such
# cube, against 160 KiB -- so cn_pretime_workspace_floats(.., with_backward = 1) answers -1 for all of them, rightly,
# and the engine keeps its generic path there. The cube runs training forward, statistics and inference; the refusal
# is asserted (test_ne3_gradient_pass_has_no_servable_shape walks every such cube).
NO_BACKWARD = ("c4t25",)


def dispatch_cases():
    """Every cube at every Cout; the output kind alternates so that each cube and each Cout meets both kinds. B HW = 2 x
    173: three tiles, the last partial, a batch boundary inside a wave."""
    cases = {}
    for i, (name, (C, T)) in enumerate(CUBES.items()):
        for j, Cout in enumerate(COUTS):
            kind = (i + j) % 2
            cases[f"{name}-o{Cout}-{'bf16' if kind else 'f32'}"] = (2, C, T, 173, Cout, kind)
    return cases


WIDE_CASES = {"c3t12-o40-f32": (2, 3, 12, 173, 40, 0), "c5t6-o56-bf16": (2, 5, 6, 173, 56, 1),
              "c4t12-o64-f32": (2, 4, 12, 173, 64, 0)}
EVAL_CASES = {"c3t12-o32-f32": (2, 3, 12, 173, 32, 0), "c6t8-o24-bf16": (2, 6, 8, 173, 24, 1)}
ACCUM_CASES = {"c3t12-o24-bf16": (2, 3, 12, 173, 24, 1), "c5t6-o8-f32": (2, 5, 6, 173, 8, 0)}
EDGE_PIXELS = {2: (2, 1), 31: (1, 31), 33: (3, 11), 127: (1, 127), 129: (3, 43)}  # B HW -> (B, HW)
EDGE_CUBES = {"c3t12": (3, 12), "c5t6": (5, 6)}
TILE_CASES = {"reg-c3t12": (3, 3, 12, 43011, 8, 0, True),     # P = 129033 > 1008 * 128, P % 128 = 9
              "inf-c4t25": (3, 4, 25, 32771, 8, 0, False),    # P = 98313 > 768 * 128, P % 128 = 9 (inference)
              "gen-c5t6": (3, 5, 6, 21849, 8, 1, True)}       # P = 65547 > 512 * 128, P % 128 = 11
OFFSET_CASE = (3, 3, 12, 211, 8, 0)  # the 32-bit offset cases: three cubes far apart in one large buffer
