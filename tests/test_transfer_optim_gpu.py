"""Segmented optimizer kernels (cn_grad_sumsq_seg_f32 / cn_adamw_step_seg_f32: frozen parameters) against a float64
restatement of torch.optim.AdamW after clip_grad_norm_ over the parameters that have a gradient. Elements outside the
segments must keep p, exp_avg and exp_avg_sq bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32_EPS = 2.0 ** -23
GRAD_REL = 1e-5  # the tolerance of tests/test_loss_optim_gpu.py::_adamw_run


def _adamw_seg_ref(p, g, m, v, segs, lr, b1, b2, eps, wd, scale, max_norm):
    """torch AdamW per parameter (each segment with its own step) after clip_grad_norm_ over the segments."""
    idx = torch.cat([torch.arange(o, o + n) for o, n, _ in segs])
    g = g * scale
    coef = 1.0
    if max_norm is not None:
        coef = min(1.0, max_norm / (float(g[idx].norm()) + 1e-6))
    p, m, v = p.clone(), m.clone(), v.clone()
    for o, n, st in segs:
        sl = slice(o, o + n)
        gi = g[sl] * coef
        p[sl] = p[sl] * (1.0 - lr * wd)
        m[sl] = b1 * m[sl] + (1.0 - b1) * gi
        v[sl] = b2 * v[sl] + (1.0 - b2) * gi * gi
        bc1, bc2 = 1.0 - b1 ** st, 1.0 - b2 ** st
        p[sl] = p[sl] - (lr / bc1) * m[sl] / (v[sl].sqrt() / math.sqrt(bc2) + eps)
    return p, m, v, idx


def _seg_call(p, g, m, v, segs, lr, b1, wd, scale, max_norm, sumsq, step_add=0, eps=1e-4, b2=0.98):
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    raw, chunks = E.segment_table([(o, n, st - step_add) for o, n, st in segs])
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda() if raw else torch.zeros(1, dtype=torch.uint8,
                                                                                                  device="cuda")
    n = p.numel()
    if max_norm is not None:
        _lib.call("cn_grad_sumsq_seg_f32", g.data_ptr(), n, table.data_ptr(), len(segs), chunks, sumsq.data_ptr(),
                  E._stream())
    _lib.call("cn_adamw_step_seg_f32", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, table.data_ptr(),
              len(segs), chunks, step_add, float(lr), float(b1), b2, eps, float(wd), float(scale),
              sumsq.data_ptr() if max_norm is not None else None, float(max_norm) if max_norm is not None else 0.0,
              E._stream())
    torch.cuda.synchronize()


def _check_step(p, m, v, p0, m0, v0, g, segs, lr, b1, wd, scale, max_norm, what, eps=1e-4, b2=0.98):
    f = lambda x: float(torch.tensor(x, dtype=torch.float32))
    pr, mr, vr, idx = _adamw_seg_ref(p0, g.double(), m0, v0, segs, f(lr), f(b1), f(b2), f(eps), f(wd), f(scale),
                                     max_norm)
    pc, mc, vc = p.cpu(), m.cpu(), v.cpu()
    inside = torch.zeros(p.numel(), dtype=torch.bool)
    inside[idx] = True
    out = ~inside
    # outside the segments nothing moves, bit for bit
    assert torch.equal(pc[out], p0.float()[out]), what
    assert torch.equal(mc[out], m0.float()[out]), what
    assert torch.equal(vc[out], v0.float()[out]), what
    pd, md, vd = pc.double()[idx], mc.double()[idx], vc.double()[idx]
    dp = (pr - p0)[idx]
    perr = ((pd - pr[idx]).abs() - 2 * F32_EPS * pr[idx].abs()).clamp(min=0).max()
    for k, err, sc in (("dp", float(perr), float(dp.abs().max())), ("m", float((md - mr[idx]).abs().max()),
                                                                     float(mr[idx].abs().max())),
                       ("v", float((vd - vr[idx]).abs().max()), float(vr[idx].abs().max()))):
        assert err <= GRAD_REL * max(sc, 1e-30), f"{what} {k}: err {err:.3e} > {GRAD_REL:.0e} * {sc:.3e}"


def _state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.02
    m = torch.randn(n, generator=gen) * 1e-3
    v = torch.rand(n, generator=gen) * 1e-5
    return gen, p.cuda(), m.cuda(), v.cuda()


def _grad(n, gen, gnorm):
    g = torch.randn(n, generator=gen)
    g[torch.rand(n, generator=gen) < 0.1] = 0.0
    return g * (gnorm / float(g.norm()))


def _many_short(n_total, gen):
    """300+ segments, lengths 1-3 mixed with longer ones, gaps between them, assorted step counts."""
    segs, o = [], 1
    k = 0
    while o < n_total - 5000 and len(segs) < 340:
        ln = [1, 2, 3, 1, 17, 3, 2, 4096 + 5][k % 8]
        segs.append((o, ln, 1 + (k * 7) % 11))
        o += ln + 1 + int(torch.randint(0, 9, (1,), generator=gen))
        k += 1
    return segs


CASES = {
    # id: (n, segments kind, grad_scale, max_norm, weight_decay, gradient norm)
    "past_grid_cap_clip_active": (2048 * 4096 + 4099, "big", 1.0, 1.0, 1e-3, 7.0),
    "many_short_clip_active": (200_000, "short", 1.0, 1.0, 1e-3, 7.0),
    "many_short_clip_inactive": (200_000, "short", 1.0, 1.0, 0.0, 0.4),
    "ddp_grad_scale": (200_000, "short", 0.5, 1.0, 1e-3, 5.0),
    "no_clip": (200_000, "short", 1.0, None, 1e-3, 7.0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_segmented_adamw_matches_float64_torch(case):
    n, kind, scale, max_norm, wd, gnorm = CASES[case]
    gen, p, m, v = _state(n, 77 + len(case))
    if kind == "big":  # one segment past the 2048-block grid cap of the update (grid-stride over chunks) + small ones
        segs = [(3, n - 4003, 4), (n - 3996, 1, 1), (n - 3990, 3, 9)]
    else:
        segs = _many_short(n, gen)
    assert len(segs) >= 3 and (kind == "big" or len(segs) >= 300)
    g = _grad(n, gen, gnorm).cuda()
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    p0, m0, v0 = p.cpu().double(), m.cpu().double(), v.cpu().double()
    _seg_call(p, g, m, v, segs, 3e-3, 0.9, wd, scale, max_norm, sumsq)
    _check_step(p, m, v, p0, m0, v0, g.cpu(), segs, 3e-3, 0.9, wd, scale, max_norm, case)
    if max_norm is not None:
        idx = torch.cat([torch.arange(o, o + ln) for o, ln, _ in segs])
        ref = float((g.cpu().double()[idx] ** 2).sum())
        assert abs(float(sumsq.item()) - ref) <= 1e-9 * ref, (float(sumsq.item()), ref)


def test_sumsq_seg_against_float64_sum():
    from cultionet_amd import _lib
    from cultionet_amd import engine as E

    n = 2048 * 4096 + 777
    gen = torch.Generator().manual_seed(5)
    g = torch.randn(n, generator=gen)
    segs = _many_short(n, gen)[:-1] + [(n - 4000, 3999, 1)]
    raw, chunks = E.segment_table(segs)
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    out = torch.full((1,), 123.0, dtype=torch.float64, device="cuda")  # zeroed by the call
    gd = g.cuda()
    _lib.call("cn_grad_sumsq_seg_f32", gd.data_ptr(), n, table.data_ptr(), len(segs), chunks, out.data_ptr(),
              E._stream())
    torch.cuda.synchronize()
    idx = torch.cat([torch.arange(o, o + ln) for o, ln, _ in segs])
    ref = float((g.double()[idx] ** 2).sum())
    assert abs(float(out.item()) - ref) <= 1e-9 * ref
    # no segments: zero, nothing launched
    _lib.call("cn_grad_sumsq_seg_f32", gd.data_ptr(), n, table.data_ptr(), 0, 0, out.data_ptr(), E._stream())
    torch.cuda.synchronize()
    assert float(out.item()) == 0.0


def test_gradual_unfreeze_schedule_with_per_parameter_steps():
    """Five steps over four 'parameters' whose trainable set changes: a parameter unfrozen later starts its own bias
    correction at 1, one frozen and unfrozen again resumes its exp_avg / exp_avg_sq / step; the table is reused across
    steps with step_add (the host's cache while the set is unchanged)."""
    sizes = [1000, 3, 5000, 257]
    offs, n = [], 0
    for s in sizes:
        offs.append(n)
        n += (s + 3) // 4 * 4
    gen, p, m, v = _state(n, 11)
    m.zero_()
    v.zero_()
    sched = [(True, False, False, True), (True, False, False, True), (True, True, False, True),
             (False, True, True, True), (True, True, True, False)]
    steps = [0] * 4
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    from cultionet_amd import engine as E

    prev_mask, built = None, None
    for k, mask in enumerate(sched):
        for i, t in enumerate(mask):
            steps[i] += int(t)
        segs = E.trainable_segments(offs, sizes, mask, steps)
        if mask == prev_mask:  # same set: the kernel adds the steps since the table was built
            step_add = k - built
        else:
            step_add, built = 0, k
        prev_mask = mask
        g = torch.zeros(n)
        for i, t in enumerate(mask):
            if t:
                g[offs[i]:offs[i] + sizes[i]] = _grad(sizes[i], gen, 2.0)
        g = g.cuda()
        p0, m0, v0 = p.cpu().double(), m.cpu().double(), v.cpu().double()
        lr, b1 = 1e-2 / (k + 1), 0.95 - 0.01 * k  # a OneCycle-like lr / beta1
        _seg_call(p, g, m, v, segs, lr, b1, 1e-3, 1.0, 1.0, sumsq, step_add=step_add)
        _check_step(p, m, v, p0, m0, v0, g.cpu(), segs, lr, b1, 1e-3, 1.0, 1.0, f"step {k}")
    assert steps == [4, 3, 2, 4]
