"""The fused PreTimeReduction kernels (cultionet_amd/csrc/cn_pretime.hip) through the C ABI (cn_pretime_fwd_f32,
cn_pretime_bwd_f32) against the float64 restatement of tests/pretime_ref.py: every output -- y, the eight saved
statistics, the updated running statistics, the fourteen parameter gradients -- per element against a bound built from
the magnitudes that feed that element. No floor, no max|ref| scale. tests/test_pretime_ref.py pins the restatement to
the oracle module, shows an fp32 evaluation inside the bounds and ten deliberate defects outside them.

Every tensor a kernel writes (and dy, the parameters and the workspace) sits between guard runs, and inside wider buffers
where a stride allows it, filled with a NaN pattern that must come back bit for bit after every call; the ticket
counters at the head of the workspace must be zero again; every shape is first confirmed with
cn_pretime_workspace_floats. Each check prints its worst err/bound (run with -s).

The constants of the bound, from the kernel's code (the full forms are in the docstring of tests/pretime_ref.py):
  u = 2^-24. c = 16 roundings for an element's own chain, the constant of tests/test_norm_gpu.py. The longest chain of a
  stage is the activation: `h * rho + off` (one FMA, with off = -mu * rho rounded twice in the pack kernel / finisher),
  `g3 * (..) + b3` (1), pt_sigmoid: the product by -log2(e) (1), v_exp_f32 (1 ulp = 2 u), 1 + e (1), v_rcp_f32 (1 ulp =
  2 u), x * s (1): 11; pt_silu_grad adds 3. The rounding of the exp2 argument is |z| u relative in e, hence (c + |z|) u.
  First convolutions: two FMA chains h0 / h1 over the C k window and h0 + h1: (C k + 2) u sum|wa||x| (the padded
  channels of CMAX carry zero weights). Second convolutions: one v_mfma_f32_32x32x2_f32 accumulator walks all C Tp
  entries of a branch: (C Tp + c) u sum|wb||a|. da = W^T dr walks the 16 MT accumulator registers of dr, two couts per
  step: (CP + c) u sum|wb||dr|. LayerNorm: m, var, s1, s2 are sums over a lane's 16 MT registers and one __shfl_xor:
  D_L = 16 MT + 1; the variance is two-pass (no cancellation term).
  Sums over pixels, D u sum|terms| with D the serial fp32 length (ns = ceil(Tp / 2) wave steps of a row; tiles = tiles of
  128 pixels per persistent block = ceil(ceil(P / 128) / maxb) with maxb of pt_launch: 512, 1008 for PASS 0 / 1 / 2 of
  the register variant, 768 for the C = 4 output pass; TREE = 6: cn_wave_sum_to_lane63 / pt_hsum16 put 5 - 6 additions on
  a term's path; + tiles: one ds_add_f32 into the wave's LDS accumulator per tile; WAVES = 3: the four waves' rows added
  in cn_t2_store's argument; the two-level ticket and the finish are double: + 0; + 2: the roundings of the summed product):
    PASS 0 (BatchNorm3d statistics), PASS 4 (dg3, db3): ns + TREE + tiles + WAVES + 2    `s += h; q += h * h` per row
    PASS 1 (BatchNorm2d statistics), PASS 3 (dg2, db2, dgL, dbL): TREE + tiles + WAVES + 2
    PASS 4 dwb: 32 tiles + WAVES + 2    accW takes a wave's 32 pixels per tile through 16 K = 2 MFMA steps, tile after tile
    PASS 5 dwa: ns tiles + TREE + tiles + WAVES + 2    gp3 / gp5 of the register variant live across the block's tiles
  Batch variances are E[x^2] - m^2 in the finisher: 3 D u (m^2 + var), as in tests/test_norm_gpu.py; rho from it exactly,
  (max(var - dv, 0) + eps)^-1/2 - rho. bf16 y: half a bf16 ulp at |y| + bound; bf16 dy is rounded before the reference
  runs. Accumulation: u |initial + gradient| for the final `+=`.

Dispatch paths and the tests that launch them (read off pt_launch / pt_reg / pt_cmax / pt_ne; c5t6 = (C, T) = (5, 6)):
  CMAX = 8, NE = 1: test_dispatch[c5t6-*], [c8t5-*]        CMAX = 8, NE = 2: test_dispatch[c6t8-*]
  CMAX = 4, NE = 2: test_dispatch[c4t12-*]
  NE = 3: not launchable. Every cube with 65 <= C (T - 2) <= 96 is refused by the with-backward query because PASS 4
  does not fit 160 KiB of LDS (test_ne3_gradient_pass_has_no_servable_shape); test_dispatch[c4t25-*] runs that cube's
  training forward and statistics (generic PASS 0 / 1, register PASS 2) and asserts the refusal.
  register variant <PASS, 4, 1, 1, 3, 12>: test_dispatch[c3t12-*]; generic kernel on (3, 12): test_generic_kernel_child
  MT = 2 (Cout 40 / 56 / 64), PASS 0 / 1 / 2 and inference: test_wide_outputs; training = 0 backward: test_eval_backward
  accumulation: test_gradients_accumulate; strides: test_strides_bitwise; P of 2 .. 129: test_pixel_edges
  tile += gridDim.x: test_more_tiles_than_blocks[reg-c3t12] (1008 / 512 blocks), [inf-c4t25] (<2, 4, 1, 1, 4, 25>, 768
  blocks), [gen-c5t6] (512 blocks); vo / vo1 past 2^31 and the host switch to the generic kernel: test_offsets_32bit.

Worst err/bound (GPU: measured on an MI355X with this file; fp32: the CPU evaluation of tests/test_pretime_ref.py):
                        GPU      fp32 (CPU)
  y fp32                0.0048   0.0052
  y bf16                0.962    0.962     (the bf16 rounding itself: half an ulp is the bound's leading term)
  saved statistics      0.033    0.031
  running statistics    0.077    0.077
  dwa                   < 5e-5   1e-4
  dwb                   5e-4     1e-3
  BatchNorm gradients   4e-4     2e-4
  LayerNorm gradients   0.060    0.861     (dbL over 129 033 pixels: the CPU's fp32 sum is longer than the kernel's D)
The gradient bounds are worst-case sums of absolute terms through two normalisations and sit three orders above what
either evaluation shows; every mutation of tests/test_pretime_ref.py still leaves them. The file takes 8 s of wall time.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import pretime_ref as R
from conv_exact_worker import part
from route_ledger import Routes, case_id

pytestmark = pytest.mark.gpu

PAT32 = 0x7FC0BEEF  # a quiet NaN with a payload
PAT16 = 0x7FC1
GUARD = 32
BN = (R.BN_EPS, R.BN_MOM, R.BN_EPS, R.BN_MOM)
RECORD = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _generic():
    return os.environ.get("CN_PRETIME_REG") == "0"


class Guarded:
    """A tensor inside a larger flat buffer filled with a NaN pattern: `t` is the part a kernel may touch (a strided
    view where `index` says so); everything else must stay as it was."""

    def __init__(self, shape, dtype=torch.float32, index=None, data=None, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.itype, self.pat = (torch.int32, PAT32) if dtype == torch.float32 else (torch.int16, PAT16)
        self.full = torch.empty(n + 2 * GUARD, dtype=dtype, device=_dev())
        self.full.view(self.itype).fill_(self.pat)
        inner = self.full[GUARD:GUARD + n].view(shape)
        self.t = inner if index is None else inner[index]
        self.mask = torch.zeros(n + 2 * GUARD, dtype=torch.bool, device=_dev())
        m = self.mask[GUARD:GUARD + n].view(shape)
        (m if index is None else m[index]).fill_(True)
        if data is not None:
            self.t.copy_(data.to(_dev()).reshape(self.t.shape))
        elif fill is not None:
            self.t.fill_(fill)
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.full.view(self.itype)[~self.mask] == self.pat).all())

    def get(self):
        return self.t.detach().float().cpu().clone()


def _tab(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.ptr if b is not None else None for b in bufs])


class Run:
    """One configuration on the device: buffers, the two ABI calls, the read-back in the reference's names."""

    def __init__(self, case, x, prm, dy, training=True, backward=True, g0=None, strided=False, xpad=0, xbuf=None,
                 routes=None):
        from cultionet_amd import _lib

        self.routes = routes  # tests/route_ledger.py Routes of the calling test, or None

        self.lib = _lib
        B, C, T, HW, Cout, kind = case
        self.case, self.training, self.backward = case, training, backward
        need = _lib.query("cn_pretime_workspace_floats", B, C, T, HW, Cout, 1 if backward else 0)
        assert need > 0, f"the fused kernel refuses {case} (with_backward = {int(backward)})"
        self.bufs = {}
        if xbuf is None:
            self.xbs = C * T * HW + xpad
            xg = Guarded((B, self.xbs), index=(slice(None), slice(0, C * T * HW)), data=x.reshape(B, -1))
            self.bufs["x"], self.xptr = xg, xg.ptr
        else:
            self.xptr, self.xbs = xbuf
        names = ("wa", "wb", "g3", "b3", "rm3", "rv3", "g2", "b2", "rm2", "rv2")
        self.params = []
        for k, p in zip(R.BR, prm["br"]):
            for n in names:
                self.bufs[f"p_{n}_{k}"] = Guarded(tuple(p[n].shape), data=p[n])
                self.params.append(self.bufs[f"p_{n}_{k}"])
        for n in ("gL", "bL"):
            self.bufs["p_" + n] = Guarded((Cout,), data=prm[n])
            self.params.append(self.bufs["p_" + n])
        self.stats = []
        for k in R.BR:
            for n, sz in (("mean3", C), ("rstd3", C), ("mean2", Cout), ("rstd2", Cout)):
                self.bufs[f"{n}_{k}"] = Guarded((sz,))
                self.stats.append(self.bufs[f"{n}_{k}"])
        P = B * HW
        if kind == 0:
            wide = Cout + 5 if strided else Cout
            idx = (slice(None), slice(2, 2 + Cout)) if strided else None
            mk = lambda data=None: Guarded((B, wide, HW), index=idx, data=data)
            self.stride = wide * HW
            dyd = dy
        else:
            wide = Cout + 8 if strided else Cout
            mk = lambda data=None: Guarded((P, wide), torch.bfloat16, index=(slice(None), slice(0, Cout)), data=data)
            self.stride = wide
            dyd = dy.permute(0, 2, 1)
        self.bufs["y"] = mk()
        if backward:
            self.bufs["dy"] = mk(dyd)
            self.grads = []
            for n in R.GRAD_NAMES:
                shape = tuple(g0[n].shape) if g0 is not None else self._gshape(n, prm)
                self.bufs[n] = Guarded(shape, data=g0[n] if g0 is not None else None, fill=None if g0 is not None else 0.0)
                self.grads.append(self.bufs[n])
        self.bufs["ws"] = Guarded((need,), fill=0.0)
        self.need = need
        self.bn = (ctypes.c_float * 4)(*BN)

    @staticmethod
    def _gshape(n, prm):
        if n in ("dgL", "dbL"):
            return tuple(prm["gL"].shape)
        base, k = n.split("_")
        p = prm["br"][R.BR.index(int(k))]
        return tuple(p[{"dwa": "wa", "dwb": "wb", "dg3": "g3", "db3": "b3", "dg2": "g2", "db2": "b2"}[base]].shape)

    def _after(self, what):
        torch.cuda.synchronize()
        for n, b in self.bufs.items():
            assert b.intact(), f"{what}: the guard around {n} was written"
        assert int(self.bufs["ws"].t[:64].view(torch.int32).abs().sum()) == 0, f"{what}: ticket counters not back to zero"

    def forward(self):
        B, C, T, HW, Cout, kind = self.case
        s = torch.cuda.current_stream().cuda_stream
        with part(self.routes, "forward", "training" if self.training else "eval"):
            self.lib.call("cn_pretime_fwd_f32", self.xptr, self.xbs, _tab(self.params), _tab(self.stats),
                          self.bufs["y"].ptr, self.stride, kind, B, C, T, HW, Cout, int(self.training), self.bn, R.LN_EPS,
                          self.bufs["ws"].ptr, self.need, s)
        self._after("forward")
        out = {"y": self._layout(self.bufs["y"].get())}
        for k in R.BR:
            for n in ("rm3", "rv3", "rm2", "rv2"):
                out[f"{n}_{k}"] = self.bufs[f"p_{n}_{k}"].get()
        if self.training:
            for n in R.STAT_NAMES:
                out[n] = self.bufs[n].get()
        return out

    def backward_(self):
        B, C, T, HW, Cout, kind = self.case
        s = torch.cuda.current_stream().cuda_stream
        with part(self.routes, "backward", "training" if self.training else "eval"):
            self.lib.call("cn_pretime_bwd_f32", self.xptr, self.xbs, _tab(self.params), _tab(self.stats),
                          self.bufs["dy"].ptr, self.stride, kind, _tab(self.grads), B, C, T, HW, Cout, int(self.training),
                          self.bn, R.LN_EPS, self.bufs["ws"].ptr, self.need, s)
        self._after("backward")
        return {n: self.bufs[n].get() for n in R.GRAD_NAMES}

    def _layout(self, y):
        B, C, T, HW, Cout, kind = self.case
        return y if kind == 0 else y.view(B, HW, Cout).permute(0, 2, 1).contiguous()


def _check(tag, got, ref, kind):
    for n, v in got.items():
        R.within(v, ref[n], f"{tag} {n}", RECORD, R.group_of(n, kind))


def _full(tag, case, training=True, backward=True, accumulate=False, strided=False, xpad=0, routes=None):
    """Forward (+ backward) of one configuration checked against float64 -> (Run, outputs, problem)."""
    B, C, T, HW, Cout, kind = case
    prob = R.problem(B, C, T, HW, Cout, kind, training, backward, accumulate, _generic())
    x, prm, dy, g0, ref = prob
    run = Run(case, x, prm, dy, training, backward, g0, strided, xpad, routes=routes)
    got = run.forward()
    if backward:
        got.update(run.backward_())
    _check(tag, got, ref, kind)
    return run, got, prob


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nGPU worst err/bound per group:", {k: round(v, 4) for k, v in sorted(RECORD.items())})


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.dispatch_cases()))
def test_dispatch(name, request, tmp_path):
    from cultionet_amd import _lib

    case = R.dispatch_cases()[name]
    served = not name.startswith(R.NO_BACKWARD)
    assert (_lib.query("cn_pretime_workspace_floats", *case[:5], 1) > 0) == served
    # (the generic-kernel child forces its kernel through CN_PRETIME_REG: forcing is its purpose, no route is asserted)
    routes = None if _generic() else Routes(case_id(request), tmp_path)
    _full(f"dispatch {name}", case, backward=served, routes=routes)
    if routes is not None:
        routes.verify()


def test_small_cube_one_entry_tile(request, tmp_path):
    """C (T - 2) = 24 <= 32 outside the register variant's cube: the generic kernels with ONE entry tile in the gradient
    pass (cn_pretime_kernel<4, 4, 1, 1>), which no cube of the dispatch cases selects without CN_PRETIME_REG=0."""
    routes = Routes(case_id(request), tmp_path)
    _full("small cube c4t8", (2, 4, 8, 173, 8, 0), routes=routes)
    routes.verify()


def test_ne3_gradient_pass_has_no_servable_shape():
    """pt_ne = 3 needs 65 <= C (T - 2) <= 96; the LDS image of PASS 4 is beyond 160 KiB at every such cube, so the
    with-backward query refuses them all (the NE = 3 instantiation is compiled but never launched) while the forward
    query accepts them."""
    from cultionet_amd import _lib

    seen = 0
    for C in range(1, 9):
        for T in range(5, 100):
            if 65 <= C * (T - 2) <= 96:
                seen += 1
                assert _lib.query("cn_pretime_workspace_floats", 2, C, T, 173, 8, 1) == -1, (C, T)
                assert _lib.query("cn_pretime_workspace_floats", 2, C, T, 173, 8, 0) > 0, (C, T)
    assert seen > 20


def test_generic_kernel_child():
    """CN_PRETIME_REG is read once per process: a child sends the (3, 12) cubes through the generic kernel."""
    if _generic():
        pytest.skip("already the generic-kernel child")
    env = dict(os.environ, CN_PRETIME_REG="0")
    r = subprocess.run([sys.executable, "-m", "pytest", __file__, "-q", "-x", "-s", "-m", "gpu", "-k",
                        "test_dispatch and c3t12"], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "3 passed" in r.stdout


@pytest.mark.parametrize("name", list(R.WIDE_CASES))
def test_wide_outputs(name, request, tmp_path):
    from cultionet_amd import _lib

    case = R.WIDE_CASES[name]
    B, C, T, HW, Cout, kind = case
    assert _lib.query("cn_pretime_workspace_floats", B, C, T, HW, Cout, 1) == -1
    routes = Routes(case_id(request), tmp_path)
    _full(f"wide train {name}", case, backward=False, routes=routes)
    _full(f"wide inference {name}", case, training=False, backward=False, routes=routes)
    routes.verify()


@pytest.mark.parametrize("name", list(R.EVAL_CASES))
def test_eval_backward(name, request, tmp_path):
    routes = Routes(case_id(request), tmp_path)
    run, got, (x, prm, dy, g0, ref) = _full(f"eval {name}", R.EVAL_CASES[name], training=False, routes=routes)
    routes.verify()
    for k, p in zip(R.BR, prm["br"]):
        for n in ("rm3", "rv3", "rm2", "rv2"):
            assert torch.equal(run.bufs[f"p_{n}_{k}"].get(), p[n]), f"{n}_{k} changed with training = 0"


@pytest.mark.parametrize("name", list(R.ACCUM_CASES))
def test_gradients_accumulate(name):
    case = R.ACCUM_CASES[name]
    run, got, (x, prm, dy, g0, ref) = _full(f"accumulate {name}", case, accumulate=True)
    again = run.backward_()
    for n in R.GRAD_NAMES:
        v, e = ref[n]
        v2 = 2 * v - g0[n].double().reshape(v.shape)
        R.within(again[n], (v2, 2 * e + R.U * v2.abs()), f"accumulate twice {name} {n}", RECORD, R.group_of(n))


@pytest.mark.parametrize("name", list(R.ACCUM_CASES))
def test_strides_bitwise(name):
    """xbs = C T HW + 7, y / dy as channel slices of a wider NCHW buffer (fp32) or with pixel stride Cout + 8 (bf16):
    the same kernel in the same tile order, so every output equals the dense call's bit for bit."""
    case = R.ACCUM_CASES[name]
    _, dense, _ = _full(f"dense {name}", case)
    _, wide, _ = _full(f"strided {name}", case, strided=True, xpad=7)
    for n in dense:
        assert torch.equal(dense[n], wide[n]), f"{n} differs between the dense and the strided call"


@pytest.mark.parametrize("P", list(R.EDGE_PIXELS))
@pytest.mark.parametrize("cube", list(R.EDGE_CUBES))
def test_pixel_edges(cube, P):
    (C, T), (B, HW) = R.EDGE_CUBES[cube], R.EDGE_PIXELS[P]
    _full(f"edge {cube} P={P}", (B, C, T, HW, 8, 0))


@pytest.mark.parametrize("name", list(R.TILE_CASES))
def test_more_tiles_than_blocks(name, request, tmp_path):
    B, C, T, HW, Cout, kind, train = R.TILE_CASES[name]
    assert (B * HW) % 128 != 0
    routes = Routes(case_id(request), tmp_path)
    _full(f"tiles {name}", (B, C, T, HW, Cout, kind), training=train, backward=train, routes=routes)
    routes.verify()


@pytest.mark.parametrize("which", ["register", "generic"])
def test_offsets_32bit(which):
    """Three cubes far apart in one uninitialised buffer. register: 2 xbs 4 > 2^31 and 3 xbs 4 < 2^32 -- the 32-bit lane
    offsets vo / vo1 of the register variant pass 2^31, bitwise equal to the dense call; generic: 3 xbs 4 >= 2^32 -- the
    host hands the shape to the generic kernel (64-bit addresses)."""
    case = R.OFFSET_CASE
    B, C, T, HW, Cout, kind = case
    xbs = 340_000_003 if which == "register" else 357_913_945
    assert 2 * xbs * 4 > 2 ** 31 and (3 * xbs * 4 < 2 ** 32) == (which == "register")
    x, prm, dy, g0, ref = R.problem(B, C, T, HW, Cout, kind, True, False, False, which == "generic" or _generic())
    big = torch.empty(2 * xbs + C * T * HW, dtype=torch.float32, device=_dev())
    try:
        for b in range(B):
            big[b * xbs:b * xbs + C * T * HW].copy_(x[b].reshape(-1))
        run = Run(case, x, prm, dy, True, False, xbuf=(big.data_ptr(), xbs))
        got = run.forward()
        _check(f"offsets {which}", got, ref, kind)
        if which == "register" and not _generic():
            dense = Run(case, x, prm, dy, True, False).forward()
            for n in dense:
                assert torch.equal(dense[n], got[n]), f"{n} differs between the dense and the far-apart call"
    finally:
        del big
        torch.cuda.empty_cache()
