"""The deferred weight-gradient slice sums against float64, from the kernel to the flush of a whole step.

Training wraps every backward pass in deferring_slice_sums, so every convolution weight gradient the optimizer reads
went through cn_ss_push -> cn_slice_sums_kernel -> flush_slice_sums. tests/slicesum_ref.py restates the records and the
sum; this file holds the device side to it.

Layer A: cn_slice_sums_run on tables the test writes. Slices sit in a buffer whose gaps (between slices, the padded rows
  and columns of kind 1, between records) hold NaN, destinations in a sentinel-filled buffer with slack after each dW.
  Exact: slices and the dW prefill are integers in -8..8, every sum of absolute terms is below 8 * 300 + 8 << 2^24
  (asserted), so the fp32 result must EQUAL float64 -- compared over the whole destination buffer, sentinels included,
  so one NaN or one moved sentinel fails. Bounded: randn slices, |err| <= depth * 2^-24 * (sum|part| + |dw0|) per
  element with the depth counted in slicesum_ref.depth, no floor; and the result equals the fp32 restatement of the
  kernel's association bit for bit (the header promises the order of the immediate kernels).
Layer B: the weight-gradient entry points with a sink registered (integer convolutions of tests/conv_exact_worker.py).
Layer C: the rules of the sink (duplicate dW, range edges, capacity, end / begin).
Layer D: cultionet_amd/scratch.py on whole training steps under every flush / table / arena setting.
"""
import ctypes
import typing as T

import numpy as np
import pytest
import torch

import slicesum_ref as R
from conv_exact_worker import (BF, F32, GARB, SENT, SLACK, Canvas, assert_exact, bwgrad_ws_floats, ints, lib, out_size,
                               part, premise, ref_conv, ref_convT, stream, term_bound, wgrad_ws_f32)
from route_ledger import Routes, case_id

pytestmark = pytest.mark.gpu

U32 = R.U32


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


_TABLES: T.Dict[int, T.Tuple[torch.Tensor, torch.Tensor]] = {}


def _tables(capacity=64):
    """(pinned host table, device table) of `capacity` records, shared by the tests (every test synchronizes before it
    returns, so no upload is in flight when the next one rewrites the host side)."""
    if capacity not in _TABLES:
        _TABLES[capacity] = (torch.zeros(capacity * 64, dtype=torch.uint8).pin_memory(),
                             torch.zeros(capacity * 64, dtype=torch.uint8, device=_dev()))
    host, devt = _TABLES[capacity]
    host.zero_()
    return host, devt


def _run(host, devt, first, n, upload=1):
    lib().call("cn_slice_sums_run", host.data_ptr(), devt.data_ptr(), first, n, upload, stream())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# layer A: the kernel on hand-built tables
# ---------------------------------------------------------------------------------------------------------------------

class Spec(T.NamedTuple):
    kind: int
    nslices: int
    n: int = 0        # kind 0
    T: int = 0        # kind 1
    CP: int = 0
    CQ: int = 0

    @property
    def outputs(self):
        return self.n if self.kind == 0 else self.T * self.CP * self.CQ

    @property
    def dims(self):
        if self.kind == 0:
            return dict(kind=0, n=self.n)
        p64 = lambda c: (c + 63) // 64 * 64
        return dict(kind=1, T=self.T, CP=self.CP, CQ=self.CQ, CPp=p64(self.CP), CQp=p64(self.CQ))


def flat(nslices, n):
    return Spec(0, nslices, n=n)


def relayout(nslices, t, cp, cq):
    return Spec(1, nslices, T=t, CP=cp, CQ=cq)


class Tables:
    """Slices and destinations of a list of records: float64 host images, fp32 device copies, the records.

    Slice buffer: record after record with 17 NaN between them; inside a record the slices are `stride` apart, which is
    the slice's extent (n, or T * CPp * CQp) plus 3 (kind 0) / 64 (kind 1) NaN. Only the elements a record may read
    hold values. Destination buffer: SENT everywhere, each dW followed by SLACK + 3 sentinels."""

    def __init__(self, specs, seed, mode, dev):
        self.specs, self.mode, self.dev = list(specs), mode, dev
        self.lay = []
        poff, doff = 7, 5
        for sp in self.specs:
            d = sp.dims
            extent = sp.n if sp.kind == 0 else d["T"] * d["CPp"] * d["CQp"]
            stride = extent + (3 if sp.kind == 0 else 64)
            self.lay.append(dict(part_off=poff, dw_off=doff, stride=stride, nslices=sp.nslices, **d))
            poff += sp.nslices * stride + 17
            doff += sp.outputs + SLACK + 3
        self.part_len, self.dw_len = poff, doff
        self.dw0 = np.full(doff, SENT, dtype=np.float64)
        rng = np.random.default_rng(seed)
        for sp, l in zip(self.specs, self.lay):
            self.dw0[l["dw_off"]:l["dw_off"] + sp.outputs] = self._draw(rng, sp.outputs)
            if mode == "ints":
                assert sp.nslices <= 300
                premise(f"slice sum {sp}", 8.0 * sp.nslices, 8.0)
        self.dw = torch.empty(doff, dtype=F32, device=dev)
        self.part = torch.empty(poff, dtype=F32, device=dev)
        self.reset_dw()
        self.new_values(seed + 1)

    def _draw(self, rng, size):
        if self.mode == "ints":
            return rng.integers(-8, 9, size=size).astype(np.float64)
        return rng.standard_normal(size).astype(np.float32).astype(np.float64)

    def new_values(self, seed):
        """Fresh slice values (the records do not change)."""
        rng = np.random.default_rng(seed)
        self.part64 = np.full(self.part_len, np.nan, dtype=np.float64)
        for sp, l in zip(self.specs, self.lay):
            src, _ = R.indices(**self._dims(l))
            for s in range(sp.nslices):
                self.part64[l["part_off"] + s * l["stride"] + src] = self._draw(rng, src.size)
        self.part.copy_(torch.from_numpy(self.part64).float())

    def reset_dw(self):
        self.dw.copy_(torch.from_numpy(self.dw0).float())

    @staticmethod
    def _dims(l):
        return {k: v for k, v in l.items() if k in ("kind", "n", "T", "CP", "CQ", "CPp", "CQp")}

    def records(self, which=None):
        which = range(len(self.specs)) if which is None else which
        return [R.record(part=self.part.data_ptr() + 4 * self.lay[i]["part_off"],
                         dw=self.dw.data_ptr() + 4 * self.lay[i]["dw_off"], stride=self.lay[i]["stride"],
                         nslices=self.lay[i]["nslices"], **self._dims(self.lay[i])) for i in which]

    def check(self, which, what):
        """The destination buffer after ONE run of records `which` over the prefill."""
        got = self.dw.cpu()
        want = self.dw0.copy()
        for i in which:
            l = self.lay[i]
            R.apply(self.part64, l["part_off"], want, l["dw_off"], l["stride"], l["nslices"], **self._dims(l))
        if self.mode == "ints":
            g = got.double()
            w = torch.from_numpy(want)
            if not torch.equal(g, w):
                bad = (g != w).nonzero().flatten()
                at = int(bad[0])
                owner = [i for i in which if self.lay[i]["dw_off"] <= at < self.lay[i]["dw_off"] + self.specs[i].outputs]
                raise AssertionError(f"{what}: {bad.numel()} of {w.numel()} destination floats differ; first at {at} "
                                     f"(record {owner or 'none: a sentinel'}): got {float(g[at])}, want {float(w[at])}")
            return 0.0
        # bounded: depth * u * (sum|part| + |dw0|) on the outputs, nothing (so: equality) everywhere else
        scale = np.abs(self.dw0)
        bound = np.zeros_like(scale)
        order = self.dw0.astype(np.float32)
        part32 = self.part64.astype(np.float32)
        for i in which:
            l = self.lay[i]
            R.apply(self.part64, l["part_off"], scale, l["dw_off"], l["stride"], l["nslices"], absolute=True,
                    **self._dims(l))
            R.apply_f32(part32, l["part_off"], order, l["dw_off"], l["stride"], l["nslices"], **self._dims(l))
            _, dst = R.indices(**self._dims(l))
            bound[l["dw_off"] + dst] = R.depth(l["kind"], l["nslices"]) * U32 * scale[l["dw_off"] + dst]
        err = np.abs(got.double().numpy() - want)
        ok = err <= bound  # (NaN compares false)
        live = bound > 0
        ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
        print(f"BOUND {what}: worst err/bound {ratio:.3f}")
        assert bool(ok.all()), f"{what}: {int((~ok).sum())} floats out of bound (or a sentinel moved), err/bound {ratio:.3f}"
        same = got.numpy() == order
        assert bool(same.all()), f"{what}: {int((~same).sum())} outputs differ from the kernel's summation order in fp32"
        return ratio


def _single(spec, seed, mode):
    """One record, one launch."""
    dev = _dev()
    host, devt = _tables()
    tab = Tables([spec], seed, mode, dev)
    recs = tab.records()
    R.write_records(host, recs)
    _run(host, devt, 0, 1)
    assert int(R.read_records(host, 0, 1)[0]["chunk0"]) == 0
    return tab.check([0], f"{spec} {mode}")


@pytest.mark.parametrize("mode", ["ints", "randn"])
@pytest.mark.parametrize("nslices", [1, 2, 3, 16, 127, 128])
def test_kernel_flat_record(nslices, mode):
    """kind 0, at most 128 slices: thread = output, two accumulators; 256 outputs per block."""
    assert R.body(0, nslices) == "flat"
    worst = max(_single(flat(nslices, n), 10 * nslices + j, mode) for j, n in enumerate((1, 255, 256, 257, 1000)))
    assert worst <= 1.0


@pytest.mark.parametrize("mode", ["ints", "randn"])
@pytest.mark.parametrize("nslices", [129, 130, 131, 132, 141, 144, 145, 300])
def test_kernel_waves_record(nslices, mode):
    """kind 0, more than 128 slices: four waves, 16-step and 4-step loops, LDS combine; 64 outputs per block. The
    counts cover every remainder of the 4-step loop (129..132), 16-step turns that end at and around a whole turn
    (141, 144, 145) and waves whose tail is empty."""
    assert R.body(0, nslices) == "waves"
    worst = max(_single(flat(nslices, n), 10 * nslices + j, mode) for j, n in enumerate((1, 63, 64, 65, 200)))
    assert worst <= 1.0


K1_SHAPES = [(1, 1, 1), (1, 40, 24), (9, 8, 8), (9, 33, 65), (9, 3, 136)]


@pytest.mark.parametrize("mode", ["ints", "randn"])
@pytest.mark.parametrize("shape", K1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_relayout_record(shape, mode):
    """kind 1: padded [T][CPp][CQp] slices into the [CP][CQ][T] weight. Both maps cross padded rows (CQ < CQp) and
    padded planes (CP < CPp), whose contents are NaN here."""
    worst = max(_single(relayout(ns, *shape), 1000 * j + sum(shape), mode) for j, ns in enumerate((1, 2, 5, 16, 17, 29)))
    assert worst <= 1.0


MIXED = [
    flat(3, 1),                   # 0: one block, first
    flat(129, 200),               # 1: waves
    relayout(5, 9, 33, 65),       # 2: 302 blocks
    flat(128, 1000),              # 3: flat, 4 blocks
    flat(2, 255),                 # 4: one block between two large records
    flat(300, 65),                # 5: waves, 2 blocks
    relayout(17, 1, 40, 24),      # 6
    flat(16, 257),                # 7: flat, 2 blocks
    relayout(29, 9, 3, 136),      # 8
    flat(141, 63),                # 9: waves, one block
    flat(127, 256),               # 10: flat, exactly one block
    relayout(1, 1, 1, 1),         # 11: one block, last
]


@pytest.mark.parametrize("mode", ["ints", "randn"])
def test_kernel_mixed_table(mode):
    """Twelve records of all three bodies in one launch (the binary search over chunk0 deals the blocks); again with
    upload = 0 after the SLICES changed (the device table is reused, the sums follow the new values); again as two
    launches over [0, 5) and [5, 12) into fresh destinations (first > 0; chunk0 restarts at 0 in each range)."""
    dev = _dev()
    host, devt = _tables()
    tab = Tables(MIXED, 77, mode, dev)
    assert {R.body(s.kind, s.nslices) for s in MIXED} == {"flat", "waves", "relayout"}
    every = list(range(12))
    recs = tab.records()
    assert R.chunks(recs[0]) == 1 and R.chunks(recs[4]) == 1 and R.chunks(recs[11]) == 1
    assert min(R.chunks(recs[3]), R.chunks(recs[5])) > 1
    R.write_records(host, recs)
    _run(host, devt, 0, 12)
    assert [int(c) for c in R.read_records(host, 0, 12)["chunk0"]] == R.deal(recs)[:-1]
    tab.check(every, f"mixed table {mode}")
    # the same records, other slice values, no upload
    before = tab.part64.copy()
    tab.new_values(178)
    live = ~np.isnan(before)
    assert np.array_equal(live, ~np.isnan(tab.part64)) and float((before[live] != tab.part64[live]).mean()) > 0.5
    tab.reset_dw()
    _run(host, devt, 0, 12, upload=0)
    tab.check(every, f"mixed table {mode}, upload 0")
    # two ranges: the device table is overwritten range by range
    tab.reset_dw()
    host.zero_()
    R.write_records(host, recs)
    _run(host, devt, 0, 5)
    assert [int(c) for c in R.read_records(host, 0, 5)["chunk0"]] == R.deal(recs[:5])[:-1]
    tab.check(every[:5], f"mixed table {mode}, range [0, 5)")
    _run(host, devt, 5, 7)
    assert [int(c) for c in R.read_records(host, 5, 7)["chunk0"]] == R.deal(recs[5:])[:-1]
    tab.check(every, f"mixed table {mode}, ranges [0, 5) + [5, 12)")
    # ... and [0, 5) once more without an upload: its part of the device table survived the launch over [5, 12)
    tab.reset_dw()
    _run(host, devt, 0, 5, upload=0)
    tab.check(every[:5], f"mixed table {mode}, range [0, 5) again, upload 0")


# ---------------------------------------------------------------------------------------------------------------------
# layers B and C: the entry points with a sink registered
# ---------------------------------------------------------------------------------------------------------------------

class Grad:
    """The flat "gradient" buffer of a test: sentinel-filled, dW canvases carved out of it one after the other (each
    with its SLACK, 3 more floats apart so that they start unaligned as parameters do)."""

    def __init__(self, floats, dev):
        self.buf = torch.full((floats,), SENT, dtype=F32, device=dev)
        self.off = 3
        self.canvases = []

    def place(self, shape, prefill):
        cv = Canvas(shape, F32, self.buf.device, data=prefill)
        n = cv.buf.numel()
        assert self.off + n <= self.buf.numel(), "gradient buffer too small"
        home = self.buf[self.off:self.off + n]
        home.copy_(cv.buf)
        cv.buf, cv.t = home, cv.view(home)
        cv.off, cv.prefill = self.off, prefill.double()
        self.off += n + 3
        self.canvases.append(cv)
        return cv

    def assert_untouched_outside(self, what):
        c = self.buf.clone()
        for cv in self.canvases:
            cv.view(c[cv.off:cv.off + cv.buf.numel()]).fill_(SENT)
        assert bool((c == SENT).all()), f"{what}: written outside the weight gradients"


class Sink:
    """cn_slice_sums_begin ... cn_slice_sums_end around a block (always ended: the sink is thread state)."""

    def __init__(self, lo_ptr, floats, capacity=64):
        self.lo, self.floats, self.cap = lo_ptr, floats, capacity
        self.host, self.devt = _tables(capacity)

    def __enter__(self):
        lib().call("cn_slice_sums_begin", self.host.data_ptr(), self.cap, self.lo, self.floats)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        lib().call("cn_slice_sums_end")
        return False

    @property
    def count(self):
        return lib().query("cn_slice_sums_count")

    def records(self):
        return R.read_records(self.host, 0, max(self.count, 0))

    def run(self, first=0, n=None):
        n = self.count - first if n is None else n
        _run(self.host, self.devt, first, n)


def _sink_over(grad, capacity=64):
    return Sink(grad.buf.data_ptr(), grad.buf.numel(), capacity)


class Wgrad:
    """One weight-gradient call: inputs (integers: exact premise asserted; or randn), float64 reference, launch."""

    def __init__(self, kind, case, seed, mode="ints", ws="full", G=1):
        # kind: "f32" | "f32g" (grouped, G sets) | "bf16" | "bf16t" (ConvTranspose2d)
        # case: B, Cin, H, W, Cout, k, stride, dil (pad = dil * (k // 2); transposed: pad 1)
        self.kind, self.case, self.mode, self.G, self.wsmode = kind, case, mode, G, ws
        B, Cin, H, W, Cout, k, s, d = case
        self.p = p = 1 if kind == "bf16t" else d * (k // 2)
        dev = _dev()
        if kind == "bf16t":
            Ho, Wo = (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
            self.wshape = (Cin, Cout, k, k)
        else:
            Ho, Wo = out_size(H, W, k, s, p, d)
            self.wshape = (Cout, Cin, k, k)
        self.Ho, self.Wo = Ho, Wo
        bf = kind in ("bf16", "bf16t")
        self.x, self.dy, self.w0, self.dw64 = [], [], [], []
        for g in range(G):
            if mode == "ints":
                x, dy = ints((B, Cin, H, W), -4, 4, seed + 10 * g), ints((B, Cout, Ho, Wo), -3, 3, seed + 10 * g + 1)
                w0 = ints(self.wshape, -8, 8, seed + 10 * g + 2)
                premise(f"dw {kind} {case}", term_bound(x, dy, B * (H * W if kind == "bf16t" else Ho * Wo)), 8)
            else:
                gen = torch.Generator().manual_seed(seed + 10 * g)
                rnd = lambda shape: torch.randn(shape, generator=gen).to(BF if bf else F32).double()
                x, dy = rnd((B, Cin, H, W)), rnd((B, Cout, Ho, Wo))
                w0 = torch.randn(self.wshape, generator=gen).double()
            zw = torch.zeros(self.wshape, dtype=torch.float64)
            # (a copy of x: the references mark their float64 inputs as requiring gradients, in place)
            dw64 = (ref_convT(x.clone(), zw, None, dy, s, p) if kind == "bf16t" else
                    ref_conv(x.clone(), zw, None, dy, s, p, d))[2]
            self.x.append(x); self.dy.append(dy); self.w0.append(w0); self.dw64.append(dw64)
        if bf:
            c8 = lambda c: (c + 7) // 8 * 8
            self.xc = [Canvas(x.shape, BF, dev, pitch=c8(Cin) + 8, fill=GARB, data=x) for x in self.x]
            self.dyc = [Canvas(y.shape, BF, dev, pitch=c8(Cout) + 16, fill=GARB, data=y) for y in self.dy]
        else:
            self.xc = [Canvas(x.shape, F32, dev, fill=GARB, data=x) for x in self.x]
            self.dyc = [Canvas(y.shape, F32, dev, fill=GARB, data=y) for y in self.dy]
        self.keep = []

    def want(self, g=0):
        return self.dw64[g] + self.w0[g]

    def launch(self, dws):
        """Into the canvases `dws` (one per group), with a workspace of its own that lives as long as this object."""
        B, Cin, H, W, Cout, k, s, d = self.case
        L, st, p = lib(), stream(), self.p
        if self.kind in ("f32", "f32g"):
            wsp, wsn, keep = wgrad_ws_f32(B, Cin, H, W, Cout, self.Ho, self.Wo, "full")
            self.ws, self.wsn = keep, wsn
        else:
            wsn = bwgrad_ws_floats(B, Cin, H, W, Cout, k, s, p, d, int(self.kind == "bf16t"), self.wsmode)
            keep = torch.empty(wsn + 4, device=_dev())
            wsp, self.ws, self.wsn = keep.data_ptr(), keep, wsn
        self.keep.append(keep)
        tab = lambda ptrs: (ctypes.c_void_p * len(ptrs))(*ptrs)
        if self.kind == "f32":
            L.call("cn_conv2d_bwd_weight_f32", self.xc[0].ptr, self.xc[0].pitch, self.dyc[0].ptr, self.dyc[0].pitch,
                   dws[0].ptr, B, Cin, H, W, Cout, k, k, s, p, d, wsp, wsn, st)
        elif self.kind == "f32g":
            L.call("cn_conv2d_bwd_weight_grouped_f32", self.G, tab([c.ptr for c in self.xc]), self.xc[0].pitch,
                   tab([c.ptr for c in self.dyc]), self.dyc[0].pitch, tab([c.ptr for c in dws]), B, Cin, H, W, Cout, k,
                   k, s, p, d, wsp, wsn, st)
        elif self.kind == "bf16":
            L.call("cn_conv2d_bwd_weight_bf16", self.xc[0].ptr, self.xc[0].pitch, self.dyc[0].ptr, self.dyc[0].pitch,
                   dws[0].ptr, B, Cin, H, W, Cout, k, k, s, p, d, wsp, wsn, st)
        else:
            L.call("cn_conv_transpose2d_bwd_weight_bf16", self.xc[0].ptr, self.xc[0].pitch, self.dyc[0].ptr,
                   self.dyc[0].pitch, dws[0].ptr, B, Cin, H, W, Cout, k, k, s, p, wsp, wsn, st)

    def place(self, grad):
        return [grad.place(self.wshape, w0) for w0 in self.w0]

    def floats(self):
        return self.G * (int(np.prod(self.wshape)) + SLACK + 3)

    def check_record(self, rec, dwc, cls):
        """One record of this call. cls: "flat" (16..128 slices), "waves" (> 128), "relayout" (kind 1, any count) or a
        slice count."""
        B, Cin, H, W, Cout, k, s, d = self.case
        n = int(np.prod(self.wshape))
        assert int(rec["dw"]) == dwc.ptr and int(rec["n"]) == n, (rec, n)
        ns = int(rec["nslices"])
        if self.kind in ("f32", "f32g"):
            assert int(rec["kind"]) == 0 and int(rec["slice_stride"]) == n
            assert ns >= 16, f"{ns} slices: the fp32 path defers from 16 on"
        else:
            cp, cq = self.wshape[0], self.wshape[1]
            p64 = lambda c: (c + 63) // 64 * 64
            got = tuple(int(rec[f]) for f in ("kind", "T", "CP", "CQ", "CPp", "CQp"))
            assert got == (1, k * k, cp, cq, p64(cp), p64(cq)), got
            assert int(rec["slice_stride"]) == k * k * p64(cp) * p64(cq) and ns >= 1
        if isinstance(cls, int):
            assert ns == cls, f"{self.kind} {self.case}: {ns} slices, the case was chosen for {cls}"
        else:
            assert R.body(int(rec["kind"]), ns) == cls, f"{self.kind} {self.case}: {ns} slices is not the {cls} body"
        lo, hi = self.ws.data_ptr(), self.ws.data_ptr() + 4 * self.ws.numel()
        assert lo <= int(rec["part"]) and int(rec["part"]) + 4 * ns * int(rec["slice_stride"]) <= hi, "slices outside ws"
        return ns


def _deferred_exact(calls, classes, what, routes=None):
    """Every call into one sink: the dWs keep their prefill until the run, then equal float64; records as expected.
    routes (tests/route_ledger.py): learns the kernel of every call, launched under the active sink."""
    dev = _dev()
    grad = Grad(sum(c.floats() for c in calls) + 16, dev)
    dws = [c.place(grad) for c in calls]
    with _sink_over(grad) as sink:
        for i, (c, d) in enumerate(zip(calls, dws)):
            with part(routes, f"dw {i} {c.kind}", "sink active", f"ws {c.wsmode}"):
                c.launch(d)
        torch.cuda.synchronize()
        assert sink.count == sum(c.G for c in calls), (what, sink.count)
        recs = sink.records()
        i = 0
        for c, d, cls in zip(calls, dws, classes):
            for g in range(c.G):
                ns = c.check_record(recs[i], d[g], cls)
                if g:  # the groups' slices follow each other in the workspace
                    assert int(recs[i]["part"]) == int(recs[i - 1]["part"]) + 4 * ns * int(recs[i]["slice_stride"])
                assert_exact(d[g].t, d[g].prefill, f"{what}: dW before the run (record {i})")
                i += 1
        print(f"RECORDS {what}: nslices {[int(r['nslices']) for r in recs]}")
        sink.run()
        assert sink.count == len(recs)
    for c, d in zip(calls, dws):
        for g in range(c.G):
            assert_exact(d[g].t, c.want(g), f"{what}: dW after the run")
    grad.assert_untouched_outside(what)
    return recs


F32_FLAT = (4, 8, 28, 28, 8, 3, 1, 1)   # 28 row chunks of 4 rows x 28 columns: 28 slices
F32_WAVES = (8, 8, 50, 50, 8, 3, 1, 1)  # 8 x 25 chunks of 2 rows: 200 slices
F32_CASES = [
    (F32_FLAT, "flat"),
    (F32_WAVES, "waves"),
    ((4, 8, 28, 28, 8, 1, 1, 1), "flat"),   # 1x1
    ((4, 8, 56, 56, 8, 3, 2, 1), "flat"),   # stride 2: the 28 x 28 gradient plane is chunked, 28 slices again
    ((4, 8, 100, 100, 40, 3, 2, 1), "flat"),  # single-buffered staging (more than 32 couts, 100-wide stride-2 halo)
]


@pytest.mark.parametrize("case,cls", F32_CASES)
def test_f32_weight_gradient_deferred_exact(case, cls, request, tmp_path):
    routes = Routes(case_id(request), tmp_path)
    recs = _deferred_exact([Wgrad("f32", case, 300)], [cls], f"f32 {case}", routes)
    routes.verify()
    if case in (F32_FLAT, F32_WAVES):
        assert int(recs[0]["nslices"]) == (28 if case == F32_FLAT else 200)


def test_f32_few_slices_are_not_deferred():
    """(2, 8, 12, 12, 8): 2 images x 2 chunks = 4 splits, below 16: float atomics straight into dW, nothing pushed."""
    dev = _dev()
    c = Wgrad("f32", (2, 8, 12, 12, 8, 3, 1, 1), 310)
    grad = Grad(c.floats() + 16, dev)
    dws = c.place(grad)
    with _sink_over(grad) as sink:
        c.launch(dws)
        torch.cuda.synchronize()
        assert sink.count == 0
        assert_exact(dws[0].t, c.want(), "dW complete at once")
    grad.assert_untouched_outside("few slices")


@pytest.mark.parametrize("kind,case,G", [
    ("f32", (2, 8, 12, 12, 8, 3, 1, 1), 1),
    ("f32g", (2, 8, 12, 12, 8, 3, 1, 1), 2),     # two sets per launch
    ("f32", (2, 8, 12, 12, 8, 1, 1, 1), 1),      # 1x1
    ("f32", (4, 8, 25, 25, 40, 3, 2, 1), 1),     # single-buffered stride-2 staging from an odd plane, 8 splits
])
def test_f32_below_16_slices_under_a_sink_exact(kind, case, G, request, tmp_path):
    """Fewer than 16 splits with a sink active, as most fp32 weight gradients of a training step run: float atomics
    straight into every dW, nothing pushed, equal to float64 (integer inputs)."""
    dev = _dev()
    c = Wgrad(kind, case, 315, G=G)
    grad = Grad(c.floats() + 16, dev)
    dws = c.place(grad)
    routes = Routes(case_id(request), tmp_path)
    with _sink_over(grad) as sink:
        with routes.part("dw", "sink active", "ws full"):
            c.launch(dws)
        torch.cuda.synchronize()
        assert sink.count == 0
        for g in range(G):
            assert_exact(dws[g].t, c.want(g), f"dW {g} complete at once")
    grad.assert_untouched_outside("few slices")
    routes.verify()


@pytest.mark.parametrize("G", [2, 4])
def test_f32_grouped_weight_gradient_deferred_exact(G, request, tmp_path):
    """G records from one push, their slices G * 28 in a row."""
    routes = Routes(case_id(request), tmp_path)
    _deferred_exact([Wgrad("f32g", F32_FLAT, 320, G=G)], [28], f"f32 grouped G={G}", routes)
    routes.verify()


BF16_CASES = [
    ((2, 8, 12, 12, 8, 3, 1, 1), "full"),
    ((2, 16, 13, 13, 31, 3, 1, 1), "full"),
    ((1, 24, 5, 6, 33, 3, 1, 1), "full"),
    ((2, 136, 9, 11, 256, 1, 1, 1), "full"),
    ((2, 24, 14, 14, 129, 3, 1, 2), "full"),
    ((2, 64, 25, 25, 64, 3, 1, 1), "one"),
    ((2, 64, 25, 25, 64, 3, 1, 1), "mid"),
    ((4, 8, 28, 28, 8, 3, 1, 1), "full"),   # at least 7 tiles per image whatever the tile: 28 or more splits, so the
                                            # 16-step loop of the sum really runs
    ((2, 16, 13, 13, 24, 1, 1, 1), "full"),  # routes of the training step (route ledger): 1x1 on an odd plane,
    ((2, 16, 20, 50, 24, 3, 2, 1), "full"),  # stride 2 on 5 x 25 tiles,
    ((2, 16, 29, 29, 24, 3, 4, 1), "full"),  # stride 4
]


def _bf16_class(case, ws):
    return 1 if ws == "one" else "relayout"


@pytest.mark.parametrize("case,ws", BF16_CASES)
def test_bf16_weight_gradient_deferred_exact(case, ws, request, tmp_path):
    """Every bf16 weight gradient defers, with one split too."""
    routes = Routes(case_id(request), tmp_path)
    recs = _deferred_exact([Wgrad("bf16", case, 400, ws=ws)], [_bf16_class(case, ws)], f"bf16 {case} ws={ws}", routes)
    routes.verify()
    ns = int(recs[0]["nslices"])
    if ws == "mid":
        assert ns > 1, "the in-between workspace was meant to leave more than one split"
    if case[0] == 4:
        assert ns >= 13, "chosen so that the 16-step loop runs"


def test_bf16_transposed_weight_gradient_deferred_exact(request, tmp_path):
    routes = Routes(case_id(request), tmp_path)
    _deferred_exact([Wgrad("bf16t", (2, 16, 13, 13, 16, 3, 2, 1), 410)], ["relayout"], "bf16 ConvTranspose2d", routes)
    routes.verify()


def test_mixed_flush_exact(request, tmp_path):
    """Three fp32 and three bf16 launches into one sink, one run."""
    calls = [Wgrad("f32", F32_FLAT, 500), Wgrad("bf16", (2, 16, 13, 13, 31, 3, 1, 1), 510),
             Wgrad("f32", F32_WAVES, 520), Wgrad("bf16", (2, 24, 14, 14, 129, 3, 1, 2), 530),
             Wgrad("bf16", (2, 136, 9, 11, 256, 1, 1, 1), 540), Wgrad("f32", (4, 8, 28, 28, 8, 1, 1, 1), 550)]
    routes = Routes(case_id(request), tmp_path)
    _deferred_exact(calls, ["flat", "relayout", "waves", "relayout", "relayout", "flat"], "mixed flush", routes)
    routes.verify()


def _immediate_and_deferred(kind, case, ws, seed):
    """The same randn call with no sink and with one: (immediate dW, deferred dW, record, the call)."""
    dev = _dev()
    c = Wgrad(kind, case, seed, mode="randn", ws=ws)
    grad = Grad(2 * c.floats() + 16, dev)
    imm, dfr = c.place(grad), c.place(grad)
    assert lib().query("cn_slice_sums_count") == -1
    c.launch(imm)
    torch.cuda.synchronize()
    with _sink_over(grad) as sink:
        c.launch(dfr)
        torch.cuda.synchronize()
        assert sink.count == 1
        rec = sink.records()[0]
        assert torch.equal(dfr[0].t.cpu().double(), c.w0[0])
        sink.run()
    grad.assert_untouched_outside(f"{kind} {case}")
    return imm[0], dfr[0], rec, c


# (the cases the route ledger added to F32_CASES / BF16_CASES follow the earlier ones, which keep their ids)
@pytest.mark.parametrize("kind,case,ws", [("f32", c, "full") for c, cls in F32_CASES[:4] if cls == "flat"] +
                         [("bf16", c, ws) for c, ws in BF16_CASES[:8]] + [("bf16t", (2, 16, 13, 13, 16, 3, 2, 1), "full")] +
                         [("f32", c, "full") for c, cls in F32_CASES[4:] if cls == "flat"] +
                         [("bf16", c, ws) for c, ws in BF16_CASES[8:]])
def test_deferred_is_bitwise_the_immediate_sum(kind, case, ws):
    """Random inputs: the batched launch sums every output with the association of the immediate kernel, so wherever
    that kernel is deterministic (bf16 always; fp32 up to 128 slices) the two results are the same bits."""
    imm, dfr, rec, _ = _immediate_and_deferred(kind, case, ws, 600)
    assert kind != "f32" or int(rec["nslices"]) <= 128
    a, b = imm.t.cpu(), dfr.t.cpu()
    assert not bool(a.isnan().any())
    assert torch.equal(a.contiguous().view(-1).view(torch.int32), b.contiguous().view(-1).view(torch.int32)), \
        f"{int((a != b).sum())} of {a.numel()} weights differ from the immediate path"


def test_f32_waves_deferred_sum_is_bounded():
    """More than 128 fp32 slices: the immediate kernel adds 16 groups with float atomics, so there is no bitwise twin.
    The deferred dW is held to the slices the contraction left in the workspace: float64 sum of exactly those, bound
    depth * 2^-24 * (sum|slice| + |dw0|) per element, and the fp32 restatement of the kernel's order bit for bit."""
    _, dfr, rec, c = _immediate_and_deferred("f32", F32_WAVES, "full", 610)
    ns, n, stride = int(rec["nslices"]), int(rec["n"]), int(rec["slice_stride"])
    assert R.body(0, ns) == "waves"
    off = (int(rec["part"]) - c.ws.data_ptr()) // 4
    part32 = c.ws[off:off + ns * stride].cpu().numpy()
    dw0 = c.w0[0].float().numpy().reshape(-1)   # what the canvas held
    want, scale, order = dw0.astype(np.float64), np.abs(dw0.astype(np.float64)), dw0.copy()
    R.apply(part32.astype(np.float64), 0, want, 0, stride, ns, kind=0, n=n)
    R.apply(part32.astype(np.float64), 0, scale, 0, stride, ns, kind=0, n=n, absolute=True)
    R.apply_f32(part32, 0, order, 0, stride, ns, kind=0, n=n)
    got = dfr.t.cpu().numpy().reshape(-1)
    err, bound = np.abs(got.astype(np.float64) - want), R.depth(0, ns) * U32 * scale
    print(f"BOUND f32 waves conv, {ns} slices: worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert np.array_equal(got, order)


# ---- layer C: the rules of the sink ----------------------------------------------------------------------------------

def test_sink_duplicate_dw_is_reduced_at_once():
    """A second launch into a dW that has a pending record must not be deferred (two records would add into one dW from
    different blocks of one launch): the count stays, its contribution lands at once, the flush adds the first."""
    dev = _dev()
    a, b = Wgrad("f32", F32_FLAT, 700), Wgrad("f32", F32_FLAT, 710)
    grad = Grad(a.floats() + 16, dev)
    dw = a.place(grad)
    with _sink_over(grad) as sink:
        a.launch(dw)
        assert sink.count == 1
        b.launch(dw)
        assert sink.count == 1
        torch.cuda.synchronize()
        assert_exact(dw[0].t, a.w0[0] + b.dw64[0], "after the second call: prefill + its contribution")
        sink.run()
    assert_exact(dw[0].t, a.w0[0] + a.dw64[0] + b.dw64[0], "after the flush: prefill + both")
    grad.assert_untouched_outside("duplicate dW")


def test_sink_partly_overlapping_dw_is_reduced_at_once():
    """The same rule for a dW that only OVERLAPS a pending record (it starts 100 floats into it): deferred, the two
    records would add into the shared floats from different blocks of one launch, unordered. The second call must
    reduce at once; every float of both ranges ends up exact."""
    dev = _dev()
    a, b = Wgrad("f32", F32_FLAT, 715), Wgrad("f32", F32_FLAT, 716)
    n, shift = int(np.prod(a.wshape)), 100
    grad = Grad(a.floats() + n + 16, dev)
    dw = a.place(grad)

    class Inside:  # b's dW: n floats from `shift` floats behind the start of a's
        ptr = dw[0].ptr + 4 * shift

    want = torch.full((grad.buf.numel(),), SENT, dtype=torch.float64)
    lo = dw[0].off
    want[lo:lo + n] = a.w0[0].reshape(-1)
    want[lo + shift:lo + shift + n] += b.dw64[0].reshape(-1)
    premise("overlap", term_bound(a.x[0], a.dy[0], 4 * 28 * 28) + term_bound(b.x[0], b.dy[0], 4 * 28 * 28), -SENT)
    with _sink_over(grad) as sink:
        a.launch(dw)
        assert sink.count == 1
        b.launch([Inside])
        assert sink.count == 1, "a dW that overlaps a pending record was deferred"
        torch.cuda.synchronize()
        assert torch.equal(grad.buf.cpu().double(), want), "after the second call: its contribution only"
        sink.run()
    want[lo:lo + n] += a.dw64[0].reshape(-1)
    assert torch.equal(grad.buf.cpu().double(), want), "after the flush: both contributions, nothing else moved"


@pytest.mark.parametrize("edge,deferred", [("ends one past", False), ("starts one before", False),
                                           ("ends at the edge", True), ("starts at the edge", True)])
def test_sink_range_edges(edge, deferred):
    """Only a dW that lies inside [dw_lo, dw_lo + dw_floats) whole is deferred."""
    dev = _dev()
    c = Wgrad("f32", F32_FLAT, 720)
    grad = Grad(c.floats() + 16, dev)
    dw = c.place(grad)
    n = int(np.prod(c.wshape))
    base = grad.buf.data_ptr()
    lo, floats = {"ends one past": (base, dw[0].off + n - 1), "starts one before": (dw[0].ptr + 4, n + 8),
                  "ends at the edge": (base, dw[0].off + n), "starts at the edge": (dw[0].ptr, n)}[edge]
    with Sink(lo, floats) as sink:
        c.launch(dw)
        torch.cuda.synchronize()
        assert sink.count == int(deferred)
        if deferred:
            assert_exact(dw[0].t, c.w0[0], "deferred: dW still the prefill")
            sink.run()
    assert_exact(dw[0].t, c.want(), f"dW, {edge}")
    grad.assert_untouched_outside(edge)


def test_sink_capacity():
    """capacity 2: the third call reduces at once. A grouped call of 4 into capacity 5 behind two pending records is
    refused WHOLE: no record of it is taken and all four dW are complete at once."""
    dev = _dev()
    singles = [Wgrad("f32", F32_FLAT, 730 + 7 * i) for i in range(3)]
    grad = Grad(sum(c.floats() for c in singles) + 16, dev)
    dws = [c.place(grad) for c in singles]
    with _sink_over(grad, capacity=2) as sink:
        for i, (c, d) in enumerate(zip(singles, dws)):
            c.launch(d)
            assert sink.count == min(i + 1, 2)
        torch.cuda.synchronize()
        assert_exact(dws[0][0].t, singles[0].w0[0], "first: pending")
        assert_exact(dws[1][0].t, singles[1].w0[0], "second: pending")
        assert_exact(dws[2][0].t, singles[2].want(), "third: reduced at once")
        sink.run()
    for c, d in zip(singles, dws):
        assert_exact(d[0].t, c.want(), "capacity 2, after the run")
    grad.assert_untouched_outside("capacity 2")

    grouped = Wgrad("f32g", F32_FLAT, 760, G=4)
    grad = Grad(singles[0].floats() * 2 + grouped.floats() + 16, dev)
    dws = [c.place(grad) for c in singles[:2]]
    gdw = grouped.place(grad)
    with _sink_over(grad, capacity=5) as sink:
        for c, d in zip(singles[:2], dws):
            c.launch(d)
        assert sink.count == 2
        grouped.launch(gdw)
        assert sink.count == 2
        torch.cuda.synchronize()
        for g in range(4):
            assert_exact(gdw[g].t, grouped.want(g), f"group {g}: complete at once")
        for c, d in zip(singles[:2], dws):
            assert_exact(d[0].t, c.w0[0], "pending")
        sink.run()
    for c, d in zip(singles[:2], dws):
        assert_exact(d[0].t, c.want(), "capacity 5, after the run")
    for g in range(4):
        assert_exact(gdw[g].t, grouped.want(g), f"group {g} after the run: not summed twice")
    grad.assert_untouched_outside("capacity 5")


def test_sink_end_and_begin_again():
    """cn_slice_sums_end: count -1, calls reduce at once. cn_slice_sums_begin: the count restarts at 0, and the same
    sequence of calls leaves the first 60 bytes of every record as they were (an identical record is not rewritten;
    its chunk0 belongs to the run)."""
    dev = _dev()
    calls = [Wgrad("f32", F32_FLAT, 800), Wgrad("bf16", (2, 16, 13, 13, 31, 3, 1, 1), 810)]
    grad = Grad(sum(c.floats() for c in calls) + 16, dev)
    dws = [c.place(grad) for c in calls]

    def reset():
        for c, d in zip(calls, dws):
            d[0].t.copy_(c.w0[0].float())

    def relaunch(c, d):  # with the workspace of the first launch: same addresses, same record
        ws = c.keep[0]
        wgrad = {"f32": "cn_conv2d_bwd_weight_f32", "bf16": "cn_conv2d_bwd_weight_bf16"}[c.kind]
        B, Cin, H, W, Cout, k, s, dil = c.case
        lib().call(wgrad, c.xc[0].ptr, c.xc[0].pitch, c.dyc[0].ptr, c.dyc[0].pitch, d[0].ptr, B, Cin, H, W, Cout, k, k,
                   s, c.p, dil, ws.data_ptr(), c.wsn, stream())

    with _sink_over(grad) as sink:
        host = sink.host
        for c, d in zip(calls, dws):
            c.launch(d)
        assert sink.count == 2
        sink.run()
        first = host.numpy().reshape(-1, 64)[:2].copy()
    assert lib().query("cn_slice_sums_count") == -1
    for c, d in zip(calls, dws):
        assert_exact(d[0].t, c.want(), "first round")
    reset()
    for c, d in zip(calls, dws):   # no sink: immediate
        relaunch(c, d)
    torch.cuda.synchronize()
    assert lib().query("cn_slice_sums_count") == -1
    for c, d in zip(calls, dws):
        assert_exact(d[0].t, c.want(), "after end: reduced at once")
    reset()
    lib().call("cn_slice_sums_begin", host.data_ptr(), 64, grad.buf.data_ptr(), grad.buf.numel())
    try:
        assert lib().query("cn_slice_sums_count") == 0
        for c, d in zip(calls, dws):
            relaunch(c, d)
        assert lib().query("cn_slice_sums_count") == 2
        again = host.numpy().reshape(-1, 64)[:2].copy()
        assert np.array_equal(first[:, :R.HEAD], again[:, :R.HEAD])
        assert np.array_equal(first, again)  # chunk0 of the earlier run is still there: nothing was rewritten
        torch.cuda.synchronize()
        for c, d in zip(calls, dws):
            assert_exact(d[0].t, c.w0[0], "second round: pending")
        _run(host, sink.devt, 0, 2)
    finally:
        torch.cuda.synchronize()
        lib().call("cn_slice_sums_end")
    for c, d in zip(calls, dws):
        assert_exact(d[0].t, c.want(), "second round")
    grad.assert_untouched_outside("end and begin")


# ---------------------------------------------------------------------------------------------------------------------
# layer D: scratch.py on a whole step
# ---------------------------------------------------------------------------------------------------------------------

STEP = {"bf16-mixed": 2, "32-true": 4}  # precision -> batch (fp32 needs 4 images of 28 x 28 to reach 16 slices)


class _Spy:
    """Counts what scratch.py asks of the library during a pass: every cn_slice_sums_run (first, n, upload) and the
    largest cn_slice_sums_count it saw."""

    def __init__(self, monkeypatch):
        from cultionet_amd import _lib

        self.runs, self.max_count = [], -1
        call, query = _lib.call, _lib.query

        def spy_call(name, *args):
            if name == "cn_slice_sums_run":
                self.runs.append((args[2], args[3], args[4]))
            return call(name, *args)

        def spy_query(name, *args):
            v = query(name, *args)
            if name == "cn_slice_sums_count":
                self.max_count = max(self.max_count, v)
            return v

        monkeypatch.setattr(_lib, "call", spy_call)
        monkeypatch.setattr(_lib, "query", spy_query)


def _trainer(precision):
    from cultionet_amd.lightning import HipTrainer
    from oracle.selfcheck import build_pair

    lit, _ = build_pair(hidden=8, device="cuda:0")
    lit.train()
    return HipTrainer(lit, precision=precision)


def _batch(precision, hw=28):
    from cultionet_amd.data import Data
    from oracle import towerunet_oracle as O

    x, y, bdist = O.seeded_batch(STEP[precision], height=hw, width=hw, seed=3, with_mask=True)
    return Data(x=x.cuda(), y=y.cuda(), bdist=bdist.cuda())


def _pass(trainer, batch):
    """One forward + backward: (flat gradient on the host, records of the pass with dw as an offset into it)."""
    trainer.forward_backward(batch)
    torch.cuda.synchronize()
    g = trainer.store.flat_grad.detach().cpu().clone()
    assert not bool(g.isnan().any())
    st = trainer.store._slice_sums
    recs = R.read_records(st.host, 0, st.flushed)
    base = trainer.store.flat_grad.data_ptr()
    ranges = sorted(((int(r["dw"]) - base) // 4, int(r["n"])) for r in recs)
    for off, n in ranges:
        assert 0 <= off and off + n <= g.numel()
    return g, ranges, recs


_BASE: T.Dict[T.Tuple[str, int], T.Any] = {}


def _baseline(precision, hw=28):
    """The pass under the default settings on a fresh trainer (computed once, before any setting is patched)."""
    if (precision, hw) not in _BASE:
        from cultionet_amd import scratch

        assert scratch._DEFER_SUMS and scratch._SS_CAP == 512 and scratch._SS_BLOCK == 64 << 20
        g, ranges, recs = _pass(_trainer(precision), _batch(precision, hw))
        assert len(ranges) > 0, "no weight gradient was deferred"
        kinds = sorted({int(k) for k in recs["kind"]})
        print(f"STEP {precision} {hw}x{hw}: {len(ranges)} deferred sums, kinds {kinds}, "
              f"nslices {min(recs['nslices'])}..{max(recs['nslices'])}")
        _BASE[(precision, hw)] = (g, ranges)
    return _BASE[(precision, hw)]


def _compare(g, base, ranges, what):
    """Bitwise on the ranges the baseline deferred, 1e-5 of the gradient's scale elsewhere (few-split float atomics)."""
    inside = torch.zeros(base.numel(), dtype=torch.bool)
    for off, n in ranges:
        inside[off:off + n] = True
    a, b = g.view(torch.int32), base.view(torch.int32)
    diff = (a != b) & inside
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {int(inside.sum())} deferred gradient floats differ"
    tol = 1e-5 * float(base.abs().max())
    worst = float((g - base).abs().max())
    assert worst <= tol, f"{what}: max difference {worst:.3e} > {tol:.3e}"


@pytest.mark.parametrize("precision", ["bf16-mixed", "32-true"])
@pytest.mark.parametrize("variant", ["flush at every take", "final flush only", "table of 4", "tiny arena"])
def test_step_under_every_flush_setting(variant, precision, monkeypatch):
    from cultionet_amd import scratch

    base, ranges = _baseline(precision)
    name, value = {"flush at every take": ("_SS_FLUSH_FLOATS", 1), "final flush only": ("_SS_FLUSH_FLOATS", 0),
                   "table of 4": ("_SS_CAP", 4), "tiny arena": ("_SS_BLOCK", 1 << 14)}[variant]
    monkeypatch.setattr(scratch, name, value)
    spy = _Spy(monkeypatch)
    trainer = _trainer(precision)
    g, vranges, _ = _pass(trainer, _batch(precision))
    print(f"STEP {precision} {variant}: runs (first, n, upload) {spy.runs}, largest count {spy.max_count}")
    what = f"{precision}, {variant}"
    if variant == "flush at every take":
        assert len(spy.runs) > 1, "the pass was meant to flush more than once"
        assert any(first > 0 for first, _, _ in spy.runs)
        assert vranges == ranges
    elif variant == "final flush only":
        assert len(spy.runs) == 1 and spy.runs[0][:2] == (0, len(ranges))
    elif variant == "table of 4":
        assert spy.max_count == 4 and len(vranges) == 4 and len(ranges) > 4
        assert sum(n for _, n, _ in spy.runs) == 4
    else:
        st = trainer.store._slice_sums
        assert vranges == ranges
        sizes = [b.numel() for b in st.blocks]
        print(f"STEP {what}: arena blocks {sizes}")
        assert len(sizes) > 1 and min(sizes) > (1 << 14), "every request is oversized and the pass changes blocks"
        _compare(g, base, ranges, what)
        g, vranges, _ = _pass(trainer, _batch(precision))  # again over the blocks that are there now
        assert vranges == ranges and [b.numel() for b in st.blocks] == sizes
    _compare(g, base, ranges, what)


def test_step_tiny_arena_flushed_at_every_take(monkeypatch):
    """Both at once in fp32, whose requests differ in size (odd planes add room for aligned copies): every flush hands
    the arena back, so a larger request meets block 0 empty and too small and replaces it."""
    from cultionet_amd import scratch

    precision = "32-true"
    base, ranges = _baseline(precision)
    monkeypatch.setattr(scratch, "_SS_BLOCK", 1 << 14)
    monkeypatch.setattr(scratch, "_SS_FLUSH_FLOATS", 1)
    needs = []
    take = scratch._SliceSums.take

    def spy_take(self, need):
        needs.append(int(need))
        return take(self, need)

    monkeypatch.setattr(scratch._SliceSums, "take", spy_take)
    trainer = _trainer(precision)
    g, vranges, _ = _pass(trainer, _batch(precision))
    st = trainer.store._slice_sums
    print(f"STEP tiny arena + flush at every take: {len(needs)} requests of {min(needs)}..{max(needs)} floats, "
          f"blocks {[b.numel() for b in st.blocks]}")
    assert vranges == ranges
    assert max(needs) > needs[0], "the pass was meant to ask for more than its first request"
    assert st.blocks[0].numel() >= max(needs)
    _compare(g, base, ranges, "32-true, tiny arena flushed at every take")


@pytest.mark.parametrize("flush", [None, 1])
def test_step_upload_cache_across_shapes(flush, monkeypatch):
    """One trainer, 28 x 28, 20 x 20, 28 x 28 and 28 x 28 again: the device table is rewritten for the other shape in
    between, and the cache of uploaded ranges must notice. With a flush at every take the ranges differ between the
    shapes."""
    from cultionet_amd import scratch

    precision = "bf16-mixed"
    base_a, ranges_a = _baseline(precision, 28)
    base_b, ranges_b = _baseline(precision, 20)
    if flush is not None:
        monkeypatch.setattr(scratch, "_SS_FLUSH_FLOATS", flush)
    spy = _Spy(monkeypatch)
    trainer = _trainer(precision)
    a, b = _batch(precision, 28), _batch(precision, 20)
    out = []
    for batch in (a, b, a, a):
        spy.runs.clear()
        g, ranges, _ = _pass(trainer, batch)
        out.append((g, ranges, list(spy.runs)))
    print(f"UPLOADS flush={flush}: " + " | ".join(str([u for _, _, u in runs]) for _, _, runs in out))
    (g1, r1, _), (g2, r2, _), (g3, r3, _), (g4, r4, runs4) = out
    assert r1 == ranges_a and r3 == r1 and r4 == r1 and r2 == ranges_b
    _compare(g1, base_a, ranges_a, "first pass, 28 x 28")
    _compare(g2, base_b, ranges_b, "second pass, 20 x 20")
    _compare(g3, g1, r1, "third pass, 28 x 28 after 20 x 20")
    _compare(g4, g1, r1, "fourth pass, 28 x 28 again")
    # the fourth pass appends the records of the third at the same addresses: nothing to upload
    assert runs4 and all(u == 0 for _, _, u in runs4), runs4
