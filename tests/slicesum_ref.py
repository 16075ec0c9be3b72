"""Plain restatement of the deferred weight-gradient slice sums (cultionet_amd/csrc/cn_slicesum.h, cn_slicesum.hip),
shared by tests/test_slicesum_ref.py (CPU) and tests/test_slice_sums_exact_gpu.py.

One record of the table says: add `nslices` partial slices into one weight gradient,

    kind 0:  dw[i]                    += sum_s part[s*stride + i]                       i < n
    kind 1:  dw[(cp*CQ + cq)*T + t]   += sum_s part[s*stride + (t*CPp + cp)*CQp + cq]   t < T, cp < CP, cq < CQ

(kind 1: a bf16 weight gradient; its slices are [T][CPp][CQp] with CPp, CQp padded to multiples of 64, and the
destination is the [CP][CQ][T] weight). `apply` below computes that in float64 over plain numpy buffers; `chunks` /
`deal` restate how the one launch deals its blocks to the records; `depth` counts the fp32 additions on the longest
path to one output, which is what the bounded tests multiply 2^-24 with.
"""
from __future__ import annotations

import numpy as np

# struct CnSliceSum, little-endian, no padding (two pointers, two longs, eight ints)
REC = np.dtype([("part", "<u8"), ("dw", "<u8"), ("slice_stride", "<i8"), ("n", "<i8"), ("nslices", "<i4"),
                ("kind", "<i4"), ("T", "<i4"), ("CP", "<i4"), ("CQ", "<i4"), ("CPp", "<i4"), ("CQp", "<i4"),
                ("chunk0", "<i4")])
HEAD = 60          # bytes of a record in front of chunk0 (which belongs to cn_slice_sums_run)
CHUNK_FLAT = 256   # outputs per block: kind 0 with at most 128 slices
CHUNK_WAVES = 64   # outputs per block: kind 0 with more than 128 slices, and kind 1
FLAT_MAX = 128     # most slices of the thread-per-output body

U32 = 2.0 ** -24


def body(kind: int, nslices: int) -> str:
    """Which of the kernel's three summation bodies a record takes."""
    if kind == 0:
        return "flat" if nslices <= FLAT_MAX else "waves"
    return "relayout"


def record(part: int, dw: int, stride: int, nslices: int, kind: int = 0, n: int = 0, T: int = 0, CP: int = 0,
           CQ: int = 0, CPp: int = 0, CQp: int = 0) -> np.ndarray:
    """One REC element. part / dw are addresses (bytes); kind 1 takes n from T * CP * CQ."""
    r = np.zeros((), dtype=REC)
    r["part"], r["dw"], r["slice_stride"], r["nslices"], r["kind"] = part, dw, stride, nslices, kind
    r["n"] = T * CP * CQ if kind == 1 else n
    r["T"], r["CP"], r["CQ"], r["CPp"], r["CQp"] = T, CP, CQ, CPp, CQp
    return r


def write_records(host_table, recs, first: int = 0) -> None:
    """Store records at [first, first + len(recs)) of a (pinned) uint8 torch tensor holding the host table."""
    recs = np.asarray(recs, dtype=REC).reshape(-1)
    tab = host_table.numpy().view(REC)
    assert first >= 0 and first + recs.size <= tab.size, "table too small"
    tab[first:first + recs.size] = recs


def read_records(host_table, first: int, n: int) -> np.ndarray:
    """A copy of records [first, first + n) of the host table."""
    return host_table.numpy().view(REC)[first:first + n].copy()


def chunks(rec) -> int:
    """Blocks of one record: cn_ss_chunks."""
    per = CHUNK_FLAT if body(int(rec["kind"]), int(rec["nslices"])) == "flat" else CHUNK_WAVES
    return (int(rec["n"]) + per - 1) // per


def deal(recs) -> list:
    """chunk0 of every record of ONE launch over `recs` (it restarts at 0 for every range that is run), and the
    launch's block count behind them: [c0, c1, ..., blocks]."""
    out, blocks = [], 0
    for r in recs:
        out.append(blocks)
        blocks += chunks(r)
    return out + [blocks]


def indices(kind: int, n: int = 0, T: int = 0, CP: int = 0, CQ: int = 0, CPp: int = 0, CQp: int = 0):
    """(src, dst): offsets inside one slice and inside dw of every output, as int64 arrays of equal length."""
    if kind == 0:
        i = np.arange(n, dtype=np.int64)
        return i, i
    t, cp, cq = np.meshgrid(np.arange(T, dtype=np.int64), np.arange(CP, dtype=np.int64),
                            np.arange(CQ, dtype=np.int64), indexing="ij")
    src = (t * CPp + cp) * CQp + cq
    dst = (cp * CQ + cq) * T + t
    return src.reshape(-1), dst.reshape(-1)


def apply(part: np.ndarray, part_off: int, dw: np.ndarray, dw_off: int, stride: int, nslices: int, kind: int = 0,
          n: int = 0, T: int = 0, CP: int = 0, CQ: int = 0, CPp: int = 0, CQp: int = 0, absolute: bool = False) -> None:
    """dw[dw_off + dst] += sum_s part[part_off + s*stride + src] in float64, in place. part / dw: 1-D float64 buffers,
    offsets in elements. absolute: sum |part| instead (the bound's scale; dw should then hold |dw0|)."""
    assert part.dtype == np.float64 and dw.dtype == np.float64
    src, dst = indices(kind, n, T, CP, CQ, CPp, CQp)
    s = np.arange(nslices, dtype=np.int64)[:, None] * stride
    v = part[part_off + s + src[None, :]]
    dw[dw_off + dst] += (np.abs(v) if absolute else v).sum(axis=0)


def apply_f32(part: np.ndarray, part_off: int, dw: np.ndarray, dw_off: int, stride: int, nslices: int, kind: int = 0,
              n: int = 0, T: int = 0, CP: int = 0, CQ: int = 0, CPp: int = 0, CQp: int = 0) -> None:
    """The same sum in float32 WITH THE ASSOCIATION OF THE KERNEL (cn_slicesum.h), in place on float32 buffers: the
    header promises that every output is summed in the order of the immediate kernels, so a result on the device has
    to equal this one bit for bit (fp32 additions round to nearest even there as here; there is nothing to contract).

    flat:  s0 = 0 + p0 + p2 + ..., s1 = 0 + p1 + p3 + ..., an odd last slice goes to s0; dw += s0 + s1.
    waves: wave kg owns slices kg, kg + 4, ...; while k + 12 < nslices one turn adds p[k], p[k+4], p[k+8], p[k+12] to
           s0, s1, s2, s3, the rest go to s0 four apart; r[kg] = (s0 + s1) + (s2 + s3);
           dw += (r[0] + r[1]) + (r[2] + r[3])."""
    assert part.dtype == np.float32 and dw.dtype == np.float32
    src, dst = indices(kind, n, T, CP, CQ, CPp, CQp)
    p = lambda k: part[part_off + k * stride + src]
    zero = lambda: np.zeros(src.size, dtype=np.float32)
    if body(kind, nslices) == "flat":
        s0, s1 = zero(), zero()
        k = 0
        while k + 1 < nslices:
            s0 = s0 + p(k)
            s1 = s1 + p(k + 1)
            k += 2
        if k < nslices:
            s0 = s0 + p(k)
        total = s0 + s1
    else:
        r = []
        for kg in range(4):
            s0, s1, s2, s3 = zero(), zero(), zero(), zero()
            k = kg
            while k + 12 < nslices:
                s0 = s0 + p(k)
                s1 = s1 + p(k + 4)
                s2 = s2 + p(k + 8)
                s3 = s3 + p(k + 12)
                k += 16
            while k < nslices:
                s0 = s0 + p(k)
                k += 4
            r.append((s0 + s1) + (s2 + s3))
        total = (r[0] + r[1]) + (r[2] + r[3])
    assert total.dtype == np.float32
    dw[dw_off + dst] = dw[dw_off + dst] + total


def depth(kind: int, nslices: int) -> int:
    """Additions on the longest chain from a slice value (or the old dw) to one output, counted from cn_slicesum.h.
    Every addition the code executes on that chain counts, the first `0.f + x` of an accumulator included.

    flat (kind 0, nslices <= 128), cn_ss_chunk_flat: s0 takes slices 0, 2, 4, ... (the pair loop's first statement and
    the odd tail), s1 takes 1, 3, ...; the longer chain is s0 with ceil(nslices / 2) additions. Then `s0 + s1` (1) and
    `dw[i] +=` (1):
        depth = ceil(nslices / 2) + 2.

    waves (kind 0 above 128 slices, and kind 1), cn_ss_chunk_waves: wave kg (0..3) takes slices kg, kg + 4, kg + 8, ...,
    m = ceil((nslices - kg) / 4) of them (0 if kg >= nslices). The 16-step loop runs while k + 12 < nslices, that is
    full = ceil((nslices - 12 - kg) / 16) times (0 if negative), and adds one slice to each of s0..s3 per turn; the
    4-step tail adds the m - 4 * full slices left (at most 3) to s0. So s0 is the longest accumulator with
    full + m - 4 * full additions. Behind it `(s0 + s1) + (s2 + s3)` is 2 additions deep, the LDS combine
    `(red0 + red1) + (red2 + red3)` 2 more, and `dw[dst] +=` 1:
        depth = max over kg of (m - 3 * full) + 5.
    The maximum is not always wave 0: with 13 slices wave 0 runs the 16-step loop once (1 addition) while wave 1 adds
    slices 1, 5, 9 in the tail (3 additions).

    With d additions the fp32 result differs from the exact sum by at most ((1 + u)^d' - 1) * sum|terms|, u = 2^-24,
    where d' < d is the number of additions that can round (at least one addition of every chain adds to an exact zero).
    (1 + u)^d' - 1 <= d * u while d'^2 * u <= 1, which holds for every slice count a 512-record table of real layers can
    carry (d' < 4096).
    """
    if nslices < 1:
        return 0
    if body(kind, nslices) == "flat":
        return (nslices + 1) // 2 + 2
    longest = 0
    for kg in range(4):
        m = max(0, -(-(nslices - kg) // 4))
        full = max(0, -(-(nslices - 12 - kg) // 16))
        longest = max(longest, m - 3 * full)
    return longest + 5
