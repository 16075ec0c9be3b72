"""The float64 restatement of the deferred slice sums (tests/slicesum_ref.py) checked on the CPU: record layout, block
dealing and summation depth on hand-computed cases, the two index maps on arrays small enough to write down."""
import inspect
import struct

import numpy as np
import pytest
import torch

import slicesum_ref as R


def test_record_layout_matches_the_struct_and_the_engine():
    assert R.REC.itemsize == 64
    offs = {name: R.REC.fields[name][1] for name in R.REC.names}
    assert offs == {"part": 0, "dw": 8, "slice_stride": 16, "n": 24, "nslices": 32, "kind": 36, "T": 40, "CP": 44,
                    "CQ": 48, "CPp": 52, "CQp": 56, "chunk0": 60}
    assert offs["chunk0"] == R.HEAD
    # the fields _SliceSums._commit reads from the raw table
    from cultionet_amd import scratch

    fmt = "<QQqqi"
    assert f'"{fmt}"' in inspect.getsource(scratch._SliceSums._commit)
    r = R.record(part=0x7F0012345670, dw=0x7F00ABCDEF04, stride=576, nslices=28, kind=0, n=575)
    assert struct.unpack_from(fmt, r.tobytes(), 0) == (0x7F0012345670, 0x7F00ABCDEF04, 576, 575, 28)
    walk = 0
    for name, code in zip(("part", "dw", "slice_stride", "n", "nslices"), "QQqqi"):
        assert offs[name] == walk, name
        walk += struct.calcsize("<" + code)
    k1 = R.record(part=64, dw=128, stride=9 * 64 * 128, nslices=5, kind=1, T=9, CP=33, CQ=65, CPp=64, CQp=128)
    assert int(k1["n"]) == 9 * 33 * 65
    assert struct.unpack_from("<8i", k1.tobytes(), 32) == (5, 1, 9, 33, 65, 64, 128, 0)


def test_write_and_read_records_in_a_byte_table():
    host = torch.zeros(4 * 64, dtype=torch.uint8)
    a = R.record(part=16, dw=32, stride=7, nslices=3, kind=0, n=5)
    b = R.record(part=48, dw=64, stride=64 * 64, nslices=2, kind=1, T=1, CP=2, CQ=3, CPp=64, CQp=64)
    R.write_records(host, [a, b], first=1)
    assert bytes(host[:64].numpy()) == bytes(64) and bytes(host[192:].numpy()) == bytes(64)
    assert bytes(host[64:128].numpy()) == a.tobytes() and bytes(host[128:192].numpy()) == b.tobytes()
    got = R.read_records(host, 1, 2)
    assert got[0] == a and got[1] == b
    with pytest.raises(AssertionError):
        R.write_records(host, [a, b], first=3)


@pytest.mark.parametrize("n,flat,waves", [(1, 1, 1), (64, 1, 1), (65, 1, 2), (256, 1, 4), (257, 2, 5), (1000, 4, 16)])
def test_chunks(n, flat, waves):
    assert R.chunks(R.record(0, 0, n, 128, kind=0, n=n)) == flat       # 256 outputs per block
    assert R.chunks(R.record(0, 0, n, 1, kind=0, n=n)) == flat
    assert R.chunks(R.record(0, 0, n, 129, kind=0, n=n)) == waves      # 64 outputs per block
    k1 = R.record(0, 0, 64 * 64, 1, kind=1, T=1, CP=1, CQ=n, CPp=64, CQp=(n + 63) // 64 * 64)
    assert R.chunks(k1) == waves                                       # kind 1: 64 whatever the slice count


def test_deal():
    recs = [R.record(0, 0, 1, 3, kind=0, n=1),                  # 1 block
            R.record(0, 0, 257, 128, kind=0, n=257),            # 2
            R.record(0, 0, 257, 129, kind=0, n=257),            # 5
            R.record(0, 0, 0, 2, kind=1, T=9, CP=3, CQ=7, CPp=64, CQp=64),   # 189 outputs: 3
            R.record(0, 0, 64, 300, kind=0, n=64)]              # 1
    assert R.deal(recs) == [0, 1, 3, 8, 11, 12]
    assert R.deal(recs[2:]) == [0, 5, 8, 9]                      # a range that starts later starts at block 0 again
    assert R.deal([]) == [0]


def _depth_by_walking(kind, nslices):
    """The loops of cn_slicesum.h transcribed statement by statement, counting the additions into each accumulator."""
    if kind == 0 and nslices <= 128:
        s0 = s1 = 0
        k = 0
        while k + 1 < nslices:
            s0 += 1
            s1 += 1
            k += 2
        if k < nslices:
            s0 += 1
        return max(s0, s1) + 1 + 1
    worst = 0
    for kg in range(4):
        s = [0, 0, 0, 0]
        k = kg
        while k + 12 < nslices:
            for a in range(4):
                s[a] += 1
            k += 16
        while k < nslices:
            s[0] += 1
            k += 4
        worst = max(worst, max(s))
    return worst + 2 + 2 + 1


def test_depth_hand_cases():
    # flat: ceil(n / 2) + 2
    assert [R.depth(0, n) for n in (1, 2, 3, 16, 127, 128)] == [3, 3, 4, 10, 66, 66]
    # waves, 129 slices: wave 0 has 33 slices = 8 turns of the 16-step loop + 1 in the tail -> 9, + 5
    assert R.depth(0, 129) == 14
    # 141 slices: wave 0 has 36 = 9 turns (k = 0..128, 128 + 12 < 141) + 0 -> 9; wave 1 has 35 = 8 turns + 3 -> 11
    assert R.depth(0, 141) == 16
    # 300 slices: 75 per wave = 18 turns + 3 in the tail -> 21
    assert R.depth(0, 300) == 26
    # kind 1 takes the waves body at every slice count: 1 slice -> 1 + 5; 13 slices: wave 1 adds 1, 5, 9 in the tail
    assert R.depth(1, 1) == 6
    assert R.depth(1, 13) == 8
    assert R.depth(1, 16) == 6 and R.depth(1, 17) == 7 and R.depth(1, 29) == 9
    assert R.depth(0, 0) == 0


def test_depth_closed_form_equals_the_transcribed_loops():
    for n in range(1, 700):
        assert R.depth(0, n) == _depth_by_walking(0, n), n
        assert R.depth(1, n) == _depth_by_walking(1, n), n


def test_body():
    assert [R.body(0, n) for n in (1, 128, 129)] == ["flat", "flat", "waves"]
    assert [R.body(1, n) for n in (1, 128, 129)] == ["relayout"] * 3


def test_apply_kind0_by_hand():
    part = np.full(40, np.nan)
    # 3 slices of 4 outputs, stride 6, first slice at 5: the two floats behind every slice stay NaN
    for s in range(3):
        part[5 + 6 * s:5 + 6 * s + 4] = [1 + s, 10 * (1 + s), -s, 0.5]
    dw = np.array([100.0, 7.0, -1.0, 2.0, 3.0, 100.0])
    R.apply(part, 5, dw, 1, stride=6, nslices=3, kind=0, n=4)
    assert dw.tolist() == [100.0, 7.0 + 6, -1.0 + 60, 2.0 - 3, 3.0 + 1.5, 100.0]
    ab = np.abs(np.array([100.0, 7.0, -1.0, 2.0, 3.0, 100.0]))
    R.apply(part, 5, ab, 1, stride=6, nslices=3, kind=0, n=4, absolute=True)
    assert ab.tolist() == [100.0, 13.0, 61.0, 5.0, 4.5, 100.0]


def test_apply_f32_keeps_the_kernels_association():
    big = float(2 ** 24)
    # flat, 4 slices of one output: s0 = p0 + p2, s1 = p1 + p3 -> (2^24 - 2^24) + (1 + 1) = 2; in slice order it is 1
    part = np.array([big, 1.0, -big, 1.0], dtype=np.float32)
    dw = np.array([0.0], dtype=np.float32)
    R.apply_f32(part, 0, dw, 0, stride=1, nslices=4, kind=0, n=1)
    assert dw.tolist() == [2.0]
    # waves, 13 slices of one output: wave 0 owns 0, 4, 8, 12 in ONE 16-step turn -> (p0 + p4) + (p8 + p12)
    # = (1 + 2^24 -> 2^24) + (1 - 2^24) = 1; as a chain ((p0 + p4) + p8) + p12 it would be 0, exactly it is 2
    part = np.zeros(13, dtype=np.float32)
    part[[0, 4, 8, 12]] = [1.0, big, 1.0, -big]
    dw = np.array([0.0], dtype=np.float32)
    R.apply_f32(part, 0, dw, 0, stride=1, nslices=13, kind=1, T=1, CP=1, CQ=1, CPp=1, CQp=1)
    assert dw.tolist() == [1.0]
    # wave 1 owns 1, 5, 9 in the 4-step tail: a chain
    part = np.zeros(13, dtype=np.float32)
    part[[1, 5, 9]] = [1.0, big, -big]
    dw = np.array([0.0], dtype=np.float32)
    R.apply_f32(part, 0, dw, 0, stride=1, nslices=13, kind=1, T=1, CP=1, CQ=1, CPp=1, CQp=1)
    assert dw.tolist() == [0.0]


@pytest.mark.parametrize("kind,nslices", [(0, 1), (0, 7), (0, 128), (0, 129), (0, 145), (1, 1), (1, 13), (1, 29)])
def test_apply_f32_equals_float64_on_integers(kind, nslices):
    rng = np.random.default_rng(nslices)
    T, CP, CQ, CPp, CQp = 3, 2, 5, 4, 8
    n = 37 if kind == 0 else T * CP * CQ
    extent = n if kind == 0 else T * CPp * CQp
    stride = extent + 3
    part = rng.integers(-8, 9, size=nslices * stride).astype(np.float64)
    dw0 = rng.integers(-8, 9, size=n + 2).astype(np.float64)
    a, b = dw0.copy(), dw0.astype(np.float32)
    kw = dict(stride=stride, nslices=nslices, kind=kind, n=n)
    if kind == 1:
        kw.update(T=T, CP=CP, CQ=CQ, CPp=CPp, CQp=CQp)
    R.apply(part, 0, a, 1, **kw)
    R.apply_f32(part.astype(np.float32), 0, b, 1, **kw)
    assert np.array_equal(a, b.astype(np.float64))
    assert a[0] == dw0[0] and a[-1] == dw0[-1]


def test_apply_kind1_by_hand():
    T, CP, CQ, CPp, CQp = 2, 2, 3, 4, 5
    stride = T * CPp * CQp + 3
    part = np.full(2 * stride + 1, np.nan)
    val = lambda s, t, cp, cq: 1000 * s + 100 * t + 10 * cp + cq
    for s in range(2):
        for t in range(T):
            for cp in range(CP):
                for cq in range(CQ):
                    part[1 + s * stride + (t * CPp + cp) * CQp + cq] = val(s, t, cp, cq)
    dw = np.full(T * CP * CQ + 2, -5.0)
    R.apply(part, 1, dw, 1, stride=stride, nslices=2, kind=1, T=T, CP=CP, CQ=CQ, CPp=CPp, CQp=CQp)
    assert dw[0] == -5.0 and dw[-1] == -5.0
    for cp in range(CP):
        for cq in range(CQ):
            for t in range(T):
                assert dw[1 + (cp * CQ + cq) * T + t] == -5.0 + val(0, t, cp, cq) + val(1, t, cp, cq)
    # the two maps are injective and the destination is dense
    src, dst = R.indices(1, T=T, CP=CP, CQ=CQ, CPp=CPp, CQp=CQp)
    assert sorted(dst.tolist()) == list(range(T * CP * CQ)) and len(set(src.tolist())) == T * CP * CQ
    assert not np.isnan(dw).any()
