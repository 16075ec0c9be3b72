"""The packed-weight registry of ParamStore without a device: the bytes of the two descriptor records against the C
structs (CnPackDesc in csrc/cn_conv.hip, CnBPackDesc in csrc/cn_bconv.hip), which records a set of changed parameters
selects, and how the backward-data copy's arguments follow from the forward copy's. The library is loaded for its pure
host helpers only (cn_conv_kpad / cn_conv_npad): no compute is launched."""
import os
import struct

import pytest


@pytest.fixture(scope="module")
def lib():
    from cultionet_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g

        g.build()
    _lib.load()
    return _lib


# (w ptr, dst ptr, T, K, N, sk, sn, st): a 3x3 Conv2d 12 -> 130 forward copy, a 2x2 ConvTranspose2d backward-data copy
RECORDS = [(0x7F0000001000, 0x7F00000A2000, 9, 12, 130, 9, 108, 1), (0x10, 0xFFFFFFFFFFF0, 4, 40, 3, 4, 160, 1)]


def test_record_layout_f32(lib):
    from cultionet_amd import engine as E

    for (w, d, T_, K, N, sk, sn, st) in RECORDS:
        kp, np_ = lib.query("cn_conv_kpad", K), lib.query("cn_conv_npad", N)
        assert kp >= K and np_ >= N
        want = struct.pack("<QQiiiiiiqqq", w, d, T_, K, N, kp, np_, 0, sk, sn, st)
        got = E.PACK_F32.record(w, d, T_, K, N, sk, sn, st)
        assert len(got) == 64 and bytes(got) == want
        assert E.PACK_F32.elems(T_, K, N) == T_ * kp * np_


def test_record_layout_bf16():
    from cultionet_amd import engine as E

    for (w, d, T_, K, N, sk, sn, st) in RECORDS:
        want = struct.pack("<QQiiiiiiqqqQ", w, d, T_, K, N, (K + 15) // 16, (N + 31) // 32, 0, sk, sn, st, 0)
        got = E.PACK_BF16.record(w, d, T_, K, N, sk, sn, st)
        assert len(got) == 72 and bytes(got) == want


def test_formats_name_their_entry_points():
    import torch

    from cultionet_amd import _lib, engine as E

    for fmt, suffix, dtype in ((E.PACK_F32, "f32", torch.float32), (E.PACK_BF16, "bf16", torch.bfloat16)):
        assert fmt.pack == "cn_pack_weights_" + suffix and fmt.batched == "cn_pack_weights_batched_" + suffix
        assert fmt.pack in _lib.SIGNATURES and fmt.batched in _lib.SIGNATURES
        assert fmt.dtype == dtype


def test_selection():
    """Padded parameter slices adjacent at 0, 8, 24, 40, 56; the third record is a declared group of two parameters
    (2 and 3) packed as one tensor."""
    from cultionet_amd.engine import select_packs

    offsets = [0, 8, 24, 40, 56]
    spans = [(0, 8), (8, 24), (24, 56)]
    assert select_packs(offsets, spans, {3}) == [2]
    assert select_packs(offsets, spans, {2}) == [2]
    assert select_packs(offsets, spans, {0, 1}) == [0, 1]
    assert select_packs(offsets, spans, frozenset()) == []
    assert select_packs(offsets, spans, {4}) == []
    assert select_packs(offsets, spans, None) == [0, 1, 2]
    # a source that starts inside a parameter (a view of part of it) still belongs to that parameter
    assert select_packs(offsets, [(12, 20)], {1}) == [0] and select_packs(offsets, [(12, 20)], {0, 2}) == []


def test_backward_data_exchange(monkeypatch):
    """The arguments packed_conv / packed_convT pack with, in both precisions: the forward tuple and the backward-data
    tuple derived from it, against the tuples written out per layer kind."""
    import torch

    from cultionet_amd import engine as E, params

    calls = []  # (packed_conv / packed_convT look _pack and _holder up where they live: cultionet_amd/params.py)
    monkeypatch.setattr(params, "_pack", lambda fmt, w, *dims: calls.append((fmt, dims)) or torch.empty(0))
    monkeypatch.setattr(params, "_holder", lambda mod: E.PackedWeight())  # (no store: nothing is registered)

    def packed(fn, mod, **kw):
        del calls[:]
        pw = fn(mod, True, **kw)
        fmts = {f for f, _ in calls}
        assert len(calls) == 2 and len(fmts) == 1
        (fmt,) = fmts
        got = (pw.fwd16, pw.bwd16, pw.fwd, pw.bwd) if fmt is E.PACK_BF16 else (pw.fwd, pw.bwd, pw.fwd16, pw.bwd16)
        assert got[0] is not None and got[1] is not None and got[2] is None and got[3] is None
        return fmt, calls[0][1], calls[1][1]

    cout, cin, taps = 24, 10, 9  # Conv2d weight [Cout][Cin][3][3]
    conv = torch.nn.Conv2d(cin, cout, 3)
    for bf16, fmt in ((False, E.PACK_F32), (True, E.PACK_BF16)):
        assert packed(E.packed_conv, conv, bf16=bf16) == (fmt, (taps, cin, cout, taps, cin * taps, 1),
                                                          (taps, cout, cin, cin * taps, taps, 1))
    cin, cout, taps = 10, 24, 4  # ConvTranspose2d weight [Cin][Cout][2][2]
    convT = torch.nn.ConvTranspose2d(cin, cout, 2, stride=2)
    for bf16, fmt in ((False, E.PACK_F32), (True, E.PACK_BF16)):
        assert packed(E.packed_convT, convT, bf16=bf16) == (fmt, (taps, cin, cout, cout * taps, taps, 1),
                                                            (taps, cout, cin, taps, cout * taps, 1))
    n = cout * taps  # the same as the [Cin][Cout*KH*KW] matrix of a 1x1 transposed convolution (fp32 only)
    want = (E.PACK_F32, (1, cin, n, n, 1, 0), (1, n, cin, 1, n, 0))
    assert packed(E.packed_convT, convT, taps_as_channels=True) == want
    assert E._bwd_data_dims(*want[1]) == want[2] and E._bwd_data_dims(*want[2]) == want[1]
