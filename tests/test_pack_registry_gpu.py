"""The packed-weight registry of ParamStore on the device: which copies one batched repack refreshes (all of them, or
those of the parameters a masked ``bump`` names), that the others keep their bits, that the descriptor tables keep their
addresses from step to step (launch plans bake them in) until a registration invalidates them, and that a plan being
recorded keeps every table it saw alive. Only weights are touched: no activation, no convolution launch.

Every comparison is of raw bits against a fresh single pack (cn_pack_weights_{f32,bf16}) of the current weights into a
NaN-filled buffer, with the stride tuples written out here."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

BATCHED = "cn_pack_weights_batched_"


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _setup():
    """(modules, store, holders): three layers, twelve registered copies (forward / backward-data, fp32 / bf16)."""
    from cultionet_amd import engine as E

    torch.manual_seed(0)
    mods = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3), torch.nn.Conv2d(16, 8, 1),
                               torch.nn.ConvTranspose2d(8, 8, 3, stride=2)).to(_dev())
    store = E.ParamStore(mods)
    with E.using_store(store):
        for bf16 in (False, True):
            E.packed_conv(mods[0], True, bf16)
            E.packed_conv(mods[1], True, bf16)
            E.packed_convT(mods[2], True, bf16)
    return mods, store, [m.__dict__["_cn_packed"] for m in mods]


def _tuples(mod):
    """(forward, backward-data) pack arguments (T, K, N, sk, sn, st) of a layer's weight."""
    w = mod.weight
    T_ = int(w[0, 0].numel())
    if isinstance(mod, torch.nn.ConvTranspose2d):
        cin, cout = w.shape[0], w.shape[1]
        return (T_, cin, cout, cout * T_, T_, 1), (T_, cout, cin, T_, cout * T_, 1)
    cout, cin = w.shape[0], w.shape[1]
    return (T_, cin, cout, T_, cin * T_, 1), (T_, cout, cin, cin * T_, T_, 1)


def _bits(t):
    return t.detach().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _fresh(mod):
    """The four copies (fwd, bwd, fwd16, bwd16) of the layer's CURRENT weight, packed one by one, as raw bits."""
    from cultionet_amd import _lib

    s = torch.cuda.current_stream().cuda_stream
    w, out = mod.weight, []
    for name, dtype in (("cn_pack_weights_f32", torch.float32), ("cn_pack_weights_bf16", torch.bfloat16)):
        for (T_, K, N, sk, sn, st) in _tuples(mod):
            if dtype == torch.float32:
                n = T_ * _lib.query("cn_conv_kpad", K) * _lib.query("cn_conv_npad", N)
            else:
                n = _lib.query("cn_bconv_packed_elems", T_, K, N)
            buf = torch.full((n,), float("nan"), dtype=dtype, device=w.device)
            _lib.call(name, w.data_ptr(), buf.data_ptr(), T_, K, N, sk, sn, st, s)
            out.append(buf)
    torch.cuda.synchronize()
    return [_bits(b) for b in out]


def _copies(pw):
    torch.cuda.synchronize()
    return [_bits(t) for t in (pw.fwd, pw.bwd, pw.fwd16, pw.bwd16)]


def _overwrite(store, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in store.params:
            p.copy_(torch.randn(p.shape, generator=g).to(p.device))


@contextlib.contextmanager
def _captured():
    """The batched repack launches, intercepted the way a launch plan is recorded: [(entry point, table, count)]."""
    from cultionet_amd import _lib

    orig, log = _lib.call, []

    def call(name, *args):
        if name.startswith(BATCHED):
            log.append((name, args[0], args[1]))
        return orig(name, *args)

    _lib.call = call
    try:
        yield log
    finally:
        _lib.call = orig


def _repack(store, mods, mask=None):
    """bump + the first layer's lookup (what the next forward does first) -> the launches this caused."""
    from cultionet_amd import engine as E

    store.bump(mask)
    with _captured() as log, E.using_store(store):
        E.packed_conv(mods[0], True)
    return log


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_full_partial_stable_invalidated():
    from cultionet_amd import engine as E

    mods, store, holders = _setup()
    assert all(t is not None for pw in holders for t in (pw.fwd, pw.bwd, pw.fwd16, pw.bwd16))

    # full: one launch per precision, bf16 first, every record
    _overwrite(store, 1)
    log = _repack(store, mods)
    assert [(n, c) for n, _t, c in log] == [(BATCHED + "bf16", 6), (BATCHED + "f32", 6)]
    for m, pw in zip(mods, holders):
        assert _same(_copies(pw), _fresh(m)), type(m).__name__

    # partial: only the second layer's weight is named
    before = [_copies(pw) for pw in holders]
    _overwrite(store, 2)
    mask = tuple(p is mods[1].weight for p in store.params)
    assert sum(mask) == 1
    keep = []
    with E.holding_allocations(keep):  # (as a plan being recorded does: no table's address is handed out twice below)
        log = _repack(store, mods, mask)
        assert [(n, c) for n, _t, c in log] == [(BATCHED + "bf16", 2), (BATCHED + "f32", 2)]
        assert _same(_copies(holders[1]), _fresh(mods[1]))
        assert not _same(_copies(holders[1]), before[1])
        for i in (0, 2):
            assert _same(_copies(holders[i]), before[i]), i
            assert not _same(before[i], _fresh(mods[i])), i  # (their weights did change: the copies are stale on purpose)

        # the same dirty set again: the same tables
        again = _repack(store, mods, mask)
        assert again == log

        # one more registered copy (the second layer seen anew: an fp32 forward copy): new tables
        del mods[1].__dict__["_cn_packed"]
        with E.using_store(store):
            E.packed_conv(mods[1], False)
        new = _repack(store, mods, mask)
        assert [(n, c) for n, _t, c in new] == [(BATCHED + "bf16", 2), (BATCHED + "f32", 3)]
        assert new[0][1] != log[0][1] and new[1][1] != log[1][1]
        assert _same(_copies(holders[1]), _fresh(mods[1]))
        torch.cuda.synchronize()
        assert torch.equal(_bits(mods[1].__dict__["_cn_packed"].fwd), _fresh(mods[1])[0])


def test_tables_are_held_by_open_sinks():
    """A plan being recorded bakes the table pointers into its launches: every table a repack uses, of everything or
    of a dirty set, is handed to the open allocation sinks."""
    from cultionet_amd import engine as E

    mods, store, _holders = _setup()
    mask = tuple(p is mods[1].weight for p in store.params)
    sink = []
    with E.holding_allocations(sink):
        full = _repack(store, mods)
        part = _repack(store, mods, mask)
    assert len(full) == 2 and len(part) == 2
    held = {t.data_ptr() for t in sink if isinstance(t, torch.Tensor)}
    assert {t for _n, t, _c in part} <= held, "partial tables"
    assert {t for _n, t, _c in full} <= held, "full tables"
