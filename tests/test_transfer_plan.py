"""Host-side plans of training with frozen parameters (no GPU): the segment table of the segmented optimizer step, the
gradient buckets over trainable ranges, and the trainable set in the launch-plan / bucket-plan keys."""
import struct
import types

import torch

from cultionet_amd import engine as E
from cultionet_amd.ddp import GradientAllReduce, plan_buckets


def _layout(sizes):
    offs, n = [], 0
    for s in sizes:
        offs.append(n)
        n += (s + 3) // 4 * 4
    return offs, n


def test_runs_merge_across_padding_and_split_on_step_counts():
    sizes = [5, 3, 8, 2, 6]
    offs, _ = _layout(sizes)  # 0, 8, 12, 20, 24
    segs = E.trainable_segments(offs, sizes, [True] * 5, [3] * 5)
    assert segs == [(0, 24 + 6, 3)]  # one run, the padding after 5 / 3 / 2 elements inside it
    segs = E.trainable_segments(offs, sizes, [True] * 5, [3, 3, 1, 1, 3])
    assert segs == [(0, 11, 3), (12, 10, 1), (24, 6, 3)]


def test_frozen_parameter_splits_a_run():
    sizes = [4, 4, 4, 4]
    offs, _ = _layout(sizes)
    assert E.trainable_segments(offs, sizes, [True, False, True, True], [1] * 4) == [(0, 4, 1), (8, 8, 1)]
    assert E.trainable_segments(offs, sizes, [False, True, False, False], [7] * 4) == [(4, 4, 7)]


def test_empty_trainable_set_gives_no_segments():
    sizes = [4, 9]
    offs, _ = _layout(sizes)
    assert E.trainable_segments(offs, sizes, [False, False], [0, 0]) == []
    raw, chunks = E.segment_table([])
    assert raw == b"" and chunks == 0


def test_segment_table_records_and_chunk_prefix():
    segs = [(0, 1, 2), (8, 2 * E.SEG_CHUNK + 1, 5), (20000, 3, 1)]
    raw, chunks = E.segment_table(segs)
    assert len(raw) == 24 * 3
    recs = [struct.unpack_from("<qqii", raw, 24 * i) for i in range(3)]
    assert recs == [(0, 1, 2, 0), (8, 2 * E.SEG_CHUNK + 1, 5, 1), (20000, 3, 1, 4)]
    assert chunks == 5


def _covered(buckets):
    cov = set()
    for lo, hi, _ in buckets:
        assert lo < hi
        new = set(range(lo, hi))
        assert not (cov & new), "buckets overlap"
        cov |= new
    return cov


def test_plan_buckets_over_a_trainable_subset_covers_exactly_the_trainable_elements():
    sizes = [64, 130, 7, 256, 64, 33, 100]
    offs, total = _layout(sizes)
    ready = [6, 5, 4, 3, 2, 1, 0]
    trainable = [False, True, True, False, True, True, False]
    plan = plan_buckets(offs, sizes, ready, total, 50, trainable)
    cov = _covered(plan)
    want = set()
    for i, (o, s) in enumerate(zip(offs, sizes)):
        slot = set(range(o, o + (s + 3) // 4 * 4))  # a parameter's padded slice
        if trainable[i]:
            want |= slot
        else:
            assert not (cov & slot), f"a bucket covers frozen parameter {i}"
    assert cov == want
    for lo, hi, r in plan:  # ready = the earliest forward node among the bucket's parameters
        inside = [ready[i] for i, o in enumerate(offs) if lo <= o < hi]
        assert inside and r == min(inside)
    # every parameter trainable: the plan of the unfrozen model, unchanged
    assert plan_buckets(offs, sizes, ready, total, 50, [True] * 7) == plan_buckets(offs, sizes, ready, total, 50)


def test_bucket_plan_key_follows_requires_grad():
    ps = [torch.nn.Parameter(torch.zeros(8)) for _ in range(3)]
    offs, total = _layout([8, 8, 8])
    store = types.SimpleNamespace(params=ps, offsets=offs, numel=total,
                                  trainable_mask=lambda: tuple(p.requires_grad for p in ps))
    tape = types.SimpleNamespace(nodes=[None] * 4, marks={0: 2, 8: 1, 16: 0})
    ar = GradientAllReduce(world_size=1, bucket_mb=1.0)
    full = ar._get_plan(tape, store)
    assert full == [(0, total, 0)]
    ps[0].requires_grad_(False)
    part = ar._get_plan(tape, store)
    assert part == [(8, total, 0)] and ar._plan_key != (4, total, (True, True, True))
    ps[0].requires_grad_(True)
    assert ar._get_plan(tape, store) == full


def test_step_key_follows_requires_grad():
    from cultionet_amd import replay as R

    # step_key names the current stream of x.device; the tensors here live on the CPU, for which torch has no stream
    # (with a GPU present the real function raises on a CPU device). A stand-in on every machine: no GPU is touched.
    orig = torch.cuda.current_stream
    try:
        torch.cuda.current_stream = lambda device=None: types.SimpleNamespace(cuda_stream=0)
        ps = [torch.nn.Parameter(torch.zeros(4)) for _ in range(2)]
        store = types.SimpleNamespace(uid=1, params=ps, trainable_mask=lambda: tuple(p.requires_grad for p in ps))
        tr = types.SimpleNamespace(store=store, bf16=False, lit=types.SimpleNamespace(loss_name="TanimotoDistLoss"))
        batch = types.SimpleNamespace(x=torch.zeros(1, 3), y=torch.zeros(1), bdist=torch.zeros(1))
        k1 = R.step_key(tr, batch)
        ps[1].requires_grad_(False)
        k2 = R.step_key(tr, batch)
        ps[1].requires_grad_(True)
        assert k1 != k2 and R.step_key(tr, batch) == k1
    finally:
        torch.cuda.current_stream = orig
