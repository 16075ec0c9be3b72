"""The engine's layers without a device: runtime -> params -> scratch -> tape -> engine import one way only, ``engine``
still binds every name the rest of the repository reaches through it, the two flags that are rebound at run time have
one home, and the per-thread state starts from its declared defaults in every thread."""
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Every ``engine.<name>`` used outside engine.py (package, tests, tools, bench.py) when the engine was split.
ENGINE_NAMES = tuple("""
    ACT_NONE ACT_SILU LOSS_KINDS MSK_F32 MSK_I64 MSK_LABEL MSK_NONE PACK_BF16 PACK_F32 PackedWeight ParamStore
    SEG_CHUNK TGT_EQ TGT_FLOAT TGT_ONEHOT TGT_RANGE Tape Var _EVAL_FUSION _OVERLAP_WGRAD _SliceSums
    _bn_group_uniform _bn_stats_epoch _bwd_data_dims _check _conv_ws _dense16 _keepalive _lib _note_bn_update
    _pad_ws _py_op _recorder _rng _state _stream _thin_conv3x3_bf16 adaptive_max_pool2d add alloc
    aux_stream_events begin_branch_backward begin_rng_step bf16_enabled bn_act bn_act_group branch_streams
    branch_streams_allowed bstride can_fuse_eval cat_channels conv2d conv2d_group conv_bn_act_eval
    conv_transpose2d current_store deferring_slice_sums dropout eval_fusion final_combine flush_slice_sums
    grad_buffer holding_allocations is16 join join_channels join_side_stream layer_norm_c manual_seed
    mixed_precision na2d new_buffer overlap_wgrad packed_conv packed_convT pretime_reduction recording
    release_branches resize_bilinear segment_table side_stream_event spatial_channel_attention spawn
    split_channels tanimoto_loss tanimoto_loss_multi thin_conv3x3 time_conv to_bf16 trainable_segments
    using_store workspace_epoch
""".split())

_IMPORT_ORDER = """
import importlib, sys
layers = ["runtime", "params", "scratch", "tape", "engine"]
for i, name in enumerate(layers[:-1]):
    importlib.import_module("cultionet_amd." + name)
    later = [m for m in layers[i + 1:] if "cultionet_amd." + m in sys.modules]
    assert not later, (name, later)
"""


def test_layers_import_one_way():
    """Each infrastructure module imports in a fresh interpreter before the ones below it -- and before ``engine`` --
    have been imported: nothing points downward."""
    r = subprocess.run([sys.executable, "-c", _IMPORT_ORDER], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_engine_binds_every_name_in_use():
    from cultionet_amd import engine as E

    assert len(ENGINE_NAMES) == len(set(ENGINE_NAMES))
    missing = [n for n in ENGINE_NAMES if not hasattr(E, n)]
    assert not missing, missing


def test_rebound_flags_have_one_home():
    from cultionet_amd import engine as E, runtime

    prev = E.overlap_wgrad(False)
    try:
        assert E._OVERLAP_WGRAD is False and runtime._OVERLAP_WGRAD is False
    finally:
        E.overlap_wgrad(prev)
    assert E._OVERLAP_WGRAD is prev and runtime._OVERLAP_WGRAD is prev

    plan, seen = [], []
    runtime._recorder = plan
    try:
        E._py_op(seen.append, 7)
        assert E._recorder is plan
    finally:
        runtime._recorder = None
    assert seen == [7] and plan == [(1, seen.append, (7,))]
    assert E._recorder is None


def test_thread_state_defaults_are_per_thread():
    from cultionet_amd import engine as E

    seen = {}

    def fresh():
        seen["bf16"], seen["no_branches"] = E.bf16_enabled(), E._state.no_branches

    with E.mixed_precision(True), E.branch_streams(False):
        assert E.bf16_enabled() is True and E._state.no_branches is True
        t = threading.Thread(target=fresh)
        t.start()
        t.join()
    assert seen == {"bf16": False, "no_branches": False}
    assert E.bf16_enabled() is False and E._state.no_branches is False
