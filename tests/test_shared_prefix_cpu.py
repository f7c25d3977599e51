"""A batch's shared prompt prefix, the parts that need no device: the rule that finds it on id lists (trace_amd/prefix.py), the default
batch threshold, and the three new C-ABI names in both libraries."""
import os

import pytest

from trace_amd.prefix import SHARE_PREFIX_MIN_BATCH, shared_prefix_len

V, IMG, SYNC = -201, -200, -205
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("trace_decode_set_shared_prefix", "trace_op_attn_decode_shared", "trace_llm_prefill_shared")


def test_one_question_for_every_video_shares_the_ids_before_the_placeholder():
    q = [1, 7, 8, 9, V, 4, 5, SYNC]
    assert shared_prefix_len([q, q, q]) == 4
    assert shared_prefix_len([q, tuple(q)]) == 4
    assert shared_prefix_len([[1, 7, IMG, 4], [1, 7, IMG, 4]]) == 2        # the image placeholder expands to the encoded rows as well
    import numpy as np
    assert shared_prefix_len([np.array(q), np.array(q)]) == 4


def test_the_placeholder_inside_the_common_part_ends_the_prefix():
    """prompts that agree beyond <video>: the shared rows still end in front of it (the video's rows differ from sequence to sequence)"""
    a, b = [1, 2, 3, V, 6, 7, 8], [1, 2, 3, V, 6, 7, 9]
    assert a[:6] == b[:6] and shared_prefix_len([a, b]) == 3
    assert shared_prefix_len([a, a]) == 3
    assert shared_prefix_len([[1, 2, 3, V], [1, 2, 3, V, 5]]) == 3        # what follows the placeholder may differ in length too


def test_prompts_that_differ_before_the_placeholder_share_nothing():
    assert shared_prefix_len([[1, 2, 3, V, 6], [1, 2, 4, V, 6]]) == 0      # not even the two ids they do have in common
    assert shared_prefix_len([[1, 2, 3, V, 6], [1, 2, V, 6]]) == 0         # the placeholder one row earlier
    assert shared_prefix_len([[1, 2, V, 6], [1, 2, 3, V, 6]]) == 0         # ... or later
    assert shared_prefix_len([[1, 2, V, 6], [1, 2, IMG, 6]]) == 0          # another placeholder is another id
    assert shared_prefix_len([[1, 2, V], [1, 2]]) == 0                     # a prompt that ends before it
    assert shared_prefix_len([[1, 2, V, 6]] * 5 + [[9, 2, V, 6]]) == 0     # one odd prompt among many


def test_empty_prefix_single_prompt_and_degenerate_batches():
    assert shared_prefix_len([[V, 4, 5], [V, 4, 5]]) == 0                  # the placeholder in front: nothing before it
    assert shared_prefix_len([[1, 2, 3, V, 4]]) == 3                       # B = 1: the rule holds; the engine asks for two prompts before it shares
    assert shared_prefix_len([]) == 0
    assert shared_prefix_len([[1, 2, 3], [1, 2, 3]]) == 0                  # no placeholder at all (trace_splice_embeds refuses such a prompt)
    assert shared_prefix_len([[], []]) == 0


def test_default_threshold_is_32():
    """the break-even of one extra prefix prefill and the copies against (B - 1) x P saved rows lies near 16 - 20 videos (prefix.py)"""
    from trace_amd.engine import TraceEngine
    assert SHARE_PREFIX_MIN_BATCH == 32
    assert TraceEngine.share_prefix_min_batch == 32


def test_new_entry_points_declared_and_exported_by_both_libraries():
    from trace_amd import _lib, build
    build.build()
    hdr = open(os.path.join(ROOT, "include", "trace_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert f"int {name}(" in hdr, name
        for element in ("bf16", "f16"):
            fn = getattr(_lib.load(element), name)
            assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.errcheck is not None
    assert len(_lib.SIGNATURES["trace_decode_set_shared_prefix"][1]) == 3
    assert len(_lib.SIGNATURES["trace_op_attn_decode_shared"][1]) == len(_lib.SIGNATURES["trace_op_attn_decode"][1]) + 3
    assert len(_lib.SIGNATURES["trace_llm_prefill_shared"][1]) == 8
    assert _lib.load().trace_abi_version() == 4                            # symbols were added; nothing that existed changed


def test_new_entry_points_reject_bad_arguments_without_a_device():
    """argument checks come before any HIP call: a NULL context or pointer is an error return, not a crash (safe without a GPU)"""
    from trace_amd import _lib, build
    build.build()
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        with pytest.raises(_lib.TraceHipError, match="trace_decode_set_shared_prefix: context not finalized"):
            lib.trace_decode_set_shared_prefix(None, 0, 64)
        with pytest.raises(_lib.TraceHipError, match="trace_llm_prefill_shared: context not finalized"):
            lib.trace_llm_prefill_shared(None, 0, 0, 1, 32, None, 4, None)
        with pytest.raises(_lib.TraceHipError, match="trace_op_attn_decode_shared: null argument"):
            lib.trace_op_attn_decode_shared(None, None, None, None, None, None, 3, 8, 2, 4, 128, 1, 1.0, 3, 32, None)


def test_integration_stub_names_the_new_entry_points():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in doc, name
