"""Prompt-prefix reuse, the parts that need no device: where a prompt is cut and how suffixes are grouped (trace_amd/prefix.py), the three
new C-ABI names in both libraries, and the model's switch."""
import pytest

from trace_amd.prefix import APPEND_GROUP_MAX, group_by_length, split_prompt, split_questions

V, IMG, TIME, SYNC = -201, -200, -203, -205


def test_split_prompt_cuts_after_the_video_placeholder():
    assert split_prompt([1, 5, V, 7, 8]) == ([1, 5, V], [7, 8])
    assert split_prompt([V, 7]) == ([V], [7])
    assert split_prompt([1, IMG, 9]) == ([1, IMG], [9])                    # the image placeholder expands to the encoded rows as well
    assert split_prompt([1, V, SYNC, TIME, 4]) == ([1, V], [SYNC, TIME, 4])   # other modal placeholders are ordinary suffix rows
    assert split_prompt((1, 2, V)) == ([1, 2, V], [])                      # empty suffix: the caller takes the unsplit path
    import numpy as np
    p, s = split_prompt(np.array([3, V, 4], dtype=np.int64))
    assert p == [3, V] and s == [4] and all(type(x) is int for x in p + s)


def test_split_prompt_needs_exactly_one_placeholder():
    with pytest.raises(ValueError, match="found 0"):
        split_prompt([1, 2, 3])
    with pytest.raises(ValueError, match="found 2"):
        split_prompt([1, V, 3, V, 4])
    with pytest.raises(ValueError, match="found 2"):
        split_prompt([1, V, IMG])
    with pytest.raises(ValueError):
        split_prompt([])


def test_split_questions_common_prefix():
    prefix, suf = split_questions([[1, 2, V, 5, 6], [1, 2, V, 7], [1, 2, V, 5, 6]])
    assert prefix == [1, 2, V] and suf == [[5, 6], [7], [5, 6]]
    assert split_questions([[1, V]]) == ([1, V], [[]])
    with pytest.raises(ValueError, match="prompt 1 differs"):
        split_questions([[1, 2, V, 5], [1, 3, V, 5]])                      # disagree inside the prefix
    with pytest.raises(ValueError, match="prompt 1 differs"):
        split_questions([[1, 2, V, 5], [1, 2, 4, V, 5]])                   # placeholder at another position
    with pytest.raises(ValueError, match="prompt 2 differs"):
        split_questions([[1, V, 5], [1, V, 6], [1, IMG, 5]])               # another placeholder kind is another prefix
    with pytest.raises(ValueError, match="found 0"):
        split_questions([[1, V, 5], [1, 2, 5]])
    with pytest.raises(ValueError):
        split_questions([])


def test_group_by_length():
    assert group_by_length([3, 5, 3, 3, 5, 1]) == [(3, [0, 2, 3]), (5, [1, 4]), (1, [5])]
    assert group_by_length([]) == []
    g = group_by_length([4] * 19)
    assert APPEND_GROUP_MAX == 8 and g == [(4, list(range(8))), (4, list(range(8, 16))), (4, [16, 17, 18])]
    assert group_by_length([2, 2, 2], max_group=2) == [(2, [0, 1]), (2, [2])]
    flat = sorted(i for _, idx in group_by_length([7, 1, 7, 2, 1, 7, 7, 7, 7, 7, 7, 7]) for i in idx)
    assert flat == list(range(12))                                         # every prompt lands in exactly one group
    with pytest.raises(ValueError):
        group_by_length([1], max_group=0)


NEW_SYMBOLS = ("trace_llm_prefill_append", "trace_kv_copy", "trace_embed_rows")


def test_new_entry_points_declared_and_exported_by_both_libraries():
    import os
    from trace_amd import _lib, build
    build.build()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trace_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert f"int {name}(" in hdr, name
        for element in ("bf16", "f16"):
            fn = getattr(_lib.load(element), name)
            assert fn.argtypes == _lib.SIGNATURES[name][1] and fn.errcheck is not None
    assert len(_lib.SIGNATURES["trace_llm_prefill_append"][1]) == 8 and len(_lib.SIGNATURES["trace_kv_copy"][1]) == 6
    assert len(_lib.SIGNATURES["trace_embed_rows"][1]) == 9
    assert _lib.load().trace_abi_version() == 4                            # symbols were added; nothing that existed changed


def test_new_entry_points_reject_a_null_context_without_a_device():
    """argument checks come before any HIP call: a NULL context is an error return, not a crash (safe without a GPU)"""
    from trace_amd import _lib, build
    build.build()
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        with pytest.raises(_lib.TraceHipError, match="trace_llm_prefill_append: context not finalized"):
            lib.trace_llm_prefill_append(None, 0, 1, 0, None, 4, None, None)
        with pytest.raises(_lib.TraceHipError, match="trace_kv_copy: context not finalized"):
            lib.trace_kv_copy(None, 0, None, 1, 1, None)
        with pytest.raises(_lib.TraceHipError, match="trace_embed_rows: context not finalized"):
            lib.trace_embed_rows(None, None, 0, None, 0, None, 0, None, None)


def test_integration_stub_names_the_new_entry_points():
    import os
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in doc, name


class _FakeEngine:
    """what TraceMistralForCausalLM.__init__ and enable_prefix_cache touch"""
    device, dtype = "cpu", None

    def __init__(self):
        self.dropped = 0

    def _drop_prefix(self):
        self.dropped += 1


def test_enable_prefix_cache_exists_and_defaults_to_off():
    from trace_amd import config as tcfg
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    eng = _FakeEngine()
    m = TraceMistralForCausalLM(tcfg.tiny(), eng)
    assert m.prefix_cache_enabled is False
    assert m.enable_prefix_cache() is m and m.prefix_cache_enabled is True
    m.enable_prefix_cache(False)
    assert m.prefix_cache_enabled is False and eng.dropped == 2           # switching either way forgets the entry (and its tensor reference)


def test_engine_has_the_prefix_reuse_surface():
    from trace_amd.engine import TraceEngine
    for name in ("prefill_append", "kv_copy", "embed_rows", "generate_questions", "set_prefix_entry", "prefix_entry"):
        assert callable(getattr(TraceEngine, name)), name
