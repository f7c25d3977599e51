"""Retiring finished rows from a running decode batch, host side: the retire rule, the loop and the book of TraceEngine.decode(retire_finished=True)
without an engine (trace_amd/decode_loop.py under DECODE's rules on the scripted device of tests/decode_loop_probes.py), and the interface (header,
signatures).  No device."""
import inspect
import os
import re

import numpy as np
import pytest

from decode_loop_probes import expected, run, script_with_ends
from trace_amd.decode_loop import DECODE, RowBook
from trace_amd.retire import RETIRE_FRACTION, retire_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("B", [1, 2, 3, 7, 8, 9, 15, 16, 17, 33, 40, 64, 100, 128, 256])
def test_retire_plan_table(B):
    assert not retire_plan(B, B), "nothing finished: never"
    assert retire_plan(B, 0), "nothing left: always allowed"
    flags = [retire_plan(B, live) for live in range(B, -1, -1)]            # by the number finished, 0 .. B
    assert flags == sorted(flags), "monotone in the number finished"
    need = max(1, B // RETIRE_FRACTION)                                  # the starting rule of the issue, with the constant the module states
    assert flags.index(True) == need
    assert [retire_plan(B, B - k) for k in range(B + 1)] == [k >= need for k in range(B + 1)]


def test_retire_plan_small_batches_retire_single_rows():
    assert all(retire_plan(B, B - 1) for B in range(1, 2 * RETIRE_FRACTION))
    assert not retire_plan(2 * RETIRE_FRACTION, 2 * RETIRE_FRACTION - 1) and retire_plan(2 * RETIRE_FRACTION, 2 * RETIRE_FRACTION - 2)


# ---------------------------------------------------------------------------------------------------------------- the bookkeeping model
def decode_retiring(script, max_new, chunk, logprobs=True):
    """the loop of TraceEngine.decode(retire_finished=True) on the scripted device: decode_loop under DECODE's rules, the batch begun at once"""
    book, dev = run(script, max_new, chunk, len(script), DECODE, logprobs)
    return book.columns(), book, dev


def test_rows_finish_in_different_chunks_and_come_back_in_order():
    max_new, chunk = 21, 4
    ends = [0, 17, 3, None, 9, 5, 20, 1, 13]          # chunk boundaries after steps 4, 8, 12, 16, 20 (ids recorded: 5, 9, 13, 17, 21)
    script = script_with_ends(ends, max_new)
    (ids, heads, lps), book, dev = decode_retiring(script, max_new, chunk)
    assert ids == expected(script)
    assert heads == [100 + r for r in range(len(ends))]
    for r, (x, lp) in enumerate(zip(ids, lps)):
        assert lp.dtype == np.float32 and len(lp) == len(x) and lp[0] == np.float32(-(r + 1))
    assert book.history == [[0, 1, 2, 3, 4, 5, 6, 7, 8],
                            [1, 3, 4, 5, 6, 8],       # after 5 ids: rows 0, 2, 7 ended (3 of 9 >= max(1, 9 // 8))
                            [1, 3, 4, 6, 8],          # after 9 ids: row 5
                            [1, 3, 6, 8],             # after 13 ids: row 4 (ends at 9: its EOS is id 10)
                            [1, 3, 6]]                # after 17 ids: row 8; row 1 (EOS is id 18) ends inside the last chunk: no retire after the last step
    assert book.retires == 4 and book.history[-1] == [1, 3, 6]
    assert dev.row_steps == 4 * (9 + 6 + 5 + 4 + 3) < 9 * (max_new - 1)


def test_every_row_finishes_in_the_first_chunk():
    max_new = 21
    script = script_with_ends([0, 1, 2, 3, 4], max_new)
    (ids, heads), book, dev = decode_retiring(script, max_new, 8, logprobs=False)
    assert ids == expected(script) and heads == [100, 101, 102, 103, 104]
    assert book.history == [[0, 1, 2, 3, 4]] and book.retires == 0 and dev.row_steps == 8 * 5


def test_no_row_ever_finishes():
    max_new = 21
    script = script_with_ends([None] * 6, max_new)
    (ids, heads, lps), book, dev = decode_retiring(script, max_new, 4)
    assert ids == expected(script) and all(len(x) == max_new for x in ids)
    assert book.history == [[0, 1, 2, 3, 4, 5]] and dev.row_steps == 6 * (max_new - 1)


def test_threshold_holds_rows_back_until_enough_have_finished():
    """B = 32: one finished row is below 32 // 8, so it rides on until three more have finished"""
    max_new, chunk = 41, 4
    ends = [None] * 32
    ends[5], ends[9], ends[20], ends[21], ends[30] = 1, 6, 10, 11, 30
    script = script_with_ends(ends, max_new)
    (ids, heads), book, _ = decode_retiring(script, max_new, chunk, logprobs=False)
    assert ids == expected(script)
    live = [r for r in range(32) if r not in (5, 9, 20, 21)]
    # one retire of four rows at the boundary after rows 20 and 21 ended; row 30 ends later, alone: one of 28 is below 28 // 8 and it stays
    assert book.history == [list(range(32)), live] and book.retires == 1 and 30 in book.history[-1]


def test_retire_book_rejects_bad_keep_lists():
    book = RowBook(range(4))
    book.admit(4)
    ids, hd = [[1], [2], [3], [4]], [0, 0, 0, 0]
    for keep in ([], [2, 1], [1, 1], [0, 4], [-1, 2]):
        with pytest.raises(ValueError):
            book.retire(keep, ids, hd)
    with pytest.raises(ValueError):
        book.retire([0], ids[:3], hd)
    with pytest.raises(ValueError):
        book.keep_list([True, False])
    assert book.rows == [0, 1, 2, 3] and book.retires == 0
    book.retire([1, 3], ids, hd)
    assert book.rows == [1, 3]
    book.finish([[2, 9], [4, 9]], [1, 2])
    assert book.columns() == ([[1], [2, 9], [3], [4, 9]], [0, 1, 0, 2])


# ---------------------------------------------------------------------------------------------------------------- the interface
def test_header_declares_trace_decode_retire():
    hdr = open(os.path.join(ROOT, "include", "trace_hip.h")).read()
    assert re.search(r"int\s+trace_decode_retire\s*\(\s*trace_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*keep\s*,\s*int\s+n_keep\s*,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    from trace_amd._lib import SIGNATURES
    assert "trace_decode_retire" in SIGNATURES and len(SIGNATURES["trace_decode_retire"][1]) == 4


def test_engine_entry_points_take_retire_finished():
    from trace_amd.engine import TraceEngine
    for name in ("decode", "generate", "generate_samples", "generate_questions", "generate_stream", "decode_stepwise"):
        p = inspect.signature(getattr(TraceEngine, name)).parameters
        assert "retire_finished" in p and p["retire_finished"].default is False, name
    assert TraceEngine.retire_chunk == 32 and callable(TraceEngine.retire_rows)


def test_model_entry_points_take_retire_finished():
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM as M
    for name in ("generate", "generate_samples"):
        p = inspect.signature(getattr(M, name)).parameters
        assert "retire_finished" in p and p["retire_finished"].default is False, name
