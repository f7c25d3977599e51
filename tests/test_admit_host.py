"""Continuous batching, host side: the admit rule, the loop and the book of TraceEngine.generate_queue without an engine
(trace_amd/decode_loop.py under QUEUE's rules on the scripted device of tests/decode_loop_probes.py), the per-row step rule restated over a shared counter (tests/admit_probes.py) with its
near misses, and the interface (header, signatures).  No device."""
import inspect
import os
import re

import numpy as np
import pytest

import admit_probes as AP
import constraint_probes as CP
import token_select_probes as P
from decode_loop_probes import expected, run as run_scripted, script_with_ends
from trace_amd.admit import ADMIT_FRACTION, admit_plan
from trace_amd.decode_loop import QUEUE, RowBook
from trace_amd.retire import RETIRE_FRACTION

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_admit_plan_edges():
    assert ADMIT_FRACTION == RETIRE_FRACTION == 8
    assert admit_plan(100, 128, 0, 28) == 0, "nothing waiting"
    assert admit_plan(100, 128, 50, 0) == 0, "no free slot"
    assert admit_plan(128, 128, 50, 40) == 0 and admit_plan(130, 128, 50, 40) == 0, "cap reached"
    assert admit_plan(113, 128, 50, 15) == 0, "room 15 below 128 // 8"
    assert admit_plan(112, 128, 50, 16) == 16 and admit_plan(112, 128, 5, 16) == 5, "room at the threshold: whatever waits, up to the room"
    assert admit_plan(100, 128, 50, 10) == 0, "the free slots bound the room"
    assert admit_plan(0, 128, 50, 3) == 3 and admit_plan(0, 128, 2, 128) == 2, "empty batch: whatever fits"
    assert admit_plan(3, 4, 9, 1) == 1 and admit_plan(7, 8, 9, 1) == 1 and admit_plan(15, 16, 9, 1) == 0, "small caps admit single rows"
    assert admit_plan(96, 128, 50, 32, fraction=2) == 0 and admit_plan(64, 128, 50, 64, fraction=2) == 50


@pytest.mark.parametrize("cap", [1, 2, 7, 8, 9, 16, 40, 64, 128, 256])
def test_admit_plan_table(cap):
    need = max(1, cap // ADMIT_FRACTION)
    for B in range(cap + 1):
        got = admit_plan(B, cap, 1000, cap - B)
        assert got == (cap - B if (B == 0 or cap - B >= need) and cap > B else 0), (cap, B)
        assert admit_plan(B, cap, 1, cap - B) == min(got, 1)


# ---------------------------------------------------------------------------------------------------------------- the bookkeeping model
def run_queue(script, max_new, chunk, cap, logprobs=True):
    """the loop of TraceEngine.generate_queue on the scripted device: decode_loop under QUEUE's rules"""
    book, dev = run_scripted(script, max_new, chunk, cap, QUEUE, logprobs)
    return book.results(), book, dev


def test_request_order_through_interleaved_retires_and_admits():
    """cap 4, chunk 4, max_new 13.  Request 0 ends with its token 0 and leaves before a step is run; request 4 takes its KV slot 0.  Request 2 ends in
    the first chunk, request 5 takes its slot 2 and ends at its own step 1, inside the chunk it was admitted in, as request 4 (its own step 6) does in
    its second.  Requests 6 and 7 take slots 0 and 2; request 6 never ends and is the last row of the batch."""
    max_new, chunk, cap = 13, 4, 4
    ends = [0, None, 3, 9, 6, 1, None, 2]
    script = script_with_ends(ends, max_new)
    out, book, dev = run_queue(script, max_new, chunk, cap)
    assert [o[0] for o in out] == expected(script)
    assert [o[1] for o in out] == [100 + r for r in range(len(ends))]
    for r, (x, _, lp) in enumerate(out):
        assert lp.dtype == np.float32 and len(lp) == len(x) and lp[0] == np.float32(-(r + 1))
    assert book.history == [[0, 1, 2, 3],                # begin: slots 0 .. 3
                            [1, 2, 3], [1, 2, 3, 4],     # 0 ended with its token 0; 4 into slot 0                    -> 4 steps of 4 rows
                            [1, 3, 4], [1, 3, 4, 5],     # 2 ended (its id 3 is EOS); 5 into slot 2                   -> 4 steps of 4 rows
                            [1, 3], [1, 3, 6, 7],        # 4 (own step 6) and 5 (own step 1) ended; 6, 7 into 0, 2    -> 4 steps of 4 rows
                            [6]]                         # 1 has max_new ids, 3 and 7 ended                           -> 8 steps of 1 row
    assert dev.prefilled == {0: 6, 1: 1, 2: 7, 3: 3} and book.retires == 4 and book.admits == 3
    assert book.free == [0, 1, 2, 3] and book.rows == [] and dev.row_steps == 3 * 4 * 4 + 8
    fixed = sum(chunk * -(-(max(len(x) for x in expected(script)[i:i + cap]) - 1) // chunk) * cap for i in range(0, len(ends), cap))
    assert dev.row_steps < fixed                          # fewer rows x steps than two fixed batches of 4, even without their retires


def test_batch_that_ends_at_once_begins_the_next():
    max_new = 9
    script = script_with_ends([1, 2, 1, 3, None, 1], max_new)
    out, book, dev = run_queue(script, max_new, 4, 4, logprobs=False)
    assert [o[0] for o in out] == expected(script) and all(len(o) == 2 for o in out)
    assert book.history == [[0, 1, 2, 3], [4, 5], [4]] and book.admits == 0 and book.retires == 1
    assert dev.row_steps == 4 * 4 + 4 * 2 + 4 * 1


def test_a_row_that_ends_with_its_first_token_rides_no_chunk():
    max_new = 9
    script = script_with_ends([1, 2, 0, 3, None, 1], max_new)
    out, book, dev = run_queue(script, max_new, 4, 4, logprobs=False)
    assert [o[0] for o in out] == expected(script)
    assert book.history == [[0, 1, 2, 3], [0, 1, 3], [0, 1, 3, 4], [4], [4, 5]] and dev.row_steps == 4 * 4 + 4 * 2


def test_nothing_ever_finishes_early():
    max_new = 9
    script = script_with_ends([None] * 5, max_new)
    out, book, dev = run_queue(script, max_new, 4, 2, logprobs=False)
    assert [o[0] for o in out] == expected(script)
    assert book.history == [[0, 1], [2, 3], [4]] and dev.row_steps == (max_new - 1) * 5


def test_queue_book_errors():
    for bad in ([], [1, 1], [-1, 2]):
        with pytest.raises(ValueError):
            RowBook(bad)
    book = RowBook([3, 1, 2])
    with pytest.raises(ValueError):
        book.admit(0)
    with pytest.raises(ValueError):
        book.admit(4)
    assert book.admit(2) == [1, 2] and book.rows == [0, 1] and book.free == [3]
    ids, hd = [[5], [6]], [0, 1]
    for keep in ([], [1, 0], [0, 0], [2], [-1]):
        with pytest.raises(ValueError):
            book.retire(keep, ids, hd)
    with pytest.raises(ValueError):
        book.retire([0], ids[:1], hd)
    with pytest.raises(ValueError):
        book.keep_list([True])
    with pytest.raises(ValueError):
        book.results()                                    # rows are still live
    with pytest.raises(ValueError):
        RowBook([0], logprobs=True).finish([], [], None)
    assert book.rows == [0, 1] and book.retires == 0
    book.retire([1], ids, hd)
    assert book.rows == [1] and book.slots == [2] and book.free == [1, 3]
    assert book.admit(2) == [1, 3] and book.rows == [1, 2, 3] and book.admits == 1
    book.finish([[6, 9], [7], [8]], [1, 2, 0])
    assert book.results() == [([5], 0), ([6, 9], 1), ([7], 2), ([8], 0)] and book.free == [1, 2, 3]


# ---------------------------------------------------------------------------------------------------------------- the per-row step rule
@pytest.fixture(scope="module")
def tables():
    cfg = P.small()
    T, plan = P.build_table(cfg)
    CT, cplan = CP.build_table(cfg)
    return cfg, T, plan, P.max_new_for(cfg, plan), CT, cplan, P.logit_scale(cfg)


def scenarios(tables):
    cfg, T, plan, mn, CT, cplan, scale = tables
    out = [dict(name="plain", table=T, max_new=mn, **AP.plain_scenario(cfg, plan, mn)),
           dict(name="sampled", table=T, max_new=mn, **AP.sampled_scenario(cfg, plan, mn))]
    out += [dict(table=CT, max_new=CP.MAX_NEW, **s) for s in AP.processor_scenarios(cfg, cplan)]
    return out


def run(tables, sc, shared=()):
    cfg, scale = tables[0], tables[6]
    return AP.restate_origins(sc["table"], cfg, sc["rows"], AP.ORIGINS, sc["eos"], sc["max_new"], scale, sc.get("params"), sc.get("cons"),
                              sc.get("sampling"), sc.get("row_ids"), shared)


def rows_alone(tables, sc):
    cfg, scale = tables[0], tables[6]
    ids = sc.get("row_ids") or range(len(sc["rows"]))
    out = [AP.alone(sc["table"], cfg, row, sc["eos"], sc["max_new"], scale, sc.get("params"), sc.get("cons"), sc.get("sampling"), r)
           for row, r in zip(sc["rows"], ids)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def test_every_row_gets_what_it_gets_alone(tables):
    """origins [0, 0, 5, 9]: whichever counter value a row joined at, its ids, length and head are those of the row decoded alone — and `alone` is
    the projects' own restatements: P.restate_batch for the greedy rows, CP.restate for the rows under processors and constraints"""
    cfg, T, plan, mn, CT, cplan, scale = tables
    for sc in scenarios(tables):
        want = rows_alone(tables, sc)
        assert run(tables, sc) == want, sc["name"]
        if sc["name"] == "plain":
            assert want == tuple(P.restate_batch(T, cfg, sc["rows"], sc["eos"], mn)) and want[1][0] == 2 and want[1][3] == 7 and want[1][1] == mn
        elif sc["name"] != "sampled":
            for b, (t, h, _) in enumerate(sc["rows"]):
                o = CP.restate(CT, cfg, t, h, sc["params"], sc["cons"], sc["eos"], CP.MAX_NEW, scale)
                assert (want[0][b], want[1][b], want[2][b]) == (list(o[0]), o[1], o[2]), (sc["name"], b)


@pytest.mark.parametrize("use", AP.USES)
def test_a_shared_step_in_any_one_use_is_told(tables, use):
    """the restatement that takes the shared counter for one use gives an admitted row something else in every scenario that names the use, and
    leaves the rows that began at counter 0 alone"""
    named = [sc for sc in scenarios(tables) if use in sc["tells"]]
    assert named, f"no scenario names {use}"
    for sc in named:
        want, got = rows_alone(tables, sc), run(tables, sc, shared=(use,))
        differ = [b for b in range(4) if (got[0][b], got[1][b]) != (want[0][b], want[1][b])]
        assert differ and set(differ) <= {2, 3}, (use, sc["name"], differ)


def test_scenarios_cover_every_use(tables):
    assert {u for sc in scenarios(tables) for u in sc["tells"]} == set(AP.USES)


# ---------------------------------------------------------------------------------------------------------------- the interface
def test_header_declares_trace_decode_admit():
    hdr = open(os.path.join(ROOT, "include", "trace_hip.h")).read()
    assert re.search(r"int\s+trace_decode_admit\s*\(\s*trace_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*slots\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*heads\s*,"
                     r"\s*const\s+int32_t\s*\*\s*row_ids\s*,\s*const\s+int32_t\s*\*\s*forced\s*,\s*void\s*\*\s*stream\s*\)\s*;", hdr)
    from trace_amd._lib import SIGNATURES
    assert "trace_decode_admit" in SIGNATURES and len(SIGNATURES["trace_decode_admit"][1]) == 7


def test_engine_and_model_entry_points():
    from trace_amd import evaluate
    from trace_amd.engine import TraceEngine
    p = inspect.signature(TraceEngine.generate_queue).parameters
    assert list(p)[:4] == ["self", "requests", "max_new_tokens", "eos"] and p["eos"].default == -1
    for name, default in (("max_rows", None), ("sampling", None), ("logprobs", False), ("logits", None), ("constraints", None), ("use_graph", True)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default, name
    p = inspect.signature(TraceEngine.admit_rows).parameters
    assert list(p) == ["self", "slots", "heads", "row_ids", "forced"] and p["row_ids"].default is None and p["forced"].default is None
    assert TraceEngine.admit_fraction == ADMIT_FRACTION
    assert inspect.signature(evaluate.evaluate_videos).parameters["continuous"].default is False
