"""The entry paths of a decode batch — trace_decode_begin, trace_decode_admit(_ex), trace_decode_retire — seen through the batch's per-row columns
(trace_debug_decode_rows: slots, pos, heads, done, out_len, row_id, step0, out_ids, forced, logprobs, row_sp, row_lp, row_max, x).

Everything runs the identity-layer decoder of tests/token_select_probes.py on rigs built as tests/test_gpu_retire.py builds them (max_new = 41,
max_ctx = 192): its logits do not depend on rounding, so two ways of seating the same rows must leave the same bits in every column, the next
step's input embedding rows included, and every assertion is exact equality.  Every refusal here is a host-side argument check that returns
before anything is queued."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import test_gpu_retire as TR  # noqa: E402
import token_select_probes as P  # noqa: E402
from trace_amd import _lib  # noqa: E402
from trace_amd.engine import row_params_c  # noqa: E402
from trace_amd.sampling import LogitsParams, RowParams, SamplingParams  # noqa: E402

_rigs = {}
PER_ROW = ("row_sp", "row_lp", "row_max")


@pytest.fixture(scope="module")
def rigs(golden_dir):
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))

    def get(kind="bf16"):
        if kind not in _rigs:                             # "spare": twelve slots, of which the tests here never prefill the last
            _rigs[kind] = TR.Rig(E, 12) if kind == "spare" else TR.Rig(E, TR.KINDS[kind]["slots"])
        return _rigs[kind]
    yield get
    for r in _rigs.values():
        r.eng.close()
    _rigs.clear()


def put(rig, slot, start):
    """KV slot <- the prompt whose last row is the start token (kept where it is the same)"""
    if rig.start.get(slot) != start:
        rig.emb[-1] = P.embedding_row(rig.cfg, start).to(rig.emb.device)
        rig.eng.prefill(slot, rig.L, embeds=rig.emb)
        rig.start[slot] = start


def columns(eng):
    """name -> int32 [B, words a row] of every column of the running batch, None for a column the armed mode does not have"""
    out, cap = {}, eng._B * max(eng._max_new, eng.cfg.hidden_size // 2, 16)
    while (name := eng.lib.trace_debug_decode_column(eng.h, len(out))) is not None:
        buf = np.full(cap, -7, np.int32)
        w = eng.lib.trace_debug_decode_rows(eng.h, len(out), buf.ctypes.data_as(C.c_void_p), cap)
        assert w or (buf == -7).all(), f"{name}: reported absent, yet written"
        out[name.decode()] = buf[: eng._B * w].reshape(eng._B, w).copy() if w else None
    assert list(out) == ["slots", "pos", "heads", "done", "out_len", "row_id", "step0", "out_ids", "forced", "logprobs", "row_sp", "row_lp", "row_max", "x"]
    assert eng.lib.trace_debug_decode_column(eng.h, -1) is None
    return out


def same(a, b, tag):
    for name in a:
        assert (a[name] is None) == (b[name] is None), f"{tag}: {name} exists on one side only"
        if a[name] is not None:
            assert a[name].shape == b[name].shape and (a[name] == b[name]).all(), f"{tag}: column {name} differs in rows {sorted(set(np.nonzero(a[name] != b[name])[0]))}"


def begin(rig, rows, n, eos=-1, params=None):
    for b, (s, _, _) in enumerate(rows[:n]):
        put(rig, b, s)
    rig.eng.decode_begin(list(range(n)), [h for _, h, _ in rows[:n]], rig.max_new, eos, [f for _, _, f in rows[:n]],
                         row_params=None if params is None else params[:n])


def admit(rig, rows, k, n, params=None, row_ids=None):
    for b in range(k, n):
        put(rig, b, rows[b][0])
    heads, forced, rid = [h for _, h, _ in rows[k:n]], [f for _, _, f in rows[k:n]], list(range(k, n)) if row_ids is None else row_ids
    if params is None:
        rig.eng.admit_rows(list(range(k, n)), heads, rid, forced)
    else:
        rig.eng.admit_rows_ex(list(range(k, n)), heads, params[k:n], rid, forced)


def mixed_params(n, mn):
    """greedy rows with and without a bound of their own, sampled rows with seeds of their own (no processors: the rows are fed forced ids)"""
    return [RowParams(SamplingParams(0.7 + 0.1 * (r % 3), 40, 0.9, 1000 + r), None, None if r % 4 else 5 + r % 7) if r % 2
            else RowParams(None, None, mn - r % 5) for r in range(n)]


# ---------------------------------------------------------------------------------------------------------------- 1: admit = begin for the rows behind
def begin_against_begin_and_admit(rig, k, n, graph, params=None, tag=""):
    rows = P.batch_rows(rig.cfg, rig.plan, n, rig.max_new)
    eng = rig.eng
    begin(rig, rows, n, params=params)
    whole0 = columns(eng)
    eng.decode_steps(4, graph)
    whole4 = columns(eng)
    begin(rig, rows, k, params=params)
    admit(rig, rows, k, n, params)
    parts0 = columns(eng)
    same(whole0, parts0, f"{tag}{k} + {n - k} against {n}, before any step")
    assert not parts0["step0"].any() and parts0["row_id"][:, 0].tolist() == list(range(n)) and (parts0["out_len"] == 1).all()
    assert (parts0["pos"] == rig.L).all() and (parts0["x"] != 0).any(1).all()
    eng.decode_steps(4, graph)
    same(whole4, columns(eng), f"{tag}{k} + {n - k} against {n}, after 4 steps")
    return parts0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("k,n", [(1, 2), (5, 8), (33, 40)])
def test_admission_is_a_begin_for_the_rows_behind(rigs, k, n, graph):
    rig = rigs()
    assert rig.eng.decode_batch_max == 40
    got = begin_against_begin_and_admit(rig, k, n, graph)
    assert all(got[c] is None for c in PER_ROW + ("logprobs",))


def test_admission_is_a_begin_with_row_params(rigs):
    rig = rigs()
    got = begin_against_begin_and_admit(rig, 5, 8, True, mixed_params(8, rig.max_new), "per-row params: ")
    assert all(got[c] is not None for c in PER_ROW) and got["logprobs"] is None


def test_admission_is_a_begin_with_logprobs(rigs):
    rig = rigs()
    rig.eng.set_logprobs(True)
    try:
        got = begin_against_begin_and_admit(rig, 5, 8, True, tag="logprobs: ")
    finally:
        rig.eng.set_logprobs(False)
    assert got["logprobs"] is not None and got["logprobs"].shape == (8, rig.max_new) and all(got[c] is None for c in PER_ROW)


# ---------------------------------------------------------------------------------------------------------------- 2: an admission after steps
def params_words(arr):
    """the words the per-row columns hold for trace_row_params [n]: SampleParams (all zero for a greedy row), LogitsParams, max_new"""
    sp, lp, mx = [], [], []
    for r in arr:
        s = r.sampling
        f = [s.temperature, s.top_p, s.min_p, s.typical_p, s.epsilon_cutoff, s.eta_cutoff, np.sqrt(np.float32(s.eta_cutoff))]
        t, p, mp, ty, ep, et, sq = (int(x) for x in np.array(f, np.float32).view(np.int32))
        seed = np.array([s.seed], np.uint64).view(np.int32)
        sp.append([t, s.top_k, p, int(seed[0]), int(seed[1]), mp, ty, ep, et, sq] if s.temperature > 0 else [0] * 10)
        lp.append([int(np.array([r.repetition_penalty], np.float32).view(np.int32)[0]), r.no_repeat_ngram_size, r.min_new_tokens])
        mx.append([r.max_new])
    return {"row_sp": np.array(sp, np.int32), "row_lp": np.array(lp, np.int32), "row_max": np.array(mx, np.int32)}


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_admission_after_steps(rigs, graph):
    rig = rigs()
    eng, mn, L = rig.eng, rig.max_new, rig.L
    rows = P.batch_rows(rig.cfg, rig.plan, 8, mn)
    params = mixed_params(8, mn)
    params[5] = RowParams(None, None, 5)                 # a row that is stepped past its own bound below
    params[6] = RowParams(SamplingParams(0.8, 50, 0.95, 2 ** 40 + 17, min_p=0.05, eta_cutoff=0.25), None, 7)
    begin(rig, rows, 5, params=params)
    eng.decode_steps(3, graph)
    admit(rig, rows, 5, 8, params, row_ids=[17, 23, 5])
    col = columns(eng)
    assert col["step0"][:, 0].tolist() == [0] * 5 + [3] * 3 and col["row_id"][:, 0].tolist() == [0, 1, 2, 3, 4, 17, 23, 5]
    assert col["slots"][:, 0].tolist() == list(range(8)) and col["pos"][:, 0].tolist() == [L + 3] * 5 + [L] * 3
    assert col["out_len"][:, 0].tolist() == [4] * 5 + [1] * 3
    want = params_words(row_params_c(params, mn))
    for name in PER_ROW:
        assert (col[name] == want[name]).all(), name
    eng.decode_steps(6, graph)
    col = columns(eng)
    own = [min(9 if b < 5 else 6, (p.max_new_tokens or mn) - 1) for b, p in enumerate(params)]           # steps of its own, up to its own bound
    assert own[5] == 4 and col["pos"][:, 0].tolist() == [L + o for o in own]
    assert col["out_len"][:, 0].tolist() == [o + 1 for o in own]
    for name in PER_ROW:
        assert (col[name] == want[name]).all(), f"{name} after the steps"


# ---------------------------------------------------------------------------------------------------------------- 3: retire moves every column
@pytest.mark.parametrize("armed", ["plain", "per-row params + logprobs"])
@pytest.mark.parametrize("keep", [[0, 1, 2, 5, 6, 8], [1, 2, 5, 6, 7]], ids=["front stays", "first and last leave"])
def test_retire_moves_every_column(rigs, keep, armed):
    """nine rows, four steps, then a keep list that drops two adjacent rows (3, 4) and one more, or the first and the last row too"""
    rig = rigs()
    eng, mn = rig.eng, rig.max_new
    rows = P.batch_rows(rig.cfg, rig.plan, 9, mn)
    full = armed != "plain"
    eng.set_logprobs(full)
    try:
        begin(rig, rows, 9, params=mixed_params(9, mn) if full else None)
        eng.decode_steps(4, True)
        before = columns(eng)
        eng.retire_rows(keep)
        after = columns(eng)
    finally:
        eng.set_logprobs(False)
    for name in before:
        assert (before[name] is None) == (after[name] is None) == (not full and name in PER_ROW + ("logprobs",)), name
        if before[name] is not None:
            assert after[name].shape[0] == len(keep) and (after[name] == before[name][keep]).all(), f"column {name} after retire({keep})"
    assert (before["out_len"] == 5).all() and len({tuple(r) for r in before["x"].tolist()}) > 1       # rows worth telling apart
    eng.decode_steps(2, True)
    assert columns(eng)["pos"][:, 0].tolist() == [rig.L + 6] * len(keep)


def test_host_mirrors_follow_a_retire_and_an_admission(rigs):
    """What the host keeps per row (slots, origins, own bounds) moves with a retire: a freed slot is admitted, a kept one refused, and the bound of
    trace_decode_steps is that of the rows that stayed and of the rows that joined."""
    rig = rigs()
    eng, mn = rig.eng, rig.max_new
    rows = P.batch_rows(rig.cfg, rig.plan, 8, mn)
    begin(rig, rows, 8)
    eng.decode_steps(2)
    eng.retire_rows([1, 2, 5, 6, 7])
    was = columns(eng)
    with pytest.raises(_lib.TraceHipError, match="slot 5 is already in the running batch"):
        eng.admit_rows([3, 5], [0, 0])
    same(was, columns(eng), "after the refused admission of a kept slot")
    eng.admit_rows([3, 0], [rows[3][1], rows[0][1]], [8, 9])
    col = columns(eng)
    assert col["slots"][:, 0].tolist() == [1, 2, 5, 6, 7, 3, 0] and col["step0"][:, 0].tolist() == [0] * 5 + [2, 2]
    with pytest.raises(_lib.TraceHipError, match="slot 0 is already in the running batch"):
        eng.admit_rows([0], [0])
    eng.decode_steps(mn - 1)                               # the admitted rows' own steps; the kept rows are past their bound
    with pytest.raises(_lib.TraceHipError, match="for every row"):
        eng.decode_steps(1)
    assert columns(eng)["out_len"][:, 0].tolist() == [mn] * 7
    # per-row bounds: row 0 alone has room; once it has left, the rows that stay have 5 - 1 - 2 steps
    begin(rig, rows, 5, params=[RowParams(None, None, mn)] + [RowParams(None, None, 5)] * 4)
    eng.decode_steps(2)
    eng.retire_rows([1, 2, 3, 4])
    with pytest.raises(_lib.TraceHipError, match="for every row"):
        eng.decode_steps(3)
    eng.decode_steps(2)
    assert columns(eng)["out_len"][:, 0].tolist() == [5] * 4


# ---------------------------------------------------------------------------------------------------------------- 4: refusals
BEGIN, ADMIT = r"in trace_decode_begin: ", r"in trace_decode_admit: trace_decode_admit: "
FORCED_BEGIN = (r"logits processors / constraints \(trace_decode_set_logits_params, trace_decode_set_constraints\) with forced ids: the history is "
                r"the recorded ids, not the fed ones$")
FORCED_ADMIT = r"forced ids with logits processors / constraints armed: the history is the recorded ids, not the fed ones$"


def test_shared_refusals_keep_each_entry_points_text(rigs):
    rig = rigs("spare")
    eng, mn = rig.eng, rig.max_new
    rows = P.batch_rows(rig.cfg, rig.plan, 8, mn)
    for b in range(8):
        put(rig, b, rows[b][0])
    long = torch.cat([rig.emb] * (152 // rig.L + 1))[:152]                  # 152 + 41 > max_ctx = 192
    eng.prefill(10, 152, embeds=long)
    rig.start.pop(10, None)
    heads, forced = [h for _, h, _ in rows], [f for _, _, f in rows]
    cases = [([12], [0], "slot not prefilled$"), ([-1], [0], "slot not prefilled$"), ([11], [0], "slot not prefilled$"), ([5], [3], "head must be 0, 1 or 2$"),
             ([5, 6, 5], [0, 0, 0], "duplicate slot$"), ([10], [0], r"prefill \+ max_new_tokens exceeds max_ctx$")]
    for slots, hd, text in cases:
        with pytest.raises(_lib.TraceHipError, match=BEGIN + text):
            eng.decode_begin(slots, hd, mn, -1)
    begin(rig, rows, 5)
    eng.decode_steps(2)
    was = columns(eng)
    for slots, hd, text in cases:
        with pytest.raises(_lib.TraceHipError, match=ADMIT + text):
            eng.admit_rows(slots, hd)
        assert eng._B == 5
        same(was, columns(eng), f"after the refused admission of {slots}")
    # two things wrong at once: the shared checks come first, per row slot -> duplicate -> head -> max_ctx, then the entry point's own
    with pytest.raises(_lib.TraceHipError, match=ADMIT + "slot not prefilled$"):
        eng.admit_rows([12, 5], [0, 3], [-1, 6])
    with pytest.raises(_lib.TraceHipError, match=ADMIT + "head must be 0, 1 or 2$"):
        eng.admit_rows([5, 2], [3, 0], [-1, 6])
    with pytest.raises(_lib.TraceHipError, match=ADMIT + "duplicate slot$"):
        eng.admit_rows([5, 5], [0, 3], [5, 6])
    with pytest.raises(_lib.TraceHipError, match="slot 2 is already in the running batch"):
        eng.admit_rows([5, 2], [0, 0], [5, -1])
    same(was, columns(eng), "after the refused admissions with two faults")
    # forced ids while processors are armed
    eng.set_logits_params(LogitsParams(repetition_penalty=1.5))
    try:
        with pytest.raises(_lib.TraceHipError, match=BEGIN + FORCED_BEGIN):
            eng.decode_begin([0], heads[:1], mn, -1, forced[:1])
        eng.decode_begin([0], heads[:1], mn, -1)
        was = columns(eng)
        with pytest.raises(_lib.TraceHipError, match=ADMIT + FORCED_ADMIT):
            eng.admit_rows([1], heads[1:2], forced=forced[1:2])
        same(was, columns(eng), "after the refused admission with forced ids")
    finally:
        eng.set_logits_params(None)


def test_admits_own_refusals_leave_every_column(rigs):
    rig = rigs("spare")
    eng, mn = rig.eng, rig.max_new
    assert rig.L > 32
    rows = P.batch_rows(rig.cfg, rig.plan, 8, mn)
    for b in range(8):
        put(rig, b, rows[b][0])
    heads = [h for _, h, _ in rows]

    def refused(text, call):
        was, B = columns(eng), eng._B
        with pytest.raises(_lib.TraceHipError, match=text):
            call()
        assert eng._B == B
        same(was, columns(eng), text)

    begin(rig, rows, 5)
    eng.decode_steps(2)
    refused("slot 2 is already in the running batch", lambda: eng.admit_rows([5, 2], heads[5:7]))
    refused("row_ids must not be negative", lambda: eng.admit_rows([5, 6], heads[5:7], [5, -1]))
    refused("begun without per-row params", lambda: eng.admit_rows_ex([5], heads[5:6], [RowParams()]))
    begin(rig, rows, 5, params=mixed_params(5, mn))
    eng.decode_steps(2)
    refused("begun with per-row params", lambda: eng.admit_rows([5], heads[5:6]))
    two = row_params_c([RowParams(), RowParams()], mn)
    two[1].size += 8
    i32 = lambda x: (C.c_int32 * len(x))(*x)             # noqa: E731
    refused("every trace_row_params must carry the same size",
            lambda: eng.lib.trace_decode_admit_ex(eng.h, i32([5, 6]), 2, i32(heads[5:7]), i32([5, 6]), None, two, None))
    # the prompts differ in their last row only: the first 32 rows of every slot are slot 0's
    eng.decode_begin(list(range(4)), heads[:4], mn, -1, [f for _, _, f in rows[:4]], shared_prefix=(0, 32))
    eng.decode_steps(2)
    refused("the running batch attends a shared prefix", lambda: eng.admit_rows([5], heads[5:6]))
    eng.host_mode(True)
    try:
        eng.decode_begin([0], heads[:1], mn, -1, want_logits=True)
        refused("not available in host-select mode", lambda: eng.admit_rows([1], heads[1:2]))
    finally:
        eng.host_mode(False)
