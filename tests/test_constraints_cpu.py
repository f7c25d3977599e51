"""Constraints of the decode step, on the CPU: the numpy restatement (sampling.constrain_row_ref / stop_match_ref) against transformers' own
processors and a plain list-slice statement, the probe table and case list of tests/constraint_probes.py against the mutants, argument validation,
and what model.generate() makes of its arguments (precedence, the EOS list, the [eos] filter on bad words).  Nothing here needs a GPU."""
import dataclasses
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import constraint_probes as CP
import token_select_probes as P
from trace_amd.sampling import (MAX_SEQ_LEN, MAX_SEQS, MAX_SUPPRESS, Constraints, LogitsParams, check_constraints, constrain_row_ref, ends_stopped,
                                process_row_ref, stop_match_ref)

GEOMS = list(CP.GEOMETRIES)


@pytest.fixture(scope="module")
def tables():
    out = {}
    for g in GEOMS:
        cfg = CP.GEOMETRIES[g]()
        T, plan = CP.build_table(cfg)
        out[g] = (cfg, T, plan, CP.decode_cases(cfg, plan))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1: the restatement
@pytest.mark.parametrize("geom", GEOMS)
def test_restatement_equals_the_probe_statement(geom):
    """constrain_row_ref is the rule-by-rule statement of constraint_probes (mutant None), bit for bit, on every loose row; only -inf is stored"""
    cfg = CP.GEOMETRIES[geom]()
    n_banned = 0
    for c in CP.row_cases(cfg):
        lo, hi = P.head_range(cfg, c.head)
        a = constrain_row_ref(c.row, c.hist, lo, hi, c.cons, c.step, c.min_new)
        b = CP.constrain_row(c.row, c.hist, lo, hi, c.cons, c.step, c.min_new)
        assert a.tobytes() == b.tobytes()
        changed = a != c.row
        assert (a[changed] == -np.inf).all() and (a[:lo] == -np.inf).all() and (a[hi:] == -np.inf).all()
        n_banned += int(changed.sum())
    assert n_banned > 100


@pytest.mark.parametrize("geom", GEOMS)
def test_restatement_equals_hf_processors(geom):
    """NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor and SuppressTokensAtBeginLogitsProcessor (begin_index 0: what HF computes when it is
    handed inputs_embeds) of the installed transformers on the whole row with the history as input_ids: the head's range must agree.  HF sees the
    device step as the history's length, so the step here is len(hist).  One known difference, asserted below: HF skips a bad word that is longer
    than the context (len(w) > len(h)), so with a generated-only context a bad word of k ids may come out as a row's first k ids; the rule here
    (include/trace_hip.h, rule 4) needs the k - 1 ids of the prefix only.  Words whose prefix is the whole history are therefore left out of
    the comparison and checked on their own."""
    lp = pytest.importorskip("transformers.generation.logits_process")
    cfg = CP.GEOMETRIES[geom]()
    cases = CP.row_cases(cfg) + [CP.RowCase(tr[2], tr[1], ids[:s], case.cons, s, 0)
                                 for case, ids, trace in _probe_traces(cfg) for s, tr in enumerate(trace) if s < 8]
    compared = boundary = 0
    for c in cases:
        lo, hi = P.head_range(cfg, c.head)
        L = len(c.hist)
        at_edge = [w for w in c.cons.bad_words_ids if len(w) > 1 and len(w) - 1 == L and list(w[:-1]) == c.hist]
        bad = [list(w) for w in c.cons.bad_words_ids if w not in at_edge]
        cons = dataclasses.replace(c.cons, bad_words_ids=bad)
        ours = constrain_row_ref(c.row, c.hist, lo, hi, cons, L, 0)
        x = torch.from_numpy(c.row.copy()).unsqueeze(0)
        ids = torch.tensor([c.hist], dtype=torch.long).view(1, L)
        if bad:
            x = lp.NoBadWordsLogitsProcessor(bad, eos_token_id=None)(ids, x)
        if cons.suppress_tokens:
            x = lp.SuppressTokensLogitsProcessor(list(cons.suppress_tokens), device="cpu")(ids, x)
        if cons.begin_suppress_tokens:
            x = lp.SuppressTokensAtBeginLogitsProcessor(list(cons.begin_suppress_tokens), 0, device="cpu")(ids, x)
        assert torch.equal(x[0, lo:hi], torch.from_numpy(ours[lo:hi])), (geom, c.head, L, c.step)
        compared += 1
        for w in at_edge:                        # the difference: the rule here bans, HF lets the word through
            full = constrain_row_ref(c.row, c.hist, lo, hi, Constraints(bad_words_ids=[w]), L, 0)
            hf = lp.NoBadWordsLogitsProcessor([list(w)], eos_token_id=None)(ids, torch.from_numpy(c.row.copy()).unsqueeze(0))[0]
            if lo <= w[-1] < hi and np.isfinite(c.row[w[-1]]):
                assert full[w[-1]] == -np.inf and hf[w[-1]] == c.row[w[-1]]
                boundary += 1
    assert compared == len(cases) and boundary > 0


def _probe_traces(cfg):
    """(case, ids, per-step (state, head, raw row, tok)) of the first row of every probe case without logits params: the probe histories"""
    T, plan = CP.build_table(cfg)
    scale = P.logit_scale(cfg)
    for case in CP.decode_cases(cfg, plan):
        if case.params is None:
            t, h = case.rows[0]
            trace = []
            ids, _, _ = CP.restate(T, cfg, t, h, None, case.cons, case.eos, CP.MAX_NEW, scale, trace=trace)
            yield case, ids, [(state, head, raw, tok) for state, head, raw, _, tok in trace]          # the RAW masked row of every step


@pytest.mark.parametrize("geom", GEOMS)
def test_stop_match_is_the_list_slice_statement(geom):
    cfg = CP.GEOMETRIES[geom]()
    fired = 0
    for hists, cons in CP.history_cases(cfg):
        for h in hists:
            want = any(len(h) >= len(w) and h[len(h) - len(w):] == list(w) for w in cons.stop_sequences)
            assert stop_match_ref(h, cons) == want == bool(CP.stop_match(h, cons))
            assert ends_stopped(h, -1, cons) == want
            fired += want
    assert fired >= 12
    assert ends_stopped([3, 7], 7) and not ends_stopped([7, 3], 7) and not ends_stopped([], 7) and not ends_stopped([7], -1)
    assert ends_stopped([1, 2, 3], 9, Constraints(stop_sequences=[[2, 3]])) and not ends_stopped([2, 3, 1], 9, Constraints(stop_sequences=[[2, 3]]))


# ---------------------------------------------------------------------------------------------------------------- 2: the cases and the mutants
@pytest.mark.parametrize("geom", GEOMS)
def test_every_case_constrains_something(tables, geom):
    """a case whose ids equal the unconstrained loop's is a test bug; a stop case must end a row before MAX_NEW"""
    cfg, T, plan, cases = tables[geom]
    scale = P.logit_scale(cfg)
    for c in cases:
        got = CP.restate_batch(T, cfg, c.rows, c.params, c.cons, c.eos, CP.MAX_NEW, scale)
        plain = CP.restate_batch(T, cfg, c.rows, None, Constraints(), c.eos, CP.MAX_NEW, scale)
        assert got[0] != plain[0], c.name
        if c.stops:
            assert min(got[1]) < CP.MAX_NEW, c.name
            assert got[1] != plain[1], c.name


@pytest.mark.parametrize("geom", GEOMS)
def test_every_mutant_is_rejected_by_a_named_case(tables, geom):
    cfg, T, plan, cases = tables[geom]
    scale = P.logit_scale(cfg)
    named = {m for c in cases for m in c.rejects}
    assert named == set(CP.MUTANTS), set(CP.MUTANTS) ^ named
    for c in cases:
        want = CP.restate_batch(T, cfg, c.rows, c.params, c.cons, c.eos, CP.MAX_NEW, scale)
        for m in c.rejects:
            got = CP.restate_batch(T, cfg, c.rows, c.params, c.cons, c.eos, CP.MAX_NEW, scale, mutant=m)
            assert (got[0], got[1]) != (want[0], want[1]), (c.name, m)


def test_the_designed_claims(tables):
    """what the case comments say, read off the restated loop"""
    cfg, T, plan, cases = tables["small"]
    V, Tv, Sv, NV, _ = P.dims(cfg)
    scale, by = P.logit_scale(cfg), {c.name: c for c in cases}
    b = plan.base
    c0, c1, c2 = b.cycle
    q0, q1, q2 = b.cycle_runner
    run = lambda name: CP.restate_batch(T, cfg, by[name].rows, by[name].params, by[name].cons, by[name].eos, CP.MAX_NEW, scale)
    assert run("badword_len1")[0][0][:2] == [c1, q1]
    assert run("badword3_once")[0][0][:3] == [c1, c2, q2]                          # fires at step 2 and at no earlier step
    assert run("badword3_short_history")[0][0][:5] == [c1, c2, c0, c1, q1]         # ... at step 4, not at step 1
    tm = V + 1
    d1 = b.tour[1][0]
    ids = run("badword_cross_heads")[0][0]
    assert ids[:2] == [d1, V] and ids[2] != tm + 5 and tm <= ids[2] < tm + Tv
    ids = run("badword_other_head")[0][0]
    assert ids[:3] == [d1, V, tm + 5] and ids[3] != tm                             # the text id touched nothing under the time head
    b0, m, y0, y1 = plan.begin
    assert run("begin_suppress")[0][0][:4] == [y0, y1, b0, m]                      # banned at step 0 only
    assert run("suppress")[0][0][:7] == [y0, y1, b0, y0, y1, b0, y0]
    ids, lens, _ = run("stop_second_eos")
    assert ids == [[plan.eos2], [b.eos]] and lens == [1, 1]
    assert run("stop3_at_step2")[0] == [[c1, c2, c0]]
    assert run("stop32")[1] == [32]
    assert run("stop_prefix_earlier")[1] == [6] and run("stop_longer_than_history")[1] == [5]
    assert run("stop_other_row")[1] == [CP.MAX_NEW, 3, 5]
    ids, _, heads = run("stop_cross_heads")
    assert ids == [[d1, V, tm + 5, tm]] and heads == [2]
    assert run("stop_not_in_prompt")[0] == [[c1, c2, c0, c1]]
    ids, lens, _ = run("min_new3_two_eos")
    assert all(not {b.eos, plan.eos2} & set(x[:3]) for x in ids) and ids[0] == [b.eos_runner, b.eos_back, b.eos_emitter, b.eos] and lens[1] == 4


# ---------------------------------------------------------------------------------------------------------------- 3: arguments
def test_argument_validation():
    ok = Constraints([[1]] * MAX_SEQS, [list(range(MAX_SEQ_LEN))] * MAX_SEQS, list(range(MAX_SUPPRESS)), list(range(MAX_SUPPRESS)))
    assert not ok.off and Constraints().off and Constraints(None, None, None, None).off
    assert Constraints([[1, 2]]) == Constraints(((1, 2),)) == Constraints([torch.tensor([1, 2])])
    for bad in (dict(stop_sequences=[[1]] * (MAX_SEQS + 1)), dict(bad_words_ids=[[1]] * (MAX_SEQS + 1)), dict(stop_sequences=[[]]),
                dict(bad_words_ids=[[]]), dict(stop_sequences=[list(range(MAX_SEQ_LEN + 1))]), dict(bad_words_ids=[list(range(MAX_SEQ_LEN + 1))]),
                dict(suppress_tokens=list(range(MAX_SUPPRESS + 1))), dict(begin_suppress_tokens=list(range(MAX_SUPPRESS + 1))),
                dict(stop_sequences=[[-1]]), dict(suppress_tokens=[1.5]), dict(bad_words_ids=[1, 2]), dict(stop_sequences="ab"), dict(suppress_tokens=[True])):
        with pytest.raises(ValueError):
            Constraints(**bad)
    c = Constraints([[5, 99]], [[100]], [3], [4])
    check_constraints(c.stop_sequences, c.bad_words_ids, c.suppress_tokens, c.begin_suppress_tokens, 101)
    for n in (100, 99):
        with pytest.raises(ValueError, match="every id"):
            check_constraints(c.stop_sequences, c.bad_words_ids, c.suppress_tokens, c.begin_suppress_tokens, n)


def test_c_struct_is_built_from_the_lists():
    import ctypes as C
    from trace_amd import _lib
    from trace_amd.engine import constraints_c
    k, keep = constraints_c(Constraints([[7, 8, 9], [4]], [[1], [2, 3]], [5, 6], []), 10)
    assert (k.size, k.n_stop, k.n_bad_words, k.n_suppress, k.n_begin_suppress) == (C.sizeof(_lib.TraceConstraintsC), 2, 2, 2, 0)
    arr = lambda p, n: list((C.c_int32 * n).from_address(p))
    assert arr(k.stop_offsets, 3) == [0, 3, 4] and arr(k.stop_ids, 4) == [7, 8, 9, 4]
    assert arr(k.bad_word_offsets, 3) == [0, 1, 3] and arr(k.bad_word_ids, 3) == [1, 2, 3] and arr(k.suppress_ids, 2) == [5, 6]
    assert k.begin_suppress_ids is None
    with pytest.raises(ValueError):
        constraints_c(Constraints([[10]]), 10)


def test_library_exports_and_refuses_bad_tables_before_any_launch():
    """both libraries export the three entry points; the loose ops refuse a bad table on the argument check alone (no GPU here)"""
    import ctypes as C
    from trace_amd import _lib, build
    build.build()
    one = (C.c_int32 * 1)(0)
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        for name in ("trace_decode_set_constraints", "trace_op_logits_process_ex", "trace_op_stop_match"):
            assert hasattr(lib, name)
        P_ = C.addressof(one)                     # any non-null address: the checks below fail before it is read as device memory
        off = (C.c_int32 * 3)(0, 1, 1)            # an empty second sequence
        ids = (C.c_int32 * 2)(1, 2)
        k = _lib.TraceConstraintsC(C.sizeof(_lib.TraceConstraintsC), 2, 0, 0, 0, C.addressof(off), C.addressof(ids), None, None, None, None)
        with pytest.raises(_lib.TraceHipError, match="error -1 in trace_op_stop_match: an empty sequence"):
            lib.trace_op_stop_match(P_, 1, P_, 1, C.byref(k), P_, None)
        k.n_stop = 65
        with pytest.raises(_lib.TraceHipError, match="at most 64 stop"):
            lib.trace_op_stop_match(P_, 1, P_, 1, C.byref(k), P_, None)
        k.n_stop, k.n_suppress = 0, 1025
        with pytest.raises(_lib.TraceHipError, match="at most 1024"):
            lib.trace_op_logits_process_ex(P_, 400, 1, P_, 320, 13, 13, P_, 1, P_, P_, -1, 1.0, 0, 0, C.byref(k), C.addressof(ids), None)
        sup = (C.c_int32 * 1)(400)
        k = _lib.TraceConstraintsC(C.sizeof(_lib.TraceConstraintsC), 0, 0, 1, 0, None, None, None, None, C.addressof(sup), None)
        with pytest.raises(_lib.TraceHipError, match="outside the vocabulary"):
            lib.trace_op_logits_process_ex(P_, 400, 1, P_, 320, 13, 13, P_, 1, P_, P_, -1, 1.0, 0, 0, C.byref(k), C.addressof(ids), None)
        k.size = 8
        with pytest.raises(_lib.TraceHipError, match="size"):
            lib.trace_op_stop_match(P_, 1, P_, 1, C.byref(k), P_, None)


# ---------------------------------------------------------------------------------------------------------------- 4: model.generate's arguments
def _model(**gen_defaults):
    from trace_amd import config as tcfg
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    cfg = tcfg.tiny(num_frames=4)
    m = TraceMistralForCausalLM.__new__(TraceMistralForCausalLM)
    m.config = cfg
    m.generation_config = SimpleNamespace(**gen_defaults)
    return m, cfg


def test_generate_eos_list_and_bad_word_filter():
    m, cfg = _model()
    e = cfg.eos_token_id
    assert m._eos_and_constraints(None, {}, None) == (e, None)
    assert m._eos_and_constraints(7, {}, None) == (7, None)
    assert m._eos_and_constraints(-1, {}, None) == (-1, None)
    eos, c = m._eos_and_constraints([7, 9, 7, 11], {}, None)
    assert eos == 7 and c.stop_sequences == ((9,), (11,)) and not c.bad_words_ids
    eos, c = m._eos_and_constraints(torch.tensor([7, 9]), {"stop_sequences": [[9], [4, 5]], "bad_words_ids": [[7], [9], [9, 7], [12]]}, None)
    assert eos == 7 and c.stop_sequences == ((9,), (4, 5)) and c.bad_words_ids == ((9, 7), (12,))       # [e] is dropped for every EOS id e, as HF does
    kw = {"suppress_tokens": [3], "begin_suppress_tokens": [4], "other": 1}
    eos, c = m._eos_and_constraints(None, kw, None)
    assert c == Constraints((), (), (3,), (4,)) and kw == {"other": 1}                                     # the names are consumed
    with pytest.raises(ValueError, match="every id"):
        m._eos_and_constraints(None, {"suppress_tokens": [cfg.total_vocab]}, None)
    with pytest.raises(ValueError, match="at most"):
        m._eos_and_constraints(None, {"bad_words_ids": [[1, 2]] * 65}, None)


def test_generate_precedence_argument_then_generation_config_then_defaults():
    m, cfg = _model(eos_token_id=[5, 6], suppress_tokens=[1], stop_sequences=[[2, 3]])
    eos, c = m._eos_and_constraints(None, {}, None)
    assert eos == 5 and c == Constraints([[6], [2, 3]], (), [1], ())
    eos, c = m._eos_and_constraints(None, {}, {"eos_token_id": 8, "suppress_tokens": [9]})
    assert eos == 8 and c == Constraints([[2, 3]], (), [9], ())
    eos, c = m._eos_and_constraints(4, {"suppress_tokens": [10], "stop_sequences": [[11]]}, SimpleNamespace(eos_token_id=8, suppress_tokens=[9]))
    assert eos == 4 and c == Constraints([[11]], (), [10], ())


def test_generation_config_json_with_an_eos_list(tmp_path):
    import json
    from trace_amd.model.builder import apply_generation_config
    (tmp_path / "generation_config.json").write_text(json.dumps({"eos_token_id": [2, 32000], "bad_words_ids": [[5, 6]], "temperature": 0.5}))
    m, cfg = _model()
    apply_generation_config(m, str(tmp_path))
    assert m.generation_config.eos_token_id == [2, 32000] and m.generation_config.temperature == 0.5
    cfg2 = dataclasses.replace(cfg, vocab_size=32064)
    m.config = cfg2
    eos, c = m._eos_and_constraints(None, {}, None)
    assert eos == 2 and c == Constraints([[32000]], [[5, 6]])


def test_stop_sequences_from_keywords():
    from trace_amd.mm_utils import KeywordsStoppingCriteria, stop_sequences_from_keywords
    tok = SimpleNamespace(bos_token_id=1, vocab_size=100)
    tok_call = lambda kw: SimpleNamespace(input_ids=[1] + [ord(ch) % 90 + 2 for ch in kw])
    crit = KeywordsStoppingCriteria(["</s>", "#"], type("T", (), {"__call__": lambda self, kw: tok_call(kw), "bos_token_id": 1, "vocab_size": 100})(),
                                    torch.zeros((1, 5), dtype=torch.long))
    got = stop_sequences_from_keywords(crit)
    assert got == [[ord(ch) % 90 + 2 for ch in "</s>"], [ord("#") % 90 + 2]] and all(isinstance(t, int) for w in got for t in w)
    Constraints(stop_sequences=got)
