"""Constraints on the device (trace_amd/csrc/constrain.h): bad words, suppressed ids, begin-suppress, stop sequences and several EOS ids inside the
decode step.

The loose-row ops are held against the numpy restatement with torch.equal (sampling.constrain_row_ref / stop_match_ref, which
tests/test_constraints_cpu.py holds against HF's own processors).  The decode step runs on the identity-layer decoder of tests/token_select_probes.py
with the table of tests/constraint_probes.py, where every rule has one right answer per step: ids, lengths and final heads are compared for exact
equality with CP.restate, eager and graph-replayed, at B = 1, 3 and 65 (the wide step), greedy and sampled; log-probabilities stay those of the RAW
row; model.generate() takes the HF arguments in the device loop and in the stepwise (stopping-criteria) loop alike."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import constraint_probes as CP  # noqa: E402
import token_select_probes as P  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402
from trace_amd.sampling import (Constraints, LogitsParams, SamplingParams, constrain_row_ref, process_row_ref, stop_match_ref,  # noqa: E402
                                token_logprob_ref)

SLOTS = 65


class Rig:
    def __init__(self, geom, E, slots=SLOTS, **engine_kw):
        self.cfg = CP.GEOMETRIES[geom]()
        self.T, self.plan = CP.build_table(self.cfg)
        self.max_new = CP.MAX_NEW
        self.eng = TraceEngine(self.cfg, max_batch=slots, max_ctx=160, max_frames=4, max_new_tokens=self.max_new, **engine_kw)
        self.eng.load_weights(P.crafted_weights(self.cfg, self.T).items())
        self.eng.encode_video(synth.synth_frames(self.cfg, 0).to(torch.bfloat16), E["timestamps"].tolist())
        self.L, emb = self.eng.splice(E["input_ids"].tolist(), want_output=True)
        self.emb = emb.clone()
        self.start = {}
        self.scale = P.logit_scale(self.cfg)
        self.cases = {c.name: c for c in CP.decode_cases(self.cfg, self.plan)}
        self._want = {}

    def place(self, rows):
        """slot b <- the prompt whose last row is row b's start token (kept from earlier batches where it is the same)"""
        for b, (start, _) in enumerate(rows):
            if self.start.get(b) != start:
                self.emb[-1] = P.embedding_row(self.cfg, start).to(self.emb.device)
                self.eng.prefill(b, self.L, embeds=self.emb)
                self.start[b] = start

    def run(self, rows, params, cons, eos, graph, sampling=None):
        """(ids, lengths, heads): decode_begin and max_new - 1 steps, replayed from the captured graph or eager one at a time"""
        self.place(rows)
        eng, mn = self.eng, self.max_new
        eng.set_logits_params(params)
        eng.set_constraints(cons)
        eng.set_sampling(sampling)
        try:
            eng.decode_begin(list(range(len(rows))), [h for _, h in rows], mn, eos=eos)
            if graph:
                eng.decode_steps(mn - 1, use_graph=True)
            else:
                for _ in range(mn - 1):
                    eng.decode_steps(1, use_graph=False)
            ids, heads = eng.decode_read()
        finally:
            eng.set_logits_params(None)
            eng.set_constraints(None)
            eng.set_sampling(None)
        return ids, [len(x) for x in ids], heads

    def want(self, rows, params, cons, eos, sampling=None):
        """the restated loop, one row at a time; a greedy row depends on its start state alone, so it is computed once per (rules, start)"""
        sp = None if sampling is None else (sampling.temperature, sampling.top_k, sampling.top_p, sampling.seed)
        cons = cons if cons is not None else Constraints()
        out = []
        for b, (t, h) in enumerate(rows):
            key = (params, cons, eos, t, h) if sp is None else None
            if key is None or key not in self._want:
                r = CP.restate(self.T, self.cfg, t, h, params, cons, eos, self.max_new, self.scale, sampling=sp, row_index=b)
                if key is None:
                    out.append(r)
                    continue
                self._want[key] = r
            out.append(self._want[key])
        return [list(o[0]) for o in out], [o[1] for o in out], [o[2] for o in out]

    def check(self, rows, params, cons, eos, graph, tag, sampling=None):
        want, got = self.want(rows, params, cons, eos, sampling), self.run(rows, params, cons, eos, graph, sampling)
        if got != want:
            bad = [b for b in range(len(rows)) if (got[0][b], got[1][b], got[2][b]) != (want[0][b], want[1][b], want[2][b])]
            b = bad[0]
            raise AssertionError(f"{tag}: {len(bad)} of {len(rows)} rows differ; row {b} (start {rows[b]}): got {got[0][b]} head {got[2][b]}, "
                                 f"want {want[0][b]} head {want[2][b]}")
        return got


_rigs = {}


@pytest.fixture(scope="module")
def rigs(golden_dir):
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))

    def get(geom):
        if geom not in _rigs:
            _rigs[geom] = Rig(geom, E)
        return _rigs[geom]
    yield get
    for r in _rigs.values():
        r.eng.close()
    _rigs.clear()


def rows_for(rig, case, B):
    """the case's own rows (B = None), or those rows and then wide_rows' different start states up to B rows"""
    if B is None:
        return case.rows
    return (list(case.rows) + CP.wide_rows(rig.plan, B))[:B]


# ---------------------------------------------------------------------------------------------------------------- 1: the loose-row ops
@pytest.mark.parametrize("element", ["bf16", "f16"])
@pytest.mark.parametrize("geom", list(CP.GEOMETRIES))
def test_logits_process_ex_equals_restatement(geom, element):
    """every row of CP.row_cases, in batches of 17, 3 and 1 rows with a different history and table use per row; torch.equal on the whole output
    row (the head range AND -inf everywhere else); the input row stays untouched.  Both with and without logits processors in front."""
    cfg = CP.GEOMETRIES[geom]()
    V, Tv, Sv, NV, _ = P.dims(cfg)
    cases = CP.row_cases(cfg)
    sizes, rows_run = [17, 3, 1], 0
    for gi, c0 in enumerate(cases):
        # the table and min_new_tokens of case gi over its own row and the rows, heads, histories and steps of the cases behind it
        cons, min_new = c0.cons, c0.min_new
        params = LogitsParams(1.3 if gi % 2 else 1.0, 0, min_new)
        part = [cases[(gi + 7 * j) % len(cases)] for j in range(sizes[gi % 3])]
        B = len(part)
        x = np.stack([c.row for c in part])
        lg = torch.from_numpy(x).cuda()
        eos = int(cons.stop_sequences[1][0])
        got = ops.logits_process_ex(lg, [c.head for c in part], [c.hist for c in part], params, [c.step for c in part], eos, cons, V, Tv, Sv,
                                    element=element).cpu()
        assert np.array_equal(lg.cpu().numpy(), x)
        for b, c in enumerate(part):
            lo, hi = P.head_range(cfg, c.head)
            want = constrain_row_ref(process_row_ref(c.row, c.hist, lo, hi, params, c.step, eos), c.hist, lo, hi, cons, c.step, min_new)
            assert torch.equal(got[b], torch.from_numpy(want)), (geom, gi, b, c.head, len(c.hist), c.step, min_new)
            assert bool((got[b, :lo] == float("-inf")).all()) and bool((got[b, hi:] == float("-inf")).all())
        rows_run += B
    assert rows_run > 7 * len(cases) // 2
    # no table: the op is trace_op_logits_process
    c = CP.row_cases(cfg)[5]
    lg = torch.from_numpy(c.row[None]).cuda()
    a = ops.logits_process_ex(lg, [c.head], [c.hist], LogitsParams(1.3, 2, 0), [1], -1, None, V, Tv, Sv, element=element)
    assert torch.equal(a, ops.logits_process(lg, [c.head], [c.hist], LogitsParams(1.3, 2, 0), [1], -1, V, Tv, Sv, element=element))


@pytest.mark.parametrize("element", ["bf16", "f16"])
@pytest.mark.parametrize("geom", list(CP.GEOMETRIES))
def test_stop_match_equals_restatement(geom, element):
    """histories shorter than, as long as and longer than the sequences (1, 2, 3, 32 ids; 64 sequences at once), one workgroup per history"""
    cfg = CP.GEOMETRIES[geom]()
    fired = 0
    for hists, cons in CP.history_cases(cfg):
        got = ops.stop_match(hists, cons, element=element).cpu()
        want = torch.tensor([1 if stop_match_ref(h, cons) else 0 for h in hists], dtype=torch.int32)
        assert torch.equal(got, want), (geom, got.tolist(), want.tolist())
        fired += int(want.sum())
    assert fired >= 12


# ---------------------------------------------------------------------------------------------------------------- 2: the decode step
CASES = [c.name for c in CP.decode_cases(P.small(), CP.build_table(P.small())[1])]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("geom", list(CP.GEOMETRIES))
def test_decode_equals_restatement(rigs, geom, case, graph):
    """ids, lengths and final heads of every row, exactly, for the case's own rows (B = 1 .. 4), at B = 3 and at B = 65 (the wide step), where the
    rows behind the case's own start in different states and so carry different histories"""
    rig = rigs(geom)
    c = rig.cases[case]
    for B in (None, 3, 65):
        rig.check(rows_for(rig, c, B), c.params, c.cons, c.eos, graph, f"{geom} {case} B={B}")


def test_decode_claims_hold_on_the_device(rigs):
    """the claims themselves, read off the device's ids"""
    rig = rigs("small")
    plan, V = rig.plan, rig.cfg.vocab_size
    c0, c1, c2 = plan.base.cycle
    b0, m, y0, y1 = plan.begin
    run = lambda name, g=True: rig.run(rig.cases[name].rows, rig.cases[name].params, rig.cases[name].cons, rig.cases[name].eos, g)
    assert run("badword3_once")[0][0][:3] == [c1, c2, plan.base.cycle_runner[2]]
    assert run("begin_suppress")[0][0][:4] == [y0, y1, b0, m]
    assert run("stop3_at_step2")[0] == [[c1, c2, c0]]
    ids, lens, heads = run("stop_cross_heads")
    assert ids == [[plan.base.tour[1][0], V, V + 6, V + 1]] and heads == [2]
    assert run("stop32")[1] == [32] and run("stop_other_row")[1] == [CP.MAX_NEW, 3, 5]
    ids, lens, _ = run("min_new3_two_eos")
    assert all(not {plan.base.eos, plan.eos2} & set(x[:3]) for x in ids) and lens[:2] == [4, 4]


def test_table_changes_between_batches_without_recapture(rigs):
    """the captured step reads the table from device memory: batches of one size replay one graph per mode, each under its own table"""
    rig = rigs("small")
    names = ("stop3_at_step2", "stop32", "stop_prefix_earlier", "stop3_at_step2", "badword_len1", "badword3_once", "suppress", "badword_len1")
    for n in names:
        k = rig.cases[n]
        rig.check(rows_for(rig, k, 3), k.params, k.cons, k.eos, True, f"replay {n}")


# ---------------------------------------------------------------------------------------------------------------- 3: sampling, log-probabilities
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("geom", list(CP.GEOMETRIES))
def test_sampling_draws_from_the_constrained_row(rigs, geom, graph):
    """temperature 0.7, top_k 5, top_p 0.9, a fixed seed: every id is the host sampler's on the constrained row under the step's Philox counter"""
    rig = rigs(geom)
    sp = SamplingParams(0.7, 5, 0.9, seed=0x1234ABCD5678)
    c = rig.cases["all_rules"]
    rig.check(rows_for(rig, c, 17), c.params, c.cons, c.eos, graph, f"{geom} sampled all_rules", sampling=sp)
    c = rig.cases["suppress"]
    rig.check(rows_for(rig, c, 3), None, c.cons, -1, graph, f"{geom} sampled suppress", sampling=sp)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_logprobs_describe_the_raw_row(rigs, sampled):
    """constraints on: logprob[b][s] is token_logprob_ref of the RAW row at the emitted id, bit for bit - not of the constrained row"""
    rig = rigs("small")
    cfg, mn = rig.cfg, rig.max_new
    c = rig.cases["suppress"]
    rows = rows_for(rig, c, 3)
    sp = SamplingParams(0.7, 5, 0.9, seed=77) if sampled else None
    rig.place(rows)
    ids, heads, lps = rig.eng.decode(list(range(3)), [h for _, h in rows], mn, eos=-1, sampling=sp, logprobs=True, constraints=c.cons)
    want = rig.want(rows, None, c.cons, -1, sp)
    assert (ids, heads) == (want[0], want[2])
    differs = 0
    for b, (t, h) in enumerate(rows):
        tr = []
        CP.restate(rig.T, cfg, t, h, None, c.cons, -1, mn, rig.scale, sampling=None if sp is None else (0.7, 5, 0.9, 77), row_index=b, trace=tr)
        for s, (state, head, raw, row, tok) in enumerate(tr[:len(ids[b])]):
            lo, hi = P.head_range(cfg, head)
            ref = token_logprob_ref(raw[lo:hi], tok - lo)
            assert np.float32(lps[b][s]).tobytes() == np.float32(ref).tobytes(), (b, s, lps[b][s], ref)
            differs += token_logprob_ref(row[lo:hi], tok - lo) != ref
    assert differs > 0                           # the constrained row would have given other values: the test can tell the two apart


# ---------------------------------------------------------------------------------------------------------------- 4: disarmed, fp8 KV, stepwise, errors
def test_disarmed_after_an_armed_batch_is_a_context_that_never_armed(rigs, golden_dir):
    rig = rigs("small")
    c = rig.cases["all_rules"]
    rows = rows_for(rig, c, 3)
    rig.run(rows, c.params, c.cons, c.eos, True)
    got = [rig.run(rows, None, None, c.eos, g) for g in (True, False)]
    fresh = Rig("small", np.load(os.path.join(golden_dir, "tiny_e2e.npz")), slots=3)
    try:
        fresh.place(rows)
        fresh.eng.decode_begin([0, 1, 2], [h for _, h in rows], fresh.max_new, eos=c.eos)
        fresh.eng.decode_steps(fresh.max_new - 1, use_graph=True)
        ids, heads = fresh.eng.decode_read()
    finally:
        fresh.eng.close()
    assert got[0] == got[1] == (ids, [len(x) for x in ids], heads)
    assert got[0] == rig.want(rows, None, Constraints(), c.eos)


def test_fp8_kv_cache_engine(golden_dir):
    rig = Rig("small", np.load(os.path.join(golden_dir, "tiny_e2e.npz")), slots=4, kv_cache="fp8")
    try:
        c = rig.cases["all_rules"]
        for graph in (False, True):
            rig.check(c.rows, c.params, c.cons, c.eos, graph, f"fp8 kv all_rules graph={graph}")
    finally:
        rig.eng.close()


@pytest.mark.parametrize("case", ["all_rules", "stop_other_row", "min_new3_two_eos", "badword_other_head"])
def test_decode_stepwise_returns_the_ids_of_decode(rigs, case):
    rig = rigs("small")
    c = rig.cases[case]
    rig.place(c.rows)
    slots, heads = list(range(len(c.rows))), [h for _, h in c.rows]
    a = rig.eng.decode(slots, heads, rig.max_new, eos=c.eos, logits=c.params, constraints=c.cons)
    b = rig.eng.decode_stepwise(slots, heads, rig.max_new, eos=c.eos, logits=c.params, constraints=c.cons)
    want = rig.want(c.rows, c.params, c.cons, c.eos)
    assert a[0] == b[0] == want[0]
    sp = SamplingParams(0.7, 5, 0.9, seed=5)
    a = rig.eng.decode(slots, heads, rig.max_new, eos=c.eos, logits=c.params, constraints=c.cons, sampling=sp)
    b = rig.eng.decode_stepwise(slots, heads, rig.max_new, eos=c.eos, logits=c.params, constraints=c.cons, sampling=sp)
    assert a[0] == b[0] == rig.want(c.rows, c.params, c.cons, c.eos, sp)[0]


def test_argument_errors(rigs):
    import ctypes as C
    rig = rigs("small")
    eng, NV = rig.eng, P.dims(rig.cfg)[3]
    rows = [(rig.plan.base.cycle[0], 0)]
    rig.place(rows)
    err_arg = r"error -1 in "                     # TRACE_ERR_ARG
    for bad in (Constraints(stop_sequences=[[NV]]), Constraints(bad_words_ids=[[1, NV]]), Constraints(suppress_tokens=[NV]),
                Constraints(begin_suppress_tokens=[NV + 5])):
        with pytest.raises(ValueError, match="every id"):
            eng.set_constraints(bad)
        with pytest.raises(ValueError, match="every id"):
            eng.decode([0], [0], rig.max_new, constraints=bad)
    sup = (C.c_int32 * 1)(NV)
    k = _lib.TraceConstraintsC(C.sizeof(_lib.TraceConstraintsC), 0, 0, 1, 0, None, None, None, None, C.addressof(sup), None)
    with pytest.raises(_lib.TraceHipError, match=err_arg + "trace_decode_set_constraints"):
        eng.lib.trace_decode_set_constraints(eng.h, C.byref(k))
    k.n_suppress = 1025
    with pytest.raises(_lib.TraceHipError, match=err_arg + "trace_decode_set_constraints"):
        eng.lib.trace_decode_set_constraints(eng.h, C.byref(k))
    for cons in (Constraints(stop_sequences=[[3]]), Constraints(suppress_tokens=[3])):
        eng.set_constraints(cons)
        try:
            with pytest.raises(_lib.TraceHipError, match=err_arg + "trace_decode_begin"):
                eng.decode_begin([0], [0], rig.max_new, eos=-1, forced=[[1] * rig.max_new])
        finally:
            eng.set_constraints(None)
    eng.decode_begin([0], [0], rig.max_new, eos=-1, forced=[[1] * rig.max_new])           # disarmed: forced ids are welcome again
    with pytest.raises(ValueError, match="forced"):
        eng.decode([0], [0], rig.max_new, forced=[[1] * rig.max_new], constraints=Constraints(stop_sequences=[[3]]))
    with pytest.raises(ValueError, match="forced"):
        eng.decode_stepwise([0], [0], rig.max_new, forced=[[1] * rig.max_new], constraints=Constraints(stop_sequences=[[3]]))
    got = rig.check(rows, None, None, -1, True, "after the errors")                        # nothing stayed armed
    assert got[1] == [rig.max_new]


# ---------------------------------------------------------------------------------------------------------------- 5: model.generate
class _Keywords:
    """KeywordsStoppingCriteria's id half on given ids (no tokenizer: the keyword ids are handed in)"""

    def __init__(self, keyword_ids):
        self.keyword_ids = [torch.tensor(k) for k in keyword_ids]

    def __call__(self, output_ids, scores=None, **kwargs):
        out = []
        for row in output_ids:
            out.append(any(row.numel() >= k.numel() and bool((row[-k.numel():] == k).all()) for k in self.keyword_ids))
        return torch.tensor(out)


def test_model_generate_takes_the_arguments_in_both_loops(golden_dir):
    """model.generate(eos_token_id=[a, b], bad_words_ids=, suppress_tokens=, begin_suppress_tokens=, stop_sequences=) on the probe model (the
    crafted weights behind a TraceMistralForCausalLM): the device loop and the same call with a stopping criterion that never fires (the stepwise
    loop) give the restated ids; stop_sequences_from_keywords of a keyword criterion gives the host loop's ids"""
    from trace_amd.mm_utils import stop_sequences_from_keywords
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    rig = Rig("small", E, slots=2)
    try:
        cfg, plan = rig.cfg, rig.plan
        model = TraceMistralForCausalLM(cfg, rig.eng, None)
        frames = synth.synth_frames(cfg, 0).to(torch.bfloat16).cuda()
        ts = E["timestamps"].tolist()
        prompt = E["input_ids"].tolist()
        c0, c1, c2 = plan.base.cycle
        b0, m, y0, y1 = plan.begin
        # the prompt's last id decides the start state: the embedding of a text id with a column is one-hot there
        def call(start, **kw):
            ids = torch.tensor([prompt[:-1] + [start]])
            out = model.generate(ids, images_or_videos=[frames], modal_list=["video"], video_timestamps=[ts], heads=[0], max_new_tokens=CP.MAX_NEW,
                                 pad_token_id=0, **kw)
            return out[0].tolist()
        never = [lambda i, s: False]
        # two EOS ids: the row from g ends on eos2, the row from e on eos
        for start, last in ((plan.eos2_emitter, plan.eos2), (plan.base.eos_emitter, plan.base.eos)):
            for extra in ({}, {"stopping_criteria": never}):
                assert call(start, eos_token_id=[plan.base.eos, plan.eos2], **extra) == [last]
        kw = dict(eos_token_id=[plan.base.eos, plan.eos2], bad_words_ids=[[c1, c2, c0], [plan.base.eos]], suppress_tokens=[m],
                  begin_suppress_tokens=[c1], stop_sequences=[[y1, b0, y0, y1]])
        cons = Constraints([[plan.eos2], [y1, b0, y0, y1]], [[c1, c2, c0]], [m], [c1])
        for start in (c0, b0, plan.base.eos_emitter):
            want, n, _ = CP.restate(rig.T, cfg, start, 0, None, cons, plan.base.eos, CP.MAX_NEW, rig.scale)
            plain, _, _ = CP.restate(rig.T, cfg, start, 0, None, Constraints(), plan.base.eos, CP.MAX_NEW, rig.scale)
            a, b = call(start, **kw), call(start, stopping_criteria=never, **kw)
            assert a == b == want, (start, a, b, want)
            assert want != plain or start == plan.base.eos_emitter                   # ([eos] as a bad word is dropped: e still emits eos)
        assert call(plan.base.eos_emitter, **kw) == [plan.base.eos]
        # generation_config carries them too; an explicit argument wins
        gc = {"stop_sequences": [[y0, y1]], "suppress_tokens": [m]}                    # (m suppressed: b0 emits y0, then y1)
        assert call(b0, generation_config=gc, eos_token_id=-1) == [y0, y1]
        assert call(b0, generation_config=gc, stop_sequences=[[y0]], eos_token_id=-1) == [y0]
        # the reference's keyword criterion against its id half on the device
        crit = _Keywords([[c2, c0], [y1, b0]])
        for start, n in ((c0, 3), (c1, 2)):
            host = call(start, stopping_criteria=[crit], eos_token_id=-1)
            dev = call(start, stop_sequences=stop_sequences_from_keywords(crit), eos_token_id=-1)
            want, _, _ = CP.restate(rig.T, cfg, start, 0, None, Constraints(stop_sequences=[[c2, c0], [y1, b0]]), -1, CP.MAX_NEW, rig.scale)
            assert host == dev == want and len(dev) == n, (start, host, dev, want)
    finally:
        rig.eng.close()
