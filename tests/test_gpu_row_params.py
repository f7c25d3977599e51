"""Per-row sampling, logits processors and max_new_tokens in one decode batch, on the device: select_next_kernel<SELECT_PER_ROW> (csrc/select.h),
the per-row forms of logits_process_kernel and of the log-probability launch, the params that move with a row (csrc/retire.hip) and arrive with an
admission (trace_decode_admit_ex), TraceEngine's row_params= and generate_queue(per_request=True).

Everything runs the identity-layer decoders of tests/token_select_probes.py (with the soft states of tests/row_params_probes.py, where a sampled
row's draw depends on its temperature, top_k, top_p and seed) and of tests/constraint_probes.py: the logits do not depend on rounding and
trace_amd.sampling.sample_row_ref restates the sampler bit for bit, so every assertion is exact equality of ids, lengths, heads and float32
log-probabilities against row_params_probes.restate_rows, whose scenarios tests/test_row_params_cpu.py holds up against the near misses."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import admit_probes as AP  # noqa: E402
import constraint_probes as CP  # noqa: E402
import row_params_probes as RP  # noqa: E402
import token_select_probes as P  # noqa: E402
from trace_amd import _lib, synth  # noqa: E402
from trace_amd.engine import TraceEngine, row_params_c  # noqa: E402
from trace_amd.sampling import Constraints, LogitsParams, RowParams, SamplingParams  # noqa: E402

CHUNK = 4
KINDS = {"bf16": dict(slots=24), "kv8": dict(slots=9, kv_cache="fp8"), "w4": dict(slots=9, llm_w4=True), "f16": dict(slots=9, dtype=torch.float16)}


class Rig:
    """test_gpu_retire.Rig on the table with soft states: P.small(), max_ctx 192, max_new 41, chunk 4"""

    def __init__(self, E, slots, dtype=torch.bfloat16, **engine_kw):
        self.cfg = P.small()
        self.T, self.plan, self.soft = RP.soft_table(self.cfg)
        self.max_new = P.max_new_for(self.cfg, self.plan)
        self.eng = TraceEngine(self.cfg, max_batch=slots, max_ctx=192, max_frames=4, max_new_tokens=self.max_new, dtype=dtype, **engine_kw)
        self.eng.retire_chunk = CHUNK
        self.eng.load_weights(P.crafted_weights(self.cfg, self.T, dtype).items())
        self.ts = E["timestamps"].tolist()
        self.eng.encode_video(synth.synth_frames(self.cfg, 0).to(dtype), self.ts)
        self.L, emb = self.eng.splice(E["input_ids"].tolist(), want_output=True)
        self.emb = emb.clone()
        self.dtype = dtype
        self.start = {}
        self.scale = P.logit_scale(self.cfg, dtype)

    def put(self, slot, start):
        if self.start.get(slot) != start:
            self.emb[-1] = P.embedding_row(self.cfg, start, self.dtype).to(self.emb.device)
            self.eng.prefill(slot, self.L, embeds=self.emb)
            self.start[slot] = start

    def place(self, rows, slot0=0):
        for b, (start, _, _) in enumerate(rows):
            self.put(slot0 + b, start)

    def want(self, sc, **kw):
        return RP.run(self.T, self.cfg, sc, self.max_new, self.scale, **kw)

    def steps(self, n, graph):
        if graph:
            self.eng.decode_steps(n, use_graph=True)
        else:
            for _ in range(n):
                self.eng.decode_steps(1, use_graph=False)

    def read(self, logprobs=False):
        ids, heads = self.eng.decode_read()
        return (ids, [len(x) for x in ids], heads) + ((self.eng.decode_read_logprobs(),) if logprobs else ())


_rigs = {}


@pytest.fixture(scope="module")
def rigs(golden_dir):
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))

    def get(kind="bf16"):
        if kind not in _rigs:
            kw = dict(KINDS[kind])
            _rigs[kind] = Rig(E, kw.pop("slots"), **kw)
        return _rigs[kind]
    yield get
    for r in _rigs.values():
        r.eng.close()
    _rigs.clear()


def forced_of(rows, mn):
    return [list(f) if f is not None else [-1] * mn for _, _, f in rows]


def begin(rig, sc, rows=None, logprobs=False, params="own"):
    """decode_begin over the scenario's rows of origin 0 (or `rows`), each under its own RowParams"""
    idx = [b for b, o in enumerate(sc["origins"]) if o == 0] if rows is None else rows
    rws = [sc["rows"][b] for b in idx]
    rig.place(rws)
    rig.eng.set_logprobs(logprobs)
    rig.eng.decode_begin(list(range(len(rws))), [h for _, h, _ in rws], rig.max_new, sc["eos"], forced_of(rws, rig.max_new),
                         row_params=[sc["params"][b] for b in idx] if params == "own" else params)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 1: the mixed batch
@pytest.mark.parametrize("kind,graph", [("bf16", False)] + [(k, True) for k in KINDS], ids=["bf16-eager"] + [k + "-graph" for k in KINDS])
def test_mixed_batch_equals_the_restatement(rigs, kind, graph):
    """eight rows, each under params of its own: ids, lengths, heads and log-probabilities are the restatement's, eager and replayed, on every kind
    of engine and through the fp16 library (the other kinds replay only: their eager tail is the same launches)"""
    rig = rigs(kind)
    mn = rig.max_new
    sc = RP.mixed_scenario(rig.cfg, rig.plan, rig.soft, mn)
    want = rig.want(sc, logprobs=True)
    try:
        begin(rig, sc, logprobs=True)
        rig.steps(mn - 1, graph)
        ids, lens, heads, lps = rig.read(True)
    finally:
        rig.eng.set_logprobs(False)
    assert ids == want[0], [r for r in range(8) if ids[r] != want[0][r]]
    assert lens == want[1] and [heads[r] for r in range(7)] == want[2][:7]
    assert same_bits(lps, want[3])


# ---------------------------------------------------------------------------------------------------------------- 2: uniform = batch-wide
def test_uniform_row_params_equal_the_batch_wide_setting(rigs):
    """the same rows under one RowParams in every row and under set_sampling / set_logits_params: the per-row form picks what SELECT_TILES (greedy,
    the ties and decoys of P.batch_rows), SELECT_SAMPLE and SELECT_ROW pick, bit for bit"""
    rig = rigs()
    eng, mn, cfg, plan = rig.eng, rig.max_new, rig.cfg, rig.plan
    rows = P.batch_rows(cfg, plan, 8, mn)
    soft = [(rig.soft[r % 2], r % 2, RP.stay(rig.soft[r % 2], mn)) for r in range(4)]
    free = [(plan.chain[(3 * r) % len(plan.chain)][0], plan.chain[(3 * r) % len(plan.chain)][1], None) for r in range(4)]
    sp = RP.S(seed=RP.SEED, **RP.WARPED)
    lp = LogitsParams(repetition_penalty=1.5, no_repeat_ngram_size=3)

    def run(rws, row_params, sampling=None, logits=None):
        rig.place(rws)
        eng.set_sampling(sampling)
        eng.set_logits_params(logits)
        eng.set_logprobs(True)
        try:
            eng.decode_begin(list(range(len(rws))), [h for _, h, _ in rws], mn, plan.eos, None if logits or (row_params and row_params[0].armed) else forced_of(rws, mn),
                             row_params=row_params)
            eng.decode_steps(mn - 1, use_graph=True)
            return rig.read(True)
        finally:
            eng.set_sampling(None)
            eng.set_logits_params(None)
            eng.set_logprobs(False)

    for name, rws, params, kw in (("greedy", rows, RowParams(), {}), ("sampled", soft + rows[:4], RowParams(sp), dict(sampling=sp)),
                                  ("processors", free, RowParams(logits=lp), dict(logits=lp))):
        wide = run(rws, None, **kw)
        per = run(rws, [params] * len(rws))
        assert per[:3] == wide[:3] and same_bits(per[3], wide[3]), name
        # the batch-wide settings are ignored by a per-row batch: set to something else, the rows decode the same
        other = run(rws, [params] * len(rws), sampling=RP.S(seed=5, **RP.COOL), logits=None if name != "processors" else LogitsParams(min_new_tokens=2))
        assert other[:3] == per[:3], name
    assert run(rows, None)[0] == P.restate_batch(rig.T, cfg, rows, plan.eos, mn)[0]


# ---------------------------------------------------------------------------------------------------------------- 3: per-row max_new
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_per_row_max_new(rigs, graph):
    rig = rigs()
    eng, mn = rig.eng, rig.max_new
    sc = RP.max_new_scenario(rig.cfg, rig.plan, rig.soft, mn)
    want = rig.want(sc, logprobs=True)
    assert want[1] == list(RP.MAX_NEWS) * 2
    try:
        begin(rig, sc, logprobs=True)
        rig.steps(mn - 2, graph)
        eng.decode_steps(1, use_graph=graph)                       # the last step any row has left
        with pytest.raises(_lib.TraceHipError, match="decode steps exceed"):
            eng.decode_steps(1, use_graph=graph)                   # refused exactly when no row has a step of its own left
        ids, lens, heads, lps = rig.read(True)
        assert ids == want[0] and lens == want[1] and same_bits(lps, want[3])
        assert all((lps[r, lens[r]:] == 0).all() for r in range(8))
        begin(rig, sc, logprobs=True, params=[RowParams(p.sampling) for p in sc["params"]])        # every row at the batch's 41
        rig.steps(mn - 1, graph)
        full = rig.read(True)
        assert all(full[0][r][:lens[r]] == ids[r] for r in range(8)) and full[0][3] == ids[3] and full[0][7] == ids[7]
        short = dict(sc, params=[RowParams(max_new_tokens=2)] * 8)
        begin(rig, short)
        eng.decode_steps(1, use_graph=graph)
        with pytest.raises(_lib.TraceHipError, match="decode steps exceed"):
            eng.decode_steps(1, use_graph=graph)
    finally:
        eng.set_logprobs(False)


# ---------------------------------------------------------------------------------------------------------------- 4: retire
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_params_move_with_a_retired_row(rigs, graph):
    rig = rigs()
    eng, mn = rig.eng, rig.max_new
    sc = RP.retire_scenario(rig.cfg, rig.plan, rig.soft, mn, CHUNK)
    want = rig.want(sc, logprobs=True)
    keep = sc["retire"][1]
    try:
        begin(rig, sc, logprobs=True)
        rig.steps(CHUNK, graph)
        first = rig.read(True)
        eng.retire_rows(keep)
        rig.steps(mn - 1 - CHUNK, graph)
        ids, lens, heads, lps = rig.read(True)
        assert [first[0][r] for r in (0, 2, 5)] == [want[0][r] for r in (0, 2, 5)]
        assert ids == [want[0][r] for r in keep] and lens == [want[1][r] for r in keep] and heads[:2] == [want[2][r] for r in keep[:2]]
        assert same_bits(lps, want[3][keep])
        begin(rig, sc, logprobs=True)                             # the unretired run's rows
        rig.steps(mn - 1, graph)
        whole = rig.read(True)
        assert [whole[0][r] for r in keep] == ids and same_bits(whole[3][keep], lps)
    finally:
        eng.set_logprobs(False)


# ---------------------------------------------------------------------------------------------------------------- 5: admit
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_admitted_rows_bring_their_params(rigs, graph):
    rig = rigs()
    eng, mn = rig.eng, rig.max_new
    sc = RP.admit_scenario(rig.cfg, rig.plan, rig.soft, mn, CHUNK)
    want = rig.want(sc, logprobs=True)
    new = sc["rows"][3:]
    try:
        rig.place(new, slot0=3)
        begin(rig, sc, logprobs=True)
        rig.steps(CHUNK, graph)
        eng.admit_rows_ex([3, 4, 5], [h for _, h, _ in new], sc["params"][3:], row_ids=sc["row_ids"][3:], forced=forced_of(new, mn))
        rig.steps(mn - 1, graph)                                  # the admitted rows' own max_new - 1: the first three are stepped past theirs
        ids, lens, heads, lps = rig.read(True)
        assert ids == want[0] and lens == want[1] and same_bits(lps, want[3])
        begin(rig, sc, logprobs=True)                             # the running rows without the admission
        rig.steps(mn - 1, graph)
        plain = rig.read(True)
        assert plain[0] == ids[:3] and same_bits(plain[3], lps[:3])
    finally:
        eng.set_logprobs(False)


# ---------------------------------------------------------------------------------------------------------------- 6: processors per row
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_processors_per_row_on_the_constraint_table(golden_dir, graph):
    import test_gpu_constraints as TC
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    rig = TC.Rig("small", E, slots=8)
    try:
        eng, mn = rig.eng, rig.max_new
        sc = RP.processor_scenario(rig.cfg, rig.plan)
        want = RP.run(rig.T, rig.cfg, sc, mn, rig.scale)
        rig.place([(t, h) for t, h, _ in sc["rows"]])
        eng.set_constraints(sc["cons"])
        try:
            eng.decode_begin(list(range(6)), [h for _, h, _ in sc["rows"]], mn, eos=sc["eos"], row_params=sc["params"])
            if graph:
                eng.decode_steps(mn - 1, use_graph=True)
            else:
                for _ in range(mn - 1):
                    eng.decode_steps(1, use_graph=False)
            ids, heads = eng.decode_read()
        finally:
            eng.set_constraints(None)
        assert ids == want[0] and [len(x) for x in ids] == want[1]
    finally:
        rig.eng.close()


# ---------------------------------------------------------------------------------------------------------------- 7: the queue
def test_queue_with_per_request_params(rigs):
    """24 requests through 8 rows, chunk 4: EOS positions of admit_probes.QUEUE_ENDS, params cycling through four sets, max_new_tokens through 3, 12, 41"""
    rig = rigs()
    cfg, plan, mn, eng, eos = rig.cfg, rig.plan, rig.max_new, rig.eng, rig.plan.eos
    rows = [RP.queue_row(plan, rig.soft, r, at, mn) for r, at in enumerate(AP.QUEUE_ENDS)]
    params = [RP.queue_params(r, mn) for r in range(24)]
    # every request restated alone with its Philox row index (its request index: one batch is begun)
    want = [RP.alone(rig.T, cfg, rows[r], eos, mn, rig.scale, params[r], row_id=r, logprobs=True) for r in range(24)]
    lengths, bounds = [w[1] for w in want], [p.max_new_tokens for p in params]
    steps, sizes, admits, retires, begun = RP.queue_schedule(lengths, bounds, 8, CHUNK)
    assert begun == 1 and admits >= 2 and retires >= 2
    for r, (s, _, _) in enumerate(rows):
        rig.put(r, s)
    a0, r0, s0 = eng.admits, eng.retires, eng.stats["decode_row_steps"]
    got = eng.decode_queue(list(range(24)), [h for _, h, _ in rows], mn, eos, max_rows=8, forced=[f for _, _, f in rows], logprobs=True, row_params=params)
    assert [g[0] for g in got] == [w[0] for w in want]
    assert all(same_bits(g[2], w[3][:w[1]]) for g, w in zip(got, want))
    assert (eng.stats["decode_row_steps"] - s0, eng.admits - a0, eng.retires - r0) == (steps, admits, retires)
    # through generate_queue, the encode stage included: the same results
    base = synth.synth_prompt_ids(cfg, n_text=24, video_pos=10).tolist()
    vid = synth.synth_frames(cfg, 1).to(torch.bfloat16).cuda()
    reqs = [(vid, rig.ts, base[:-1] + [s], h, f) for s, h, f in rows]
    rig.start.clear()
    full = eng.generate_queue(iter(r + (p,) for r, p in zip(reqs, params)), mn, eos, max_rows=8, per_request=True)
    assert [g[0] for g in full] == [w[0] for w in want]
    # per_request=False and no sixth element: what the parent gives (greedy, one bound)
    plainrows = [RP.ending_row(plan, r, at, mn) for r, at in enumerate(AP.QUEUE_ENDS)]
    s1 = eng.stats["decode_row_steps"]
    plain = eng.generate_queue([(vid, rig.ts, base[:-1] + [s], 0, f) for s, _, f in plainrows], mn, eos, max_rows=8)
    ref = P.restate_batch(rig.T, cfg, plainrows, eos, mn)
    assert [g[0] for g in plain] == ref[0] and eng.stats["decode_row_steps"] - s1 == AP.queue_schedule(ref[1], mn, 8, CHUNK)[0] == 376
    with pytest.raises(ValueError, match="per_request=True"):
        eng.generate_queue([reqs[0] + (params[0],)], mn, eos)
    rig.start.clear()


# ---------------------------------------------------------------------------------------------------------------- 8: errors
def test_errors_leave_the_batch_as_it_was(rigs):
    rig = rigs()
    eng, mn, lib = rig.eng, rig.max_new, rig.eng.lib
    sc = RP.mixed_scenario(rig.cfg, rig.plan, rig.soft, mn)
    want = rig.want(sc)
    rig.place(sc["rows"])
    rig.put(8, rig.soft[0])
    heads = [h for _, h, _ in sc["rows"]]
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)
    ok = lambda n: row_params_c([RowParams()] * n, mn)

    def refused(match, fn):
        with pytest.raises(_lib.TraceHipError, match=match):
            fn()

    def raw_begin(n_rows, arr, n_arr, max_new=mn, forced=None):
        lib.trace_decode_set_row_params(eng.h, arr, n_arr)
        lib.trace_decode_begin(eng.h, i32(list(range(n_rows))), n_rows, i32(heads[:n_rows]), max_new, sc["eos"], forced, None, None)

    taken = [0]

    def step_on():
        """one more step of the running batch: it is as it was (the ids at the end are the restatement's)"""
        rig.steps(1, True)
        taken[0] += 1

    begin(rig, sc)
    step_on()
    # --- a begin that is refused leaves the running batch alone
    refused("rows, the batch has", lambda: raw_begin(8, ok(5), 5))                                          # n != B
    step_on()
    bad = ok(8)
    bad[2].sampling.temperature, bad[2].sampling.top_k = 1.0, 2000
    refused("top_k", lambda: lib.trace_decode_set_row_params(eng.h, bad, 8))                               # top_k 2000
    step_on()
    bad = ok(8)
    bad[3].max_new = 0
    refused("max_new of a row", lambda: lib.trace_decode_set_row_params(eng.h, bad, 8))                    # max_new 0
    step_on()
    refused("max_new of a row", lambda: raw_begin(8, ok(8), 8, max_new=mn - 1))                             # max_new above the batch's
    step_on()
    eng.host_mode(True)
    try:
        refused("host-select", lambda: lib.trace_decode_set_row_params(eng.h, ok(8), 8))                   # host mode
    finally:
        eng.host_mode(False)
    step_on()
    armed = row_params_c([RowParams(logits=LogitsParams(repetition_penalty=1.3))] * 8, mn)
    refused("forced ids on a row", lambda: raw_begin(8, armed, 8, forced=i32(sum(forced_of(sc["rows"], mn), []))))    # forced ids on a row with processors
    step_on()
    with pytest.raises(ValueError):
        eng.decode_begin([0, 1], [0, 0], mn, row_params=[RowParams(SamplingParams(1.0, 2000, 1.0))] * 2)
    # --- so does a refused admission
    refused("begun with per-row params", lambda: eng.admit_rows([8], [0]))                                 # plain admit into a per-row batch
    step_on()
    refused("max_new of a row", lambda: lib.trace_decode_admit_ex(eng.h, i32([8]), 1, i32([0]), i32([8]), None, _over(mn), None))
    step_on()
    rig.steps(mn - 1 - taken[0], True)
    ids, lens, heads_now = rig.read()
    assert ids == want[0] and lens == want[1]                                                              # it ran on to the restatement
    # --- rows into a plain batch
    rig.eng.decode_begin(list(range(8)), heads, mn, sc["eos"], forced_of(sc["rows"], mn))
    rig.steps(CHUNK, True)
    refused("begun without per-row params", lambda: eng.admit_rows_ex([8], [0], [RowParams()]))    # _ex with rows into a plain batch
    rig.steps(mn - 1 - CHUNK, True)
    assert rig.read()[0] == P.restate_batch(rig.T, rig.cfg, [(t, h, f) for (t, h, _), f in zip(sc["rows"], forced_of(sc["rows"], mn))], sc["eos"], mn)[0]


def _over(mn):
    """one trace_row_params whose max_new is above the batch's (built by hand: row_params_c refuses it)"""
    arr = row_params_c([RowParams()], mn)
    arr[0].max_new = mn + 1
    return arr


# ---------------------------------------------------------------------------------------------------------------- 9: graphs
def test_per_row_batches_capture_graphs_of_their_own(rigs):
    rig = rigs()
    eng, mn = rig.eng, rig.max_new

    def sizes():
        buf = (C.c_int32 * 257)()
        n = eng.lib.trace_debug_step_graphs(eng.h, buf, 257)
        return set(buf[:n])

    rows = P.batch_rows(rig.cfg, rig.plan, 5, mn)
    want = P.restate_batch(rig.T, rig.cfg, rows, -1, mn)
    rig.place(rows)

    def plain():
        eng.decode_begin(list(range(5)), [h for _, h, _ in rows], mn, -1, forced_of(rows, mn))
        eng.decode_steps(mn - 1, use_graph=True)
        return rig.read()

    assert plain()[0] == want[0] and 5 in sizes()
    g0 = sizes()
    sc = RP.sampled_first_scenario(rig.cfg, rig.plan, rig.soft, mn)
    begin(rig, sc)                                                 # four rows: a size no plain batch of this test has captured
    rig.steps(mn - 1, True)
    assert rig.read()[0] == rig.want(sc)[0]
    assert sizes() >= g0 | {4}
    rig.place(rows)
    assert plain()[0] == want[0] and sizes() >= g0 | {4}           # the plain batch replays the graph it had: the same ids
