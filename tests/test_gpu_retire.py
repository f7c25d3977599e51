"""Retiring finished rows from a running decode batch on the device: trace_decode_retire (csrc/retire.hip), TraceEngine.retire_rows and
decode(..., retire_finished=True).

Parts 1-4, 6 and 7 run the identity-layer decoder of tests/token_select_probes.py, whose logits do not depend on rounding: every id, length and
(for live rows) head has one right answer, P.restate_batch, whatever batch size a row is decoded in, so every assertion there is exact equality.
The engine's chunk is set to 4 steps on the instance, so several retires happen within max_new_for(...) = 41 tokens.  Part 5 runs the tiny Gaussian
model: there a row that decodes on in a smaller batch sees that batch's rounding, and the check is a bound measured on existing code inside the
test.  A retired row's returned head is the one it had when it left; heads are compared for the rows live at the end only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import token_select_probes as P  # noqa: E402
from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402
from trace_amd.sampling import Constraints, LogitsParams, SamplingParams, sample_rows_host  # noqa: E402

CHUNK = 4
KINDS = {"bf16": dict(slots=40), "kv8": dict(slots=9, kv_cache="fp8"), "w4": dict(slots=9, llm_w4=True)}


class Rig:
    """test_gpu_token_select.Rig's few lines: the crafted decoder, one prompt whose last row is replaced by a row's start token, prefilled per slot"""

    def __init__(self, E, slots, **engine_kw):
        self.cfg = P.small()
        self.T, self.plan = P.build_table(self.cfg)
        self.max_new = P.max_new_for(self.cfg, self.plan)
        self.eng = TraceEngine(self.cfg, max_batch=slots, max_ctx=192, max_frames=4, max_new_tokens=self.max_new, **engine_kw)
        self.eng.retire_chunk = CHUNK
        self.eng.load_weights(P.crafted_weights(self.cfg, self.T).items())
        self.ts = E["timestamps"].tolist()
        self.eng.encode_video(synth.synth_frames(self.cfg, 0).to(torch.bfloat16), self.ts)
        self.L, emb = self.eng.splice(E["input_ids"].tolist(), want_output=True)
        self.emb = emb.clone()
        self.start = {}
        self.scale = P.logit_scale(self.cfg)

    def place(self, rows):
        for b, (start, _, _) in enumerate(rows):
            if self.start.get(b) != start:
                self.emb[-1] = P.embedding_row(self.cfg, start).to(self.emb.device)
                self.eng.prefill(b, self.L, embeds=self.emb)
                self.start[b] = start

    def decode(self, rows, eos, graph=True, retire=True, free=False, **kw):
        """eng.decode over the placed rows -> (ids, heads[, logprobs]), and what the call cost: (retires, rows x steps, _rows history)"""
        self.place(rows)
        eng = self.eng
        r0, s0 = eng.retires, eng.stats["decode_row_steps"]
        out = eng.decode(list(range(len(rows))), [h for _, h, _ in rows], self.max_new, eos, use_graph=graph,
                         forced=None if free else [f for _, _, f in rows], retire_finished=retire, **kw)
        return out, (eng.retires - r0, eng.stats["decode_row_steps"] - s0, [list(x) for x in eng._rows_history])

    def want(self, rows, eos):
        return P.restate_batch(self.T, self.cfg, rows, eos, self.max_new)


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


def ending_row(plan, r, at, max_new):
    """a teacher-forced row under head 0 that emits EOS at step `at` (None: never): filler states, row r's own rotation of them, the EOS emitter at `at`"""
    st = [plan.fillers[(3 * r + i) % len(plan.fillers)] for i in range(max_new + 1)]
    if at is not None:
        st[at] = plan.eos_emitter
    return (st[0], 0, st[1:])


def live_at(lengths, ids, eos, n_ids):
    """rows of a restatement that are unfinished once n_ids ids are recorded"""
    return [r for r, (n, x) in enumerate(zip(lengths, ids)) if not (n <= n_ids and x[n - 1] == eos)]


def check_exact(got, want, live, tag):
    ids, heads = got[0], got[1]
    assert ids == want[0], f"{tag}: rows {[r for r in range(len(ids)) if ids[r] != want[0][r]]} differ"
    assert [len(x) for x in ids] == want[1], tag
    assert [heads[r] for r in live] == [want[2][r] for r in live], f"{tag}: heads of the live rows"


# ---------------------------------------------------------------------------------------------------------------- 1: greedy and forced
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_eos_rows_equal_restate(rigs, graph):
    """rows that emit EOS at step 0, 1, the middle, the last step and never, and four more that never do: rows 0 and 1 leave after the first chunk,
    row 2 after the one that holds step 20, and the ids, lengths and live heads are the restatement's"""
    rig = rigs()
    mn = rig.max_new
    rows, fin = P.eos_rows(rig.cfg, rig.plan, P.EOS_BATCH, mn)
    want = rig.want(rows, rig.plan.eos)
    assert [want[1][r] for r in range(5)] == [1, 2, mn // 2 + 1, mn, mn]
    got, (retires, row_steps, hist) = rig.decode(rows, rig.plan.eos, graph)
    check_exact(got, want, hist[-1], f"eos rows, graph={graph}")
    assert retires >= 2 and [len(h) for h in hist] == [9, 7, 6] and hist[-1] == [3, 4, 5, 6, 7, 8]
    assert row_steps == CHUNK * 9 + 4 * CHUNK * 7 + 5 * CHUNK * 6 < 9 * (mn - 1)


# ---------------------------------------------------------------------------------------------------------------- 2: across the routes
def test_live_count_crosses_every_step_body(rigs):
    """40 -> 33 -> 17 -> 16 -> 1 rows at successive chunk boundaries: the wide step (and head_logits_kernel's second launch, 33 rows), the GEMV step at
    17 rows (the second 16-row half) and at 16, the fused step at 1.  Rows 0 and 39 stay through every retire but the last, row 20 (a teacher-forced
    tour row of batch_rows) to the end.  retire_fraction is raised on the instance so that the single row that ends in the third chunk leaves."""
    rig = rigs()
    cfg, plan, mn, eng = rig.cfg, rig.plan, rig.max_new, rig.eng
    B = 40
    assert [ops.decode_route(b, 0, cfg.hidden_size, cfg.intermediate_size, (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * 128)["step"]
            for b in (40, 33, 17, 16, 1)] == [3, 3, 1, 1, 2]
    rows = P.batch_rows(cfg, plan, B, mn)
    order = sorted((r for r in range(B) if r not in (0, 20, 39)), key=lambda r: (r * 7) % 37)      # the rows that end, spread over the batch
    ends = {}
    for i, r in enumerate(order[:7]):
        ends[r] = i % 5                                  # steps 0 .. 4: inside the first chunk (5 ids)
    for i, r in enumerate(order[7:23]):
        ends[r] = 5 + i % 4                              # steps 5 .. 8
    ends[order[23]] = 10                                 # steps 9 .. 12: one row
    for i, r in enumerate(order[24:] + [0, 39]):
        ends[r] = 13 + i % 4                             # steps 13 .. 16
    assert len(ends) == 39 and 20 not in ends
    for r, at in ends.items():
        rows[r] = ending_row(plan, r, at, mn)
    want = rig.want(rows, plan.eos)
    counts = [len(live_at(want[1], want[0], plan.eos, n)) for n in (1 + CHUNK, 1 + 2 * CHUNK, 1 + 3 * CHUNK, 1 + 4 * CHUNK)]
    assert counts == [33, 17, 16, 1] and want[1][20] == mn, counts        # on the restatement, before the device is touched
    eng.retire_fraction = 64
    try:
        got, (retires, row_steps, hist) = rig.decode(rows, plan.eos, True)
    finally:
        del eng.retire_fraction
    assert [len(h) for h in hist] == [40, 33, 17, 16, 1] and hist[-1] == [20] and all(0 in h and 39 in h for h in hist[:4])
    check_exact(got, want, [20], "40 -> 33 -> 17 -> 16 -> 1")
    assert row_steps == CHUNK * (40 + 33 + 17 + 16) + (mn - 1 - 4 * CHUNK) * 1


# ---------------------------------------------------------------------------------------------------------------- 3: sampled
def _host_draw(rig, state, head, step, index, sp):
    """the id sample_rows_host draws for the exact logits row of `state` under `head`, at Philox counter (step, index)"""
    V, Tv, Sv, NV, _ = P.dims(rig.cfg)
    lo, hi = P.head_range(rig.cfg, head)
    row = np.full(NV, -np.inf, np.float32)
    row[lo:hi] = rig.T[state, lo:hi].astype(np.float32) * np.float32(rig.scale)
    lg = np.repeat(row[None], index + 1, 0)
    return int(sample_rows_host(lg, [head] * (index + 1), V, Tv, Sv, sp, [step] * (index + 1))[index])


def _host_rows(rig, rows, eos, sp, index_of):
    """restate with the pick drawn on the host; index_of(r, step) = the Philox row index the draw uses"""
    V, Tv, _, _, _ = P.dims(rig.cfg)
    out = []
    for r, (state, head, forced) in enumerate(rows):
        ids, done = [], False
        for s in range(rig.max_new):
            tok = _host_draw(rig, state, head, s, index_of(r, s), sp)
            if not done:
                ids.append(tok)
            done = done or tok == eos
            feed = forced[s] if forced[s] >= 0 else tok
            head = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(feed, head)
            state = feed
        out.append(ids)
    return out


def test_sampled_rows_keep_their_philox_row(rigs):
    """Every state of every row is a flat head (all logits of the range equal): the draw is uniform over the range and depends on nothing but the
    Philox counter (seed, step, row index).  Rows 0, 3 and 6 (head 0) are fed the EOS emitter at steps 2, 6 and 10 and leave; the five others (the
    time head, no EOS among its ids) move to lower positions.  Retire on = retire off = the host's draws with the ORIGINAL row index, id for id —
    and the host's draws with the position a row moved to are different ids, so a sampler that took blockIdx.x would not pass."""
    rig = rigs()
    plan, mn, eos = rig.plan, rig.max_new, rig.plan.eos
    case = {c.name: c for c in plan.cases}
    f0, f1 = case["flat@0"].token, case["flat@1"].token
    sp = SamplingParams(1.0, 0, 1.0, 20261019)
    assert sp.on_device
    rows = []
    for r in range(8):
        if r % 3 == 0:
            st = [f0] * (mn + 1)
            st[{0: 2, 3: 6, 6: 10}[r]] = plan.eos_emitter
            rows.append((st[0], 0, st[1:]))
        else:
            rows.append((f1, 1, [f1] * mn))
    want = _host_rows(rig, rows, eos, sp, lambda r, s: r)
    final_pos = {r: p for p, r in enumerate([1, 2, 4, 5, 7])}
    moved = _host_rows(rig, rows, eos, sp, lambda r, s: final_pos.get(r, r) if s > 3 * CHUNK else r)
    for r in final_pos:                                   # two different row indices draw different ids, for every row that moves
        assert want[r] != moved[r] and len({tuple(want[q]) for q in final_pos}) == 5, r
    off, (n_off, _, _) = rig.decode(rows, eos, True, retire=False, sampling=sp)
    on, (n_on, row_steps, hist) = rig.decode(rows, eos, True, retire=True, sampling=sp)
    eager, _ = rig.decode(rows, eos, False, retire=True, sampling=sp)
    assert off[0] == want, [r for r in range(8) if off[0][r] != want[r]]
    assert on[0] == off[0] and eager[0] == off[0], [r for r in range(8) if on[0][r] != off[0][r]]
    assert n_off == 0 and n_on >= 2 and hist[-1] == [1, 2, 4, 5, 7] and [on[1][r] for r in hist[-1]] == [off[1][r] for r in hist[-1]]
    assert row_steps < 8 * (mn - 1)


# ---------------------------------------------------------------------------------------------------------------- 4: the entry point itself
def test_retire_rows_directly(rigs):
    rig = rigs()
    eng, mn = rig.eng, rig.max_new
    rows = P.batch_rows(rig.cfg, rig.plan, 6, mn)
    rig.place(rows)
    heads, forced = [h for _, h, _ in rows], [f for _, _, f in rows]

    def begin(n):
        eng.decode_begin(list(range(6)), heads, mn, eos=-1, forced=forced)
        eng.decode_steps(n)

    begin(mn - 1)
    full, full_heads = eng.decode_read()
    assert (full, full_heads) == (rig.want(rows, -1)[0], rig.want(rows, -1)[2])
    begin(3)
    r0 = eng.retires
    eng.retire_rows(range(6))                            # every row: a no-op
    assert eng.retires == r0 and eng._rows == [0, 1, 2, 3, 4, 5]
    for bad in ([4, 1], [1, 1], [0, 6], [-1, 2], [], [0, 1, 2, 3, 4, 5, 5]):
        with pytest.raises(_lib.TraceHipError):
            eng.retire_rows(bad)
        assert eng._rows == [0, 1, 2, 3, 4, 5] and eng._B == 6
    eng.retire_rows([1, 4, 5])                           # ... and after the errors the batch is as it was
    assert eng._rows == [1, 4, 5] and eng.retires == r0 + 1
    eng.decode_steps(5)
    eng.retire_rows([0, 2])
    assert eng._rows == [1, 5]
    eng.decode_steps(mn - 1 - 8, use_graph=False)
    ids, hd = eng.decode_read()
    assert ids == [full[1], full[5]] and hd == [full_heads[1], full_heads[5]]
    with pytest.raises(_lib.TraceHipError):              # max_new - 1 steps are taken: the bound of trace_decode_steps did not move
        eng.decode_steps(1)
    eng.host_mode(True)
    try:
        eng.decode_begin(list(range(6)), heads, mn, eos=-1, forced=forced)
        with pytest.raises(_lib.TraceHipError, match="host-select"):
            eng.retire_rows([0, 1])
    finally:
        eng.host_mode(False)
    with pytest.raises(ValueError):
        eng.decode_stepwise([0, 1], heads[:2], mn, retire_finished=True)
    with pytest.raises(ValueError):                      # top_k = 0 with top_p < 1: outside the device sampler's domain
        eng.decode([0, 1], heads[:2], mn, sampling=SamplingParams(1.0, 0, 0.5, 1), retire_finished=True)


# ---------------------------------------------------------------------------------------------------------------- 5: real arithmetic
NEW5 = 24


@pytest.fixture(scope="module")
def gauss():
    cfg = tcfg.tiny(num_frames=4)
    eng = TraceEngine(cfg, device=0, max_batch=6, max_ctx=192, max_frames=4, max_new_tokens=NEW5)
    eng.retire_chunk = CHUNK
    eng.load_weights(synth.state_dict(cfg).items())
    vids = [synth.synth_frames(cfg, i).to(torch.bfloat16).cuda() for i in range(6)]
    ts = [[[j * 2.5 + i] for j in range(4)] for i in range(6)]
    ids = [synth.synth_prompt_ids(cfg, n_text=24 + i, video_pos=10, seed=31 + i).tolist() for i in range(6)]
    yield cfg, eng, vids, ts, ids
    eng.close()


def _bound_check(on_lps, off_lps, alone_lps, full_lps, tag):
    """the check of part 5 on four sets of per-row log-probabilities: D from (off, alone), the sensitivity floor from the rows of `full`, then
    |on - off| <= 2 D.  Returns (D, observed)."""
    D = max(float(np.abs(a[:min(len(a), len(b))] - b[:min(len(a), len(b))]).max()) for a, b in zip(off_lps, alone_lps))
    floor = min(float(np.abs(full_lps[a][:n] - full_lps[b][:n]).max())
                for a in range(len(off_lps)) for b in range(a) for n in [min(len(off_lps[a]), len(off_lps[b]))])
    seen = max(float(np.abs(a[:min(len(a), len(b))] - b[:min(len(a), len(b))]).max()) for a, b in zip(on_lps, off_lps))
    print(f"{tag}: D (batch of 6 vs alone, retire off) = {D:.6f}, bound 2 D = {2 * D:.6f}, observed max |retire on - off| = {seen:.6f}, "
          f"smallest row-pair difference = {floor:.4f}")
    path = os.environ.get("TRACE_RETIRE_MEASURED")         # TRACE_RETIRE_MEASURED=FILE: the figures are appended to FILE (profiles/retire_ab.txt quotes them)
    if path:
        with open(path, "a") as fh:
            fh.write(f"{tag}: D = {D:.6f}, 2 D = {2 * D:.6f}, observed = {seen:.6f}, smallest row-pair difference = {floor:.4f}\n")
    assert D > 0 and floor >= 10 * (2 * D), f"{tag}: sensitivity floor {floor} < 20 D = {20 * D}: choose other prompts"
    assert seen <= 2 * D, f"{tag}: |retire on - off| = {seen} > 2 D = {2 * D}"
    return D, seen


def _real_rows(cfg, eng, vids, ts, ids, tag, **decode_kw):
    """Part 5 on an engine: six prompts, one forced continuation of time ids under the time head (so nothing that is fed can diverge), EOS = the
    time id that, on the retire-off run without EOS, ends the rows at the most different chunks.  Measured on the tiny Gaussian model (bf16):
    see profiles/retire_ab.txt."""
    V = cfg.vocab_size
    cont = [V + 2 + (5 * i) % 11 for i in range(NEW5)]              # time ids other than V + 1 (which would switch to the score head)
    shared = eng.encode_prefill(vids, ts, ids, 0)
    run = lambda slots, eos, retire: eng.decode(slots, [1] * len(slots), NEW5, eos, forced=[cont] * len(slots), logprobs=True, shared_prefix=shared if len(slots) > 1 else None,
                                                retire_finished=retire, **decode_kw)
    full = run(list(range(6)), -1, False)
    best = None
    for e in range(V + 1, V + 1 + cfg.time_vocab_size):
        end = [x.index(e) if e in x else None for x in full[0]]
        early = {n // CHUNK for n in end if n is not None and n < NEW5 - 1 - CHUNK}
        if all(n is None or n >= 2 for n in end) and (best is None or len(early) > best[0]):
            best = (len(early), e, end)
    assert best is not None and best[0] >= 2, f"{tag}: no EOS id ends these rows in two different chunks: choose other prompts ({best})"
    eos = best[1]
    off = run(list(range(6)), eos, False)
    alone = [run([b], eos, False) for b in range(6)]
    r0 = eng.retires
    on = run(list(range(6)), eos, True)
    on2 = run(list(range(6)), eos, True)
    assert eng.retires - r0 >= 4 and len({len(x) for x in off[0]}) >= 3, (best, eng.retires - r0, [len(x) for x in off[0]])
    assert on[0] == on2[0] and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(on[2], on2[2])), f"{tag}: two runs differ"
    assert [len(x) for x in on[0]] == [len(x) for x in off[0]], f"{tag}: lengths"
    return _bound_check(on[2], off[2], [a[2][0] for a in alone], full[2], tag)


def test_state_moves_with_the_row_on_real_weights(gauss):
    cfg, eng, vids, ts, ids = gauss
    _real_rows(cfg, eng, vids, ts, ids, "tiny Gaussian model, B = 6, 24 tokens")


# ---------------------------------------------------------------------------------------------------------------- 6: neighbours
@pytest.mark.parametrize("kind", ["kv8", "w4"])
def test_other_engines_on_the_exact_decoder(rigs, kind):
    """the e4m3 KV cache (its own append launch in every step) and w4 weights (the GEMV step at every size): deterministic, and the restatement"""
    rig = rigs(kind)
    rows, _ = P.eos_rows(rig.cfg, rig.plan, P.EOS_BATCH, rig.max_new)
    want = rig.want(rows, rig.plan.eos)
    a, (retires, _, hist) = rig.decode(rows, rig.plan.eos, True)
    b, _ = rig.decode(rows, rig.plan.eos, True)
    off, _ = rig.decode(rows, rig.plan.eos, True, retire=False)
    assert a == b and a[0] == off[0] and retires >= 2
    check_exact(a, want, hist[-1], kind)


def test_shared_prefix_down_to_one_row(rigs):
    """four prompts that agree on the 32 ids before <video>, prefilled once and attended from slot 0 (share_prefix_min_batch = 2 on the instance);
    rows 0, 1, 2 leave one chunk after the other — row 0 is the one whose slot holds the shared rows — and the last row decodes on unshared"""
    rig = rigs()
    cfg, plan, mn, eng = rig.cfg, rig.plan, rig.max_new, rig.eng
    rows = [ending_row(plan, r, at, mn) for r, at in enumerate([2, 6, 10, None])]
    base = synth.synth_prompt_ids(cfg, n_text=32 + 14, video_pos=32).tolist()
    vids = [synth.synth_frames(cfg, b).to(torch.bfloat16).cuda() for b in range(4)]
    ids = [base[:-1] + [start] for start, _, _ in rows]
    rig.start.clear()                                    # slots 0 .. 3 hold other prompts from here on
    eng.share_prefix_min_batch = 2
    try:
        shared = eng.encode_prefill(vids, [rig.ts] * 4, ids, 0)
    finally:
        del eng.share_prefix_min_batch
    assert shared == (0, 32)
    want = rig.want(rows, plan.eos)
    run = lambda retire: eng.decode(range(4), [0] * 4, mn, plan.eos, forced=[f for _, _, f in rows], shared_prefix=shared, retire_finished=retire)
    a = run(True)
    hist = [list(h) for h in eng._rows_history]
    b, off = run(True), run(False)
    assert [len(h) for h in hist] == [4, 3, 2, 1] and hist[-1] == [3]
    assert a == b and a[0] == off[0]
    check_exact(a, want, [3], "shared prefix")


def test_generate_stream_equals_generate(rigs):
    rig = rigs()
    cfg, plan, mn, eng = rig.cfg, rig.plan, rig.max_new, rig.eng
    base = synth.synth_prompt_ids(cfg, n_text=24, video_pos=10).tolist()
    batches = []
    for k, ats in enumerate(([2, None, 7], [None, 1, 11])):
        rows = [ending_row(plan, 3 * k + r, at, mn) for r, at in enumerate(ats)]
        vids = [synth.synth_frames(cfg, 3 * k + r).to(torch.bfloat16).cuda() for r in range(3)]
        batches.append((rows, (vids, [rig.ts] * 3, [base[:-1] + [s] for s, _, _ in rows], [0] * 3, [f for _, _, f in rows])))
    rig.start.clear()
    r0 = eng.retires
    got = list(eng.generate_stream([item for _, item in batches], mn, eos=plan.eos, retire_finished=True))
    assert eng.retires - r0 >= 4
    for (rows, item), g in zip(batches, got):
        ref = eng.generate(*item[:4], mn, eos=plan.eos, forced=item[4])
        live = [r for r in range(3) if plan.eos not in ref[0][r]]
        assert g[0] == ref[0] and [g[1][r] for r in live] == [ref[1][r] for r in live]
        check_exact(g, rig.want(rows, plan.eos), live, "generate_stream")
    rig.start.clear()


def test_processors_and_stop_sequences_move_with_the_row(rigs):
    """free rows along the chain, each from another point of it, under a repetition penalty and the two-id stop sequence (chain[9], chain[10]): a row
    ends once it has recorded both, so the match reads the row's recorded ids, the ones before the retires included.  Rows started at chain[6] and
    chain[8] leave after the first chunk, chain[2] and chain[4] after the second; the rows started at chain[9] and chain[10] have moved by then and
    still end where the chain says (chain[9]'s first id is chain[10] with nothing before it: it ends a cycle later)."""
    rig = rigs()
    plan, mn = rig.plan, rig.max_new
    n = len(plan.chain)
    starts = [0, 2, 4, 6, 8, 9, 10]
    rows = [(plan.chain[i][0], plan.chain[i][1], [-1] * mn) for i in starts]
    lens = [10 - i if i <= 8 else 10 - i + n for i in starts]
    want = [[plan.chain[(i + 1 + j) % n][0] for j in range(m)] for i, m in zip(starts, lens)]
    kw = dict(free=True, logits=LogitsParams(repetition_penalty=1.2), constraints=Constraints(stop_sequences=((plan.chain[9][0], plan.chain[10][0]),)))
    on, (retires, _, hist) = rig.decode(rows, -1, True, **kw)
    off, _ = rig.decode(rows, -1, True, retire=False, **kw)
    assert on[0] == want and off[0] == want
    assert retires == 2 and hist == [[0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 5, 6], [0, 5, 6]]


# ---------------------------------------------------------------------------------------------------------------- 7: the model
def test_model_generate(rigs):
    """free rows whose start tokens run into the EOS emitter after 1, 3, 6 and 7 ids, and two that never do: the padded tensor of retire_finished=True
    is the one of the default, and stopping_criteria= refuses the flag"""
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    rig = rigs()
    cfg, plan, mn, eng = rig.cfg, rig.plan, rig.max_new, rig.eng
    starts = [3, 305, 245, 104, 5, 218]
    rows = [(t, 0, [-1] * mn) for t in starts]
    want = rig.want(rows, plan.eos)
    assert want[1] == [mn, 1, 6, 3, mn, 7]
    base = synth.synth_prompt_ids(cfg, n_text=24, video_pos=10).tolist()
    ids = torch.tensor([base[:-1] + [t] for t in starts])
    vids = [synth.synth_frames(cfg, b).to(torch.bfloat16).cuda() for b in range(6)]
    m = TraceMistralForCausalLM(cfg, eng)
    kw = dict(images_or_videos=vids, video_timestamps=[rig.ts] * 6, max_new_tokens=mn, eos_token_id=plan.eos)
    rig.start.clear()
    off = m.generate(ids, heads=[0] * 6, **kw)
    r0 = eng.retires
    on = m.generate(ids, heads=[0] * 6, retire_finished=True, **kw)
    assert eng.retires - r0 == 2 and [len(h) for h in eng._rows_history] == [6, 4, 2]
    assert on.shape == off.shape == (6, mn) and torch.equal(on, off)
    assert [row[:n] for row, n in zip(on.tolist(), want[1])] == want[0]
    with pytest.raises(ValueError):
        m.generate(ids, heads=[0] * 6, retire_finished=True, stopping_criteria=[lambda i, s: torch.zeros(6, dtype=torch.bool)], **kw)
    rig.start.clear()
