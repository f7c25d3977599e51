"""Token selection on the device against exact answers: head_logits_kernel, select_next_kernel and trace_llm_head_logits.

Parts 1-3 run the identity-layer decoder of tests/token_select_probes.py: zero o_proj / down_proj, unit final norm, one-hot embeddings and head
rows T / 16 make the logit of id n after feeding token t exactly s * T[t][n] / 16, so every emitted id, every length and every head has one right
answer — P.restate, which tests/test_token_select_cpu.py holds up against the oracle and against ten broken selectors.  Every assertion is exact
equality: no tolerance, no near-tie exit.  Row b's prompt is the tiny_e2e.npz prompt with its last row replaced by the (one-hot) embedding of the
row's start token, prefilled into slot b; the attention output is multiplied by zero, so the video rows do not matter.

Part 4 holds trace_llm_head_logits against float64 on random head weights: one-hot hidden rows bit for bit, Gaussian rows inside the worst-case
bound of an fp32 sum in any order."""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import token_select_probes as P  # noqa: E402
from trace_amd import synth  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402
from trace_amd.sampling import token_logprob_ref  # noqa: E402

KINDS = {"bf16": dict(dtype=torch.bfloat16), "f16": dict(dtype=torch.float16), "fp8": dict(dtype=torch.bfloat16, llm_fp8="w8a8")}
SLOTS = {("small", "bf16"): 256, ("big", "bf16"): 100, ("small", "f16"): 17, ("small", "fp8"): 40}


class Rig:
    def __init__(self, geom, kind, E):
        self.geom, self.kind = geom, kind
        self.cfg = P.GEOMETRIES[geom]()
        self.T, self.plan = P.build_table(self.cfg)
        self.max_new = P.max_new_for(self.cfg, self.plan)
        self.dtype = KINDS[kind]["dtype"]
        self.eng = TraceEngine(self.cfg, max_batch=SLOTS[geom, kind], max_ctx=160, max_frames=4, max_new_tokens=self.max_new, **KINDS[kind])
        self.eng.load_weights(P.crafted_weights(self.cfg, self.T, self.dtype).items())
        self.eng.encode_video(synth.synth_frames(self.cfg, 0).to(self.dtype), E["timestamps"].tolist())
        self.L, emb = self.eng.splice(E["input_ids"].tolist(), want_output=True)
        self.emb = emb.clone()
        self.start = {}                     # slot -> the start token it was prefilled with
        self.scale = P.logit_scale(self.cfg, self.dtype)

    def place(self, rows):
        """slot b <- the prompt whose last row is row b's start token (kept from earlier batches where it is the same)"""
        for b, (start, _, _) in enumerate(rows):
            if self.start.get(b) != start:
                self.emb[-1] = P.embedding_row(self.cfg, start, self.dtype).to(self.emb.device)
                self.eng.prefill(b, self.L, embeds=self.emb)
                self.start[b] = start

    def run(self, rows, eos, graph):
        """(ids, lengths, heads) of the batch: decode_begin and max_new - 1 steps, replayed from the captured graph or eager one at a time"""
        self.place(rows)
        eng, mn = self.eng, self.max_new
        eng.decode_begin(list(range(len(rows))), [h for _, h, _ in rows], mn, eos=eos, forced=[f for _, _, f in rows])
        if graph:
            eng.decode_steps(mn - 1, use_graph=True)
        else:
            for _ in range(mn - 1):
                eng.decode_steps(1, use_graph=False)
        ids, heads = eng.decode_read()
        return ids, [len(x) for x in ids], heads

    def check(self, rows, eos, graph, tag):
        want = P.restate_batch(self.T, self.cfg, rows, eos, self.max_new)
        got = self.run(rows, eos, graph)
        if got != want:
            raise AssertionError(f"{tag}: " + self.explain(rows, eos, got, want))

    def explain(self, rows, eos, got, want):
        by_token = {(c.token, c.head): c.name for c in self.plan.cases}
        for b, (t, h, f) in enumerate(rows):
            if (got[0][b], got[1][b], got[2][b]) == (want[0][b], want[1][b], want[2][b]):
                continue
            tr = []
            P.restate(self.T, self.cfg, t, h, f, eos, self.max_new, trace=tr)
            g, w = got[0][b], want[0][b]
            s = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
            state, head, tok = tr[min(s, len(tr) - 1)]
            nbad = sum(1 for r in range(len(rows)) if (got[0][r], got[1][r], got[2][r]) != (want[0][r], want[1][r], want[2][r]))
            return (f"{nbad} of {len(rows)} rows differ; first: row {b} ({'free' if f[0] < 0 else 'forced'}) step {s}: state {state} under head {head} "
                    f"(case {by_token.get((state, head), '-')}) must emit {tok}, got {g[s] if s < len(g) else 'nothing'}; lengths {got[1][b]} / {want[1][b]}, "
                    f"final head {got[2][b]} / {want[2][b]}")
        return "?"


_rigs = {}


@pytest.fixture(scope="module")
def rigs(golden_dir):
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))

    def get(geom, kind="bf16"):
        if (geom, kind) not in _rigs:
            _rigs[geom, kind] = Rig(geom, kind, E)
        return _rigs[geom, kind]
    yield get
    for r in _rigs.values():
        r.eng.close()
    _rigs.clear()


# ---------------------------------------------------------------------------------------------------------------- 1: ids, lengths, heads
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("geom,B", [(g, B) for g in P.BATCHES for B in P.BATCHES[g]])
def test_batch_equals_restate(rigs, geom, B, graph):
    """B = 1 is the fused step, 17 fills the kernel's second 16 rows, 33 takes head_logits_kernel's second launch (and, from 32, the wide step); the
    rows start in different heads, so every tile sees rows it holds for and rows it does not.  big: 283 tiles — the strided loop, all 64 lanes
    and the cross-wave merge of select_next_kernel."""
    rig = rigs(geom)
    rig.check(P.batch_rows(rig.cfg, rig.plan, B, rig.max_new), -1, graph, f"{geom} B={B}")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("geom", list(P.BATCHES))
def test_eos_stops_a_row_and_nothing_else(rigs, geom, graph):
    """rows that emit EOS at step 0, 1, the middle, the last step and never: ids stop at and include EOS, lengths freeze, the head of a finished
    row keeps switching, and the other rows (teacher-forced and free) are what they are without EOS"""
    rig = rigs(geom)
    rows, fin = P.eos_rows(rig.cfg, rig.plan, P.EOS_BATCH, rig.max_new)
    want = P.restate_batch(rig.T, rig.cfg, rows, rig.plan.eos, rig.max_new)
    assert [want[1][r] for r in range(5)] == [1, 2, rig.max_new // 2 + 1, rig.max_new, rig.max_new]
    rig.check(rows, rig.plan.eos, graph, f"{geom} eos")


# ---------------------------------------------------------------------------------------------------------------- 2: the logits rows
@pytest.mark.parametrize("geom", list(P.BATCHES))
def test_logits_rows_are_scale_times_table_inside_the_head(rigs, geom):
    """want_logits at every step of a 33-row batch: finite exactly on the row's head range, and there s * T[state] / 16 bit for bit"""
    rig = rigs(geom)
    cfg, T, mn = rig.cfg, rig.T, rig.max_new
    NV = P.dims(cfg)[3]
    rows = P.batch_rows(cfg, rig.plan, 33, mn)
    traces = []
    for t, h, f in rows:
        traces.append([])
        P.restate(T, cfg, t, h, f, -1, mn, trace=traces[-1])
    rig.place(rows)
    eng = rig.eng
    lg = eng.decode_begin(list(range(33)), [h for _, h, _ in rows], mn, eos=-1, forced=[f for _, _, f in rows], want_logits=True)
    for s in range(mn):
        want = torch.full((33, NV), float("-inf"))
        for b in range(33):
            state, head, _ = traces[b][s]
            lo, hi = P.head_range(cfg, head)
            want[b, lo:hi] = torch.from_numpy(T[state, lo:hi].astype(np.float32)) * rig.scale
        got = lg.cpu()
        assert torch.equal(torch.isfinite(got), torch.isfinite(want)), f"step {s}: the finite pattern is not the head range"
        assert torch.equal(got, want), f"step {s}: rows {sorted(set(torch.nonzero(got != want)[:, 0].tolist()))[:8]}"
        if s < mn - 1:
            lg = eng.decode_steps(1, use_graph=False, want_logits=True)
    ids, heads = eng.decode_read()
    assert (ids, heads) == (P.restate_batch(T, cfg, rows, -1, mn)[0], P.restate_batch(T, cfg, rows, -1, mn)[2])


# ---------------------------------------------------------------------------------------------------------------- 3: the other callers
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_f16_library(rigs, graph):
    rig = rigs("small", "f16")
    rig.check(P.batch_rows(rig.cfg, rig.plan, 17, rig.max_new), -1, graph, "f16 B=17")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_fp8_w8a8(rigs, graph):
    """the fp8 GEMV step feeds the same selector (fp8 batches stop at 64 rows); the zero projections quantise to zero, the residual stays exact"""
    rig = rigs("small", "fp8")
    rig.check(P.batch_rows(rig.cfg, rig.plan, 40, rig.max_new), -1, graph, "fp8 B=40")


def test_gemv_step_at_40_rows(rigs):
    """decode.wide_min_rows = 65: 40 bf16 rows take the GEMV step instead of the wide one (eager: a graph captured for a batch size keeps its route)"""
    rig = rigs("small")
    assert ops.element == "bf16"
    with ops.tuned(decode__wide_min_rows=65):
        rig.check(P.batch_rows(rig.cfg, rig.plan, 40, rig.max_new), -1, False, "GEMV step B=40")


def test_host_select_mode(rigs):
    """B = 3, the host feeds designed tokens: the recorded ids are the fed ones, the heads follow the switch rule, and each step's logits have their
    lowest-id maximum where T says"""
    rig = rigs("small")
    cfg, T, mn, eng = rig.cfg, rig.T, rig.max_new, rig.eng
    V, Tv, Sv, NV, _ = P.dims(cfg)
    rows = P.batch_rows(cfg, rig.plan, 3, mn)
    rig.place(rows)
    state, head = [t for t, _, _ in rows], [h for _, h, _ in rows]
    fed = [[], [], []]
    eng.host_mode(True)
    try:
        lg = eng.decode_begin([0, 1, 2], head, mn, eos=-1, forced=None, want_logits=True)
        for s in range(mn):
            got = lg.cpu()
            for b in range(3):
                lo, hi = P.head_range(cfg, head[b])
                fin = torch.nonzero(torch.isfinite(got[b]))[:, 0]
                assert fin.tolist() == list(range(lo, hi)), (s, b)
                assert int(torch.nonzero(got[b] == got[b].max())[0]) == P.select(T[state[b]], lo, hi), (s, b, state[b], head[b])
            tok = [rows[b][2][s] for b in range(3)]
            eng.feed(tok)
            for b in range(3):
                fed[b].append(tok[b])
                head[b] = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(tok[b], head[b])
                state[b] = tok[b]
            ids, heads = eng.decode_read()
            assert ids == fed and heads == head, (s, ids, fed, heads, head)
            if s < mn - 1:
                lg = eng.decode_steps(1, use_graph=False, want_logits=True)
    finally:
        eng.host_mode(False)
    assert {h for b in range(3) for h in [rows[b][1]]} == {0, 1, 2}


def _stepwise_rows(rig):
    """B = 3 for decode_stepwise, one row per head, every row's first pick a tie case (so the host's pick has to be the lowest id of the range,
    inside the head, with larger decoys outside it).  Row 0 runs free under the time head; row 1 runs free under the text head except that step 2
    feeds the EOS emitter (step 3 then picks EOS); row 2, under the score head, is fed three more cases at steps 1, 3 and 5 and picks from each of
    them at the free step that follows (a forced step records the fed id, so only a free step shows the pick)."""
    plan, mn = rig.plan, rig.max_new
    case = {c.name: c for c in plan.cases}
    c0, c1, c2 = case["tie_same_tile@1"], case["tie3_tile_wave@0"], case["tie_same_tile@2"]
    assert all(len(c.ties) > 1 and c.decoys for c in (c0, c1, c2))
    f2 = [-1] * mn
    f2[1], f2[3], f2[5] = case["decoys@2"].token, case["all_negative@2"].token, case["tie3_tile_wave@2"].token
    return [(c0.token, 1, [-1] * mn), (c1.token, 0, [-1, -1, plan.eos_emitter] + [-1] * (mn - 3)), (c2.token, 2, f2)]


def _stepwise_want(rig, rows, eos):
    """P.restate_batch under host-select mode's one own rule (test_host_select_mode): the id recorded at a forced step is the fed one, not the pick.
    No row here is fed EOS, so lengths and heads are the restatement's as they are."""
    ids, lens, heads = P.restate_batch(rig.T, rig.cfg, rows, eos, rig.max_new)
    ids = [[f[s] if f[s] >= 0 else t for s, t in enumerate(x)] for x, (_, _, f) in zip(ids, rows)]
    return ids, lens, heads


@pytest.mark.parametrize("case", ["no_eos", "eos", "stopping", "logprobs"])
def test_decode_stepwise_equals_restate(rigs, case):
    """TraceEngine.decode_stepwise, greedy, on the identity-layer rig: the host's pick is the device's - the lowest id among equal maxima of the
    head's range, whatever lies outside it (every row starts at a tie case, row 2 is fed into three more).  Exact equality."""
    rig = rigs("small")
    cfg, T, mn, eng = rig.cfg, rig.T, rig.max_new, rig.eng
    rows = _stepwise_rows(rig)
    rig.place(rows)
    heads, forced = [h for _, h, _ in rows], [f for _, _, f in rows]
    eos = rig.plan.eos if case == "eos" else -1
    want = _stepwise_want(rig, rows, eos)
    named = {c.name: c for c in rig.plan.cases}
    assert [want[0][2][s] for s in (0, 2, 4, 6)] == [named[n + "@2"].expect for n in ("tie_same_tile", "decoys", "all_negative", "tie3_tile_wave")]
    assert want[0][0][0] == named["tie_same_tile@1"].expect and want[0][1][0] == named["tie3_tile_wave@0"].expect
    if case in ("no_eos", "eos"):
        ids, hd = eng.decode_stepwise([0, 1, 2], heads, mn, eos, forced=forced)
        assert (ids, [len(x) for x in ids], hd) == want
        assert want[1] == ([mn, 4, mn] if case == "eos" else [mn] * 3) and (case != "eos" or ids[1][-1] == eos)
    elif case == "stopping":
        calls = []

        def stop(cur):
            calls.append([len(x) for x in cur])
            return [False, len(cur[1]) >= 3, False]
        ids, hd = eng.decode_stepwise([0, 1, 2], heads, mn, -1, forced=forced, stopping=stop)
        assert ids == [want[0][0], want[0][1][:3], want[0][2]] and hd == want[2]       # (a stopped row is still fed: its head is the full run's)
        assert calls == [[s + 1] * 3 for s in range(mn - 1)]                           # asked after every step but the last, with the recorded ids
    else:
        ids, hd, lps = eng.decode_stepwise([0, 1, 2], heads, mn, -1, forced=forced, logprobs=True)
        assert (ids, [len(x) for x in ids], hd) == want
        n_inf = 0
        for b, (t, h, f) in enumerate(rows):
            tr = []
            P.restate(T, cfg, t, h, f, -1, mn, trace=tr)
            assert lps[b].dtype == np.float32 and len(lps[b]) == mn
            for s, (state, head, _) in enumerate(tr):
                lo, hi = P.head_range(cfg, head)
                raw = T[state, lo:hi].astype(np.float32) * np.float32(rig.scale)       # the raw row, bit for bit (test_logits_rows_are_scale_times_table)
                w = token_logprob_ref(raw, ids[b][s] - lo)
                assert np.float32(lps[b][s]).view(np.uint32) == np.float32(w).view(np.uint32), (b, s, lps[b][s], w)
                n_inf += int(np.isneginf(w))
        assert n_inf == 3 and all(np.isfinite(lps[b]).all() for b in (0, 1))           # row 2 is fed three text ids under the score head (-inf); picks never are
        dev = eng.decode([0, 1, 2], heads, mn, -1, use_graph=False, forced=[[-1] * mn, forced[1], [-1] * mn], logprobs=True)
        free = eng.decode_stepwise([0, 1, 2], heads, mn, -1, forced=[[-1] * mn, forced[1], [-1] * mn], logprobs=True)
        for b in (0, 2):                                                                # free rows: the device loop's ids, heads and float bits
            assert free[0][b] == dev[0][b] and free[1][b] == dev[1][b] and np.array_equal(free[2][b].view(np.uint32), dev[2][b].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 4: trace_llm_head_logits
HL_COLUMNS = [0, 7, 8, 15, 16, 63, 64, 511, 512, 2047, 2048, 4095] + [512 * w + 293 for w in range(8)]      # + one inside each wave's 512 columns
HL_ROWS = (1, 16, 17, 32, 33, 257)                                                                            # 257 crosses the 256-row loop


@pytest.fixture(scope="module")
def random_heads():
    cfg = P.small()
    sd = synth.state_dict(cfg)
    eng = TraceEngine(cfg, max_batch=1, max_ctx=128, max_frames=4, max_new_tokens=8)
    eng.load_weights(sd.items())
    W = torch.cat([sd["lm_head.weight"], sd["sync_head.weight"], sd["time_head.weight"], sd["score_head.weight"]])       # bf16 [NV, 4096]
    yield cfg, eng, W
    eng.close()


def _columns(R, head):
    """a different column for every row: the listed ones first (rotated by the head, so the short batches meet all of them), then others"""
    k = len(HL_COLUMNS)
    cols = [HL_COLUMNS[(i + 7 * head) % k] for i in range(min(R, k))]
    n = 5
    while len(cols) < R:
        n = (n + 61) % 4096
        if n not in cols:
            cols.append(n)
    assert len(set(cols)) == R
    return cols


@pytest.mark.parametrize("head", [0, 1, 2])
@pytest.mark.parametrize("R", HL_ROWS)
def test_head_logits_one_hot_rows_are_weight_columns(random_heads, R, head):
    """hidden row r is one-hot at column j_r: logits[r, n] is W[n, j_r] bit for bit inside the head (one product and exact zeros) and -inf outside;
    every row has its own column, so a row computed from another row's data shows"""
    cfg, eng, W = random_heads
    NV = P.dims(cfg)[3]
    cols = _columns(R, head)
    x = torch.zeros((R, cfg.hidden_size), dtype=torch.bfloat16)
    x[torch.arange(R), torch.tensor(cols)] = 1
    got = eng.head_logits(x.cuda().contiguous(), head).cpu()
    lo, hi = P.head_range(cfg, head)
    want = torch.full((R, NV), float("-inf"))
    want[:, lo:hi] = W[lo:hi].float()[:, cols].t()
    assert got.shape == want.shape
    assert torch.equal(got, want), f"rows {sorted(set(torch.nonzero(got != want)[:, 0].tolist()))[:8]}"


HL_K = 4096          # |got - ref| <= K 2^-23 sum |w_i x_i|: K - 1 = 4095 additions each rounded once is the worst case of ANY fp32 summation order
                     # (gamma_n ~ n u, u = 2^-24), with the unit doubled to 2^-23 because the MFMA's internal rounding is not documented as
                     # round-to-nearest.  Derived, not measured.


def test_head_logits_random_rows_vs_float64(random_heads):
    cfg, eng, W = random_heads
    NV = P.dims(cfg)[3]
    g = torch.Generator().manual_seed(11)
    x = torch.randn((33, cfg.hidden_size), generator=g).to(torch.bfloat16)
    ref = x.double() @ W.double().t()
    bound = HL_K * 2.0 ** -23 * (x.double().abs() @ W.double().abs().t())
    worst = 0.0
    for head in range(3):
        got = eng.head_logits(x.cuda().contiguous(), head).cpu()
        lo, hi = P.head_range(cfg, head)
        fin = torch.zeros((33, NV), dtype=torch.bool)
        fin[:, lo:hi] = True
        assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == float("-inf")).all()), f"head {head}: mask pattern"
        ratio = ((got.double() - ref).abs() / bound)[fin]
        worst = max(worst, float(ratio.max()))
        print(f"head {head}: largest |got - ref| / bound = {float(ratio.max()):.3e}")
        assert bool((ratio <= 1).all()), f"head {head}: {int((ratio > 1).sum())} elements outside the bound, worst ratio {float(ratio.max()):.3g}"
    # the figure goes where the other parity tests keep theirs: the parity_measured.txt of this run, in a directory beside tests/
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in glob.glob(os.path.join(root, "*", "parity_measured.txt")):
        with open(path, "a") as fh:
            fh.write(f"trace_llm_head_logits, 33 Gaussian bf16 rows, tiny heads vs float64: largest |err| / (4096 * 2^-23 * sum|w x|) = {worst:.3e}\n")
