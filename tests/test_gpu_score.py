"""Scoring given continuations on the device (trace_amd/csrc/score.hip, trace_llm_score_append, TraceEngine.score_continuations, model.score):
the loose-row op against the float32 restatement bit for bit on logits that are exact, against float64 on random weights, the teacher-forced
reference fixture, the decode path's own log-probabilities, group / padding invariance, the prefix cache, the e4m3 KV cache and the argument
errors.  The measured worst differences of the tolerance tests are kept in profiles/score_parity_measured.txt."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import token_select_probes as P  # noqa: E402
from trace_amd import config as tcfg, scoring, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402
from trace_amd.sampling import head_bounds, score_logprob_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_TOL = 0.15                                              # the project's logit budget against the reference fixtures (test_gpu_parity.py)
RECORD = os.path.join(ROOT, "profiles", "score_parity_measured.txt")
_recorded = []


def record(line):
    """the measured figures of this run, printed and kept in profiles/score_parity_measured.txt (rewritten from the run's first line on; a tree that
    cannot be written to only prints)"""
    print(line)
    _recorded.append(line)
    try:
        with open(RECORD, "w") as f:
            f.write("scoring parity as tests/test_gpu_score.py measured it (bounds: the tests' docstrings)\n")
            f.write("\n".join(_recorded) + "\n")
    except OSError:
        pass


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- 1. loose rows, exact logits ----
def _exact_rows(cfg, T, plan):
    """[(token whose one-hot row is the hidden row, head, target id)]: every named case of the table under its head with targets at the tied maxima,
    lo and hi - 1 (<sync> for the text head); for the text head the first and last column of column tiles (the second, a middle and the last tile);
    ignore (-1) and ids just outside the head (where the table holds decoys larger than every in-range value).  Heads interleave along the list."""
    V, Tv, Sv, NV, _ = P.dims(cfg)
    ct = ops.score_tile()
    per_head = {0: [], 1: [], 2: []}
    for c in plan.cases:
        lo, hi = P.head_range(cfg, c.head)
        tg = [c.ties[0], c.ties[-1], lo, hi - 1, -1, hi if hi < NV else lo - 1]
        if lo > 0:
            tg.append(lo - 1)
        if c.head == 0:
            last = (hi - 1) // ct
            tg += [ct - 1, ct, ct * (last // 2) - 1, ct * (last // 2), ct * last - 1, ct * last]
        per_head[c.head] += [(c.token, c.head, int(t)) for t in tg]
    rows, k = [], 0
    while any(per_head.values()):
        if per_head[k % 3]:
            rows.append(per_head[k % 3].pop(0))
        k += 1
    return rows


@pytest.mark.parametrize("element", ["bf16", "f16"])
@pytest.mark.parametrize("geom", ["small", "big"])
def test_op_score_rows_equals_restatement_on_exact_logits(geom, element):
    """trace_op_score_rows == score_logprob_ref on the float bits.  The head rows are token_select_probes' crafted table / 16 and every hidden row is
    s times a one-hot row, so a logit is ONE fp32 product s * T / 16 plus exact zeros: exact in any accumulation order, in the MFMA GEMM and in
    the time / score dot products alike.  R = 1, 33, 129 (one row more than the 128-row tile) and the whole list; V = 320 and V = 4499 (every
    head boundary and the last column tile mid-tile); heads mixed within each call; both element types."""
    cfg = P.GEOMETRIES[geom]()
    V, Tv, Sv, NV, _ = P.dims(cfg)
    T, plan = P.build_table(cfg)
    dtype = torch.bfloat16 if element == "bf16" else torch.float16
    W = (torch.from_numpy(T[:, :NV].astype(np.float32).T.copy()) / 16.0)            # [NV ids, NV tokens] -> place the tokens' columns
    toks = P.tokens_with_columns(cfg)
    cols = np.array([P.column(cfg, int(t)) for t in toks])
    Wh = torch.zeros((NV, P.HIDDEN), dtype=torch.float32)
    Wh[:, torch.from_numpy(cols)] = W[:, torch.from_numpy(toks)]
    Wd = Wh.to(dtype).cuda()
    assert torch.equal(Wd.float().cpu(), Wh), "the table / 16 is not exact in the element type"
    rows = _exact_rows(cfg, T, plan)
    assert len(rows) > 129 and {h for _, h, _ in rows[:33]} == {0, 1, 2}
    scales = (3.921875, 1.0, 0.5)
    checked = 0
    for R in (1, 33, 129, len(rows)):
        sub = rows[:R] if R > 1 else rows[3:4]
        X = torch.zeros((R, P.HIDDEN), dtype=torch.float32)
        want = np.zeros(R, np.float32)
        for r, (tok, h, t) in enumerate(sub):
            s = scales[r % 3]
            X[r, P.column(cfg, tok)] = s
            logits = (np.float32(s) * (T[tok, :NV].astype(np.float32) / np.float32(16.0))).astype(np.float32)
            lo, hi = head_bounds(h, V, Tv, Sv)
            want[r] = score_logprob_ref(logits, lo, hi, t)
        got = ops.score_rows(X.to(dtype).cuda(), Wd, [h for _, h, _ in sub], [t for _, _, t in sub], V, Tv, Sv, element=element).cpu().numpy()
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert len(bad) == 0, (geom, element, R, [(sub[i], got[i], want[i]) for i in bad[:6]])
        checked += R
        kinds = {("ignore" if t == -1 else "out" if not head_bounds(h, V, Tv, Sv)[0] <= t < head_bounds(h, V, Tv, Sv)[1] else "in") for _, h, t in sub}
        if R >= 33:
            assert kinds == {"ignore", "out", "in"} and (want[[t == -1 for _, _, t in sub]] == 0).all()
            assert np.isneginf(want[[k for k, (_, h, t) in enumerate(sub) if t != -1 and not head_bounds(h, V, Tv, Sv)[0] <= t < head_bounds(h, V, Tv, Sv)[1]]]).all()
    assert checked > 300


# ---- 2. loose rows, random weights ----
def test_op_score_rows_random_weights_against_float64():
    """K = 4096, V = 4499, 70 rows of mixed heads against float64 computed from the same 16-bit hidden rows and weights.  Bound, derived from the
    inputs before the device runs: an fp32 dot product of K terms accumulated in any order errs by at most K * 2^-24 * sum_k |x_k w_k| (the
    standard gamma_K bound; the bf16 x bf16 products themselves are exact in fp32); that enters once on the target logit and, as a weighted
    mean, once on log S: 2 * K * 2^-24 * max sum|x w|, plus 1e-4 for the restated sums (test_score_cpu.py's bound for a 36-tile head)."""
    V, Tv, Sv = 4499, 13, 13
    NV, K, R = V + 1 + Tv + Sv, 4096, 70
    g = torch.Generator().manual_seed(11)
    W = (torch.randn(NV, K, generator=g) * 0.02).to(torch.bfloat16)
    X = torch.randn(R, K, generator=g).to(torch.bfloat16)
    rng = np.random.RandomState(3)
    heads = [int(h) for h in rng.randint(0, 3, R)]
    ids = [int(rng.randint(*head_bounds(h, V, Tv, Sv))) for h in heads]
    ids[5], ids[6] = -1, (ids[6] + 2000) % NV if heads[6] else V + 3
    x64, w64 = X.double().numpy(), W.double().numpy()
    bound = 2 * K * 2.0 ** -24 * float((np.abs(x64) @ np.abs(w64).T).max()) + 1e-4
    lg = x64 @ w64.T
    got = ops.score_rows(X.cuda(), W.cuda(), heads, ids, V, Tv, Sv, element="bf16").cpu().numpy()
    worst = 0.0
    for r in range(R):
        lo, hi = head_bounds(heads[r], V, Tv, Sv)
        if ids[r] == -1:
            assert got[r] == 0.0
            continue
        if not lo <= ids[r] < hi:
            assert got[r] == -np.inf
            continue
        x = lg[r, lo:hi]
        want = lg[r, ids[r]] - x.max() - np.log(np.exp(x - x.max()).sum())
        worst = max(worst, abs(float(got[r]) - want))
    record(f"test 2 (random weights, K = 4096, V = 4499, 70 rows): worst |device - float64| = {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound


# ---- engines ----
def _engine(cfg, sd=None, **kw):
    eng = TraceEngine(cfg, device=0, max_batch=8, max_ctx=256, max_frames=4, max_new_tokens=64, **kw)
    eng.load_weights((sd or synth.state_dict(cfg)).items())
    return eng


@pytest.fixture(scope="module")
def tiny(golden_dir):
    cfg = tcfg.tiny(num_frames=4)
    eng = _engine(cfg)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16).cuda()
    yield cfg, eng, E, frames
    eng.close()


def _prompt_in_slot0(eng, E, frames):
    """the fixture's prompt: rows 0 .. P - 2 prefilled into slot 0 -> (P, the last prompt row's embedding)"""
    eng.encode_video(frames, E["timestamps"].tolist())
    L, emb = eng.splice(E["input_ids"].tolist(), want_output=True)
    emb = emb.clone()
    eng.prefill(0, L - 1, emb[: L - 1])
    return L, emb


def _reference_logprobs(E):
    ref, forced = E["tf_logits"].astype(np.float64), E["forced_ids"].tolist()
    want, widths = [], []
    for i, t in enumerate(forced):
        fin = np.isfinite(ref[i])
        assert fin[t]
        x = ref[i][fin]
        want.append(ref[i][t] - x.max() - np.log(np.exp(x - x.max()).sum()))
        widths.append(int(fin.sum()))
    return np.array(want), widths


# ---- 3. the reference fixture ----
def test_score_continuations_against_the_reference_fixture(tiny):
    """tests/golden/tiny_e2e.npz: score_continuations of forced_ids after the fixture's prompt.  All 48 entries within 2 LOGIT_TOL = 0.30 of the
    float64 log-softmax of tf_logits (the logit budget once on the chosen logit, once on log S: test_gpu_logprob.py's bound and reason); no entry
    excluded.  Also: the same rows through prefill(want_hidden) + score_rows give the same float bits (a row's bits do not depend on the cut)."""
    cfg, eng, E, frames = tiny
    forced = E["forced_ids"].tolist()
    L, emb = _prompt_in_slot0(eng, E, frames)
    rows0 = eng.stats["score_rows"]
    lps, chains, sums = eng.score_continuations(0, L, emb[L - 1], [forced], head=1)
    assert eng.stats["score_rows"] - rows0 == 48
    want, widths = _reference_logprobs(E)
    assert len(lps) == 1 and lps[0].dtype == np.float32 and len(lps[0]) == 48 == len(want)
    assert widths.count(13) == 36 and widths.count(321) == 12
    assert chains[0] == scoring.head_chain(cfg, forced, 1) and sums.dtype == np.float64 and sums[0] == np.sum(lps[0], dtype=np.float64)
    worst = 0.0
    for i in range(48):
        d = abs(float(lps[0][i]) - want[i])
        print(f"step {i:2d} width {widths[i]:3d} id {forced[i]:3d}: device {float(lps[0][i]):+.4f} reference {want[i]:+.4f} diff {d:.4f}")
        worst = max(worst, d)
    record(f"test 3 (tiny_e2e, 48 forced ids): worst |device - reference float64| = {worst:.4f}, bound {2 * LOGIT_TOL:.2f}")
    assert worst <= 2 * LOGIT_TOL
    fed = eng.embed_rows(*scoring.embed_placeholders(cfg, forced[:-1]), want_output=True)
    hid = eng.prefill(1, L + 47, torch.cat([emb, fed], 0), want_hidden=True)
    again = eng.score_rows(hid[L - 1:].contiguous(), chains[0], forced)
    assert np.array_equal(_bits(again), _bits(lps[0]))


# ---- 4. against the decode path ----
def test_score_of_the_ids_generate_emitted(tiny):
    """generate(output_logprobs=True) greedily at B = 1, then score() of the ids it emitted: per token |difference| <= 2 LOGIT_TOL = 0.30 (two 16-bit
    paths to the same logits — decode GEMVs over a cache against prefill GEMMs — each within the logit budget's half on the chosen logit and on
    log S), the heads equal."""
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    cfg, eng, E, frames = tiny
    m = TraceMistralForCausalLM(cfg, eng)
    ids = torch.from_numpy(E["input_ids"])
    kw = dict(images_or_videos=[frames], video_timestamps=[E["timestamps"].tolist()])
    gen = m.generate(ids, heads=[1], max_new_tokens=24, eos_token_id=-1, output_logprobs=True, **kw)
    out = gen.sequences[0].tolist()
    res = m.score(ids, continuations=[out], heads=[1], **kw)
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    assert len(res.logprobs[0]) == 24 and res.order == [0]
    for t, h in zip(out, res.heads[0]):
        lo, hi = head_bounds(h, V, Tv, Sv)
        assert lo <= t < hi                                       # the decode step drew every id from the head the chain names
    assert scoring.swap(cfg, out[-1], res.heads[0][-1]) == gen.heads[0]
    d = np.abs(res.logprobs[0].astype(np.float64) - gen.logprobs[0].cpu().numpy().astype(np.float64))
    record(f"test 4 (generate's own 24 ids re-scored): worst |score - decode logprob| = {d.max():.4f}, bound {2 * LOGIT_TOL:.2f}")
    assert d.max() <= 2 * LOGIT_TOL and np.isfinite(res.logprobs[0]).all() and (res.logprobs[0] <= 0).all()
    assert abs(res.scores[0] - float(np.sum(res.logprobs[0], dtype=np.float64))) == 0


# ---- 5. group invariance ----
def _continuations(cfg, n, seed=2):
    """n continuations of unequal length over all three heads (switch tokens included)"""
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    rng = np.random.RandomState(seed)
    out = []
    for b in range(n):
        c, h = [], 1
        for _ in range(3 + 5 * b + b % 3):
            lo, hi = head_bounds(h, V, Tv, Sv)
            t = int(rng.randint(lo, hi))
            if rng.rand() < 0.25:
                t = {0: V, 1: V + 1, 2: V + Tv + 1}[h]              # the id of this head that switches to the next one
            c.append(t)
            h = scoring.swap(cfg, t, h)
        out.append(c)
    return out


@pytest.mark.parametrize("n", [1, 3, 8])
def test_group_and_padding_invariance(tiny, n):
    """each continuation's floats are bit-identical alone and in a group of n (unequal lengths: the shorter ones are padded), under two padding ids,
    and from a second call"""
    cfg, eng, E, frames = tiny
    conts = _continuations(cfg, 8)[:n]
    assert len({len(c) for c in conts}) == n
    L, emb = _prompt_in_slot0(eng, E, frames)
    grp, chains, sums = eng.score_continuations(0, L, emb[L - 1], conts, head=1)
    assert all(np.isfinite(x).all() and len(x) == len(c) for x, c in zip(grp, conts))
    if n == 8:
        assert {h for ch in chains for h in ch} == {0, 1, 2}
    other, _, _ = eng.score_continuations(0, L, emb[L - 1], conts, head=1, pad_id=7)
    again, _, sums2 = eng.score_continuations(0, L, emb[L - 1], conts, head=1)
    assert _same_bits(grp, other) and _same_bits(grp, again) and np.array_equal(sums, sums2)
    for b, c in enumerate(conts):
        alone, ch, _ = eng.score_continuations(0, L, emb[L - 1], [c], head=1)
        assert np.array_equal(_bits(alone[0]), _bits(grp[b])) and ch[0] == chains[b], b
    if n == 8:                                                    # k > 1 trailing prompt rows handed in: the same bits (a row's bits do not depend on the cut)
        eng.prefill(0, L - 5, emb[: L - 5])
        tail, _, _ = eng.score_continuations(0, L, emb[L - 5:], conts, head=1)
        assert _same_bits(tail, grp)


# ---- 6. prefix cache ----
def test_model_score_with_the_prefix_cache(tiny):
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    cfg, eng, E, frames = tiny
    m = TraceMistralForCausalLM(cfg, eng)
    ids = torch.from_numpy(E["input_ids"])
    conts = _continuations(cfg, 4, seed=5)
    kw = dict(images_or_videos=[frames], video_timestamps=[E["timestamps"].tolist()])
    gkw = dict(heads=[1], max_new_tokens=12, eos_token_id=-1, **kw)
    base = m.score(ids, continuations=conts, **kw)
    gen0 = m.generate(ids, **gkw)
    m.enable_prefix_cache(True)
    try:
        st = eng.stats
        f0, r0 = st["vit_frames"], st["prefill_rows"]
        miss = m.score(ids, continuations=conts, **kw)
        f1, r1 = st["vit_frames"], st["prefill_rows"]
        hit = m.score(ids, continuations=conts, **kw)
        f2, r2 = st["vit_frames"], st["prefill_rows"]
        assert eng.prefix_entry() is not None, "score dropped the prefix entry"
        P0 = eng.prefix_entry()[1]
        gen1 = m.generate(ids, **gkw)
        f3 = st["vit_frames"]
    finally:
        m.enable_prefix_cache(False)
    suffix = len(E["input_ids"]) - 1 - int(np.nonzero(E["input_ids"] == -201)[0][0])
    Lrun = suffix - 1 + max(len(c) for c in conts)
    assert f1 - f0 == 4 and f2 == f1 and f3 == f2                 # one tower pass in all
    assert r1 - r0 == P0 + 4 * Lrun and r2 - r1 == 4 * Lrun       # the hit prefilled only the appended rows: four options, one append pass
    for r in (miss, hit):
        assert _same_bits(r.logprobs, base.logprobs) and r.heads == base.heads and r.order == base.order and np.array_equal(r.scores, base.scores)
    assert torch.equal(gen1, gen0)
    assert base.order == sorted(range(4), key=lambda b: (-base.scores[b], b))


# ---- 7. the e4m3 KV cache ----
def test_score_under_the_fp8_kv_cache(tiny):
    """kv_cache="fp8": finite, identical call to call, and every one of the 48 entries of test 3 within 1.08 of the reference.  The figure, derived
    before running: test_gpu_kv8_engine.py's budget for this depth (2 layers) is rms(2) = 1.3 * sqrt(2) * 0.036 * sqrt(2) * 1.5 = 0.140 and
    max = 4.5 * rms + LOGIT_TOL = 0.782 on a logit.  A log-probability errs by e_t - sum_i p_i e_i: the chosen logit's error (<= max) and a
    probability-weighted MEAN of the head's errors, which the 16-bit part of test 3's bound already allows at its maximum — so the e4m3 budget
    enters once, added to test 3's 2 LOGIT_TOL: 0.782 + 0.30 = 1.082."""
    cfg, _, E, frames = tiny
    rms = 1.3 * 2.0 ** 0.5 * 0.036 * 2.0 ** 0.5 * 1.5
    bound = 4.5 * rms + LOGIT_TOL + 2 * LOGIT_TOL
    assert abs(bound - 1.082) < 1e-3
    forced = E["forced_ids"].tolist()
    eng = _engine(cfg, kv_cache="fp8")
    try:
        L, emb = _prompt_in_slot0(eng, E, frames)
        a, chains, _ = eng.score_continuations(0, L, emb[L - 1], [forced, forced[:20]], head=1)
        b, _, _ = eng.score_continuations(0, L, emb[L - 1], [forced, forced[:20]], head=1)
    finally:
        eng.close()
    assert _same_bits(a, b) and all(np.isfinite(x).all() for x in a)
    want, _ = _reference_logprobs(E)
    worst = float(np.abs(a[0].astype(np.float64) - want).max())
    record(f"test 7 (kv_cache='fp8', tiny_e2e, 48 forced ids): worst |device - reference float64| = {worst:.4f}, bound {bound:.3f}")
    assert worst <= bound
    assert float(np.abs(a[1].astype(np.float64) - want[:20]).max()) <= bound


# ---- 8. argument errors ----
def test_score_append_argument_errors_come_before_any_launch(tiny):
    cfg, eng, E, frames = tiny
    NV = cfg.vocab_size + 1 + cfg.time_vocab_size + cfg.score_vocab_size
    L, emb = _prompt_in_slot0(eng, E, frames)
    eng.kv_copy(0, [1], L - 1)
    good, _, _ = eng.score_continuations(0, L, emb[L - 1], [[5, 6, 7]], head=0)
    eng.prefill(0, L - 1, emb[: L - 1])

    def lengths_unchanged():
        for slot, other in ((0, 2), (1, 3)):
            eng.kv_copy(slot, [other], L - 1)                     # the slot still holds exactly L - 1 rows
            with pytest.raises(TraceHipError, match="rows exceeds"):
                eng.kv_copy(slot, [other], L)

    lengths_unchanged()
    rows = torch.cat([emb[L - 1:], emb[:2]], 0).contiguous()
    ptr2 = (C.c_void_p * 2)(rows.data_ptr(), rows.data_ptr())
    out = (C.c_float * 64)()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    i32 = lambda xs: (C.c_int32 * len(xs))(*xs)
    call = lambda slot0, n, past, L_, hd, ii, ptrs=ptr2: eng.lib.trace_llm_score_append(eng.h, slot0, n, past, ptrs, L_, i32(hd), i32(ii), out, st)
    ok_h, ok_i = [0] * 6, [5, 6, 7] * 2
    for args, msg in (((0, 2, L - 1, 3, [0, 3, 0, 0, 0, 0], ok_i), "head must be"), ((0, 2, L - 1, 3, [0, -1, 0, 0, 0, 0], ok_i), "head must be"),
                      ((0, 2, L - 1, 3, ok_h, [5, -2, 7] * 2), "id must be"), ((0, 2, L - 1, 3, ok_h, [5, 6, NV] * 2), "id must be"),
                      ((0, 9, L - 1, 3, ok_h, ok_i), "bad slot"), ((7, 2, L - 1, 3, ok_h, ok_i), "bad slot"), ((0, 2, -1, 3, ok_h, ok_i), "bad L / past"),
                      ((0, 2, L - 1, 0, ok_h, ok_i), "bad L / past"), ((0, 2, 254, 3, ok_h, ok_i), "max_ctx"), ((0, 2, L, 3, ok_h, ok_i), "past exceeds"),
                      ((0, 2, L - 1, 3, ok_h, ok_i, None), "embeds may be NULL"), ((0, 2, L - 1, 3, ok_h, ok_i, (C.c_void_p * 2)(rows.data_ptr(), None)), "null embeds")):
        with pytest.raises(TraceHipError, match=msg):
            call(*args)
    lengths_unchanged()
    again, _, _ = eng.score_continuations(0, L, emb[L - 1], [[5, 6, 7]], head=0)
    assert np.array_equal(_bits(again[0]), _bits(good[0]))
    with pytest.raises(TraceHipError):                            # the loose op: K not a multiple of 64
        x = torch.zeros((2, 96), dtype=torch.bfloat16).cuda()
        w = torch.zeros((347, 96), dtype=torch.bfloat16).cuda()
        ops.score_rows(x, w, [0, 1], [1, 322], 320, 13, 13)
