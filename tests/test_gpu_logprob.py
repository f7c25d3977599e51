"""Per-token log-probabilities on the device (trace_amd/csrc/sample.h token_logprob_row): the loose-row op against the float32 restatement bit
for bit, the decode step's values (greedy / sampled, eager / graph replay, the setting toggled between batches) against the restatement applied
to that step's logits, the teacher-forced reference fixture, generate_samples against generate() of the repeated prompt, and the model /
pipeline / evaluate_videos surfaces."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine, ops  # noqa: E402
from trace_amd.sampling import LogitsParams, head_bounds, token_logprob_ref  # noqa: E402

GEOMS = [(32000, 13, 13), (320, 13, 13), (20, 3, 2)]          # TRACE-7B, the tiny config, a toy
LOGIT_TOL = 0.15                                              # the project's logit budget against the reference fixtures (test_gpu_parity.py)
SAMPLED = [SamplingParams(1.0, 50, 1.0, 2024), SamplingParams(0.7, 20, 0.8, 77)]


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _rows(B, V, Tv, Sv, rng, kind, scale):
    NV = V + 1 + Tv + Sv
    lg = np.full((B, NV), -np.inf, np.float32)
    heads = rng.randint(0, 3, size=B).astype(np.int32)
    for b in range(B):
        lo, hi = head_bounds(heads[b], V, Tv, Sv)
        x = (rng.randn(hi - lo) * scale).astype(np.float32)
        if kind == "ties" or (kind == "mixed" and b % 4 == 1):
            x = (np.round(x * 2) / 2).astype(np.float32)
        if kind == "flat" or (kind == "mixed" and b % 8 == 3):
            x[:] = np.float32(1.25)
        lg[b, lo:hi] = x
    return lg, heads


@pytest.mark.parametrize("geom", GEOMS)
def test_op_token_logprob_equals_restatement(geom):
    """np.array_equal on the float bits: no tolerance, no excluded rows; ids inside the head's range, at its arg-max, and outside it (-inf)"""
    V, Tv, Sv = geom
    NV = V + 1 + Tv + Sv
    rng = np.random.RandomState(sum(geom) + 5)
    total = 0
    for B, kind, scale in ((256, "mixed", 3.0), (48, "plain", 0.5), (48, "ties", 10.0), (7, "flat", 3.0), (1, "plain", 10.0)):
        lg, heads = _rows(B, V, Tv, Sv, rng, kind, scale)
        ids = np.zeros(B, np.int32)
        for b in range(B):
            lo, hi = head_bounds(heads[b], V, Tv, Sv)
            ids[b] = (rng.randint(lo, hi), lo + int(lg[b, lo:hi].argmax()), rng.randint(0, NV), hi - 1)[b % 4]
        got = ops.token_logprob(torch.from_numpy(lg).cuda(), torch.from_numpy(heads).cuda(), torch.from_numpy(ids).cuda(), V, Tv, Sv).cpu().numpy()
        want = np.zeros(B, np.float32)
        for b in range(B):
            lo, hi = head_bounds(heads[b], V, Tv, Sv)
            want[b] = token_logprob_ref(lg[b, lo:hi], int(ids[b]) - lo)
            if not lo <= ids[b] < hi:
                assert want[b] == -np.inf
        assert np.array_equal(_bits(got), _bits(want)), (geom, B, kind, np.nonzero(_bits(got) != _bits(want))[0][:8], got[:4], want[:4])
        total += B
    assert total >= 360
    out = ops.token_logprob(torch.from_numpy(lg).cuda(), [int(heads[0])], [int(ids[0])], V, Tv, Sv, element="f16").cpu().numpy()   # the fp16 library: same code
    assert np.array_equal(_bits(out), _bits(want[:1]))


# ---- the decode step ----
@pytest.fixture(scope="module")
def tiny():
    cfg = tcfg.tiny(num_frames=4)
    eng = _engine(cfg)
    vids = [synth.synth_frames(cfg, i).to(torch.bfloat16).cuda() for i in range(8)]
    ts = [[[j * 2.5] for j in range(4)] for _ in range(8)]
    ids = [synth.synth_prompt_ids(cfg, n_text=24, video_pos=10, seed=7 + i).tolist() for i in range(8)]
    yield cfg, eng, vids, ts, ids
    eng.close()


def _engine(cfg, **kw):
    eng = TraceEngine(cfg, device=0, max_batch=8, max_ctx=192, max_frames=4, max_new_tokens=24, **kw)
    eng.load_weights(synth.state_dict(cfg).items())
    return eng


def _stepwise(eng, cfg, vids, ts, ids, heads, n, sp):
    """eager steps with the masked logits of every step brought back (want_logits) and log-probabilities on:
    (ids, heads, logprobs per row, logits [n][B, NV])"""
    B = len(vids)
    eng.encode_prefill(vids, ts, ids, 0)
    eng.set_sampling(sp)
    eng.set_logprobs(True)
    try:
        lgs = [eng.decode_begin(list(range(B)), heads, n, eos=-1, want_logits=True).cpu().numpy()]
        for _ in range(n - 1):
            lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).cpu().numpy())
        out, hd = eng.decode_read()
        lp = eng.decode_read_logprobs([len(x) for x in out])
    finally:
        eng.set_logprobs(False)
        eng.set_sampling(None)
    return out, hd, lp, lgs


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_decode_logprobs_graph_eager_and_restatement(tiny, B, mode):
    cfg, eng, vids, ts, ids = tiny
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    sp = None if mode == 0 else SAMPLED[mode - 1]
    a = (vids[:B], ts[:B], ids[:B], [1] * B, 20)
    off, off_h = eng.generate(*a, sampling=sp, use_graph=True)
    g, gh, glp = eng.generate(*a, sampling=sp, use_graph=True, logprobs=True)
    e, eh, elp = eng.generate(*a, sampling=sp, use_graph=False, logprobs=True)
    assert g == off and gh == off_h                              # the setting changes no id (same seed for the sampled cases)
    assert e == g and eh == gh and _same_bits(glp, elp)          # graph replay == eager, ids and float bits
    s, sh, slp, lgs = _stepwise(eng, cfg, *a, sp)
    assert s == g and sh == gh and _same_bits(slp, glp)
    for b in range(B):
        assert len(glp[b]) == len(g[b]) == 20 and glp[b].dtype == np.float32
        h = 1
        for step, t in enumerate(g[b]):
            lo, hi = head_bounds(h, V, Tv, Sv)
            assert lo <= t < hi
            want = token_logprob_ref(lgs[step][b, lo:hi], t - lo)
            assert _bits(glp[b][step]) == _bits(want), (b, step, glp[b][step], want)
            assert np.isfinite(want) and want <= 0
            h = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(t, h)
    with pytest.raises(TraceHipError, match="without log-probabilities"):
        eng.decode_begin(list(range(B)), [1] * B, 4)
        eng.decode_read_logprobs()


def test_toggling_between_batches_equals_fresh_engines(tiny):
    """off -> on -> off -> on on one engine (graph replay: four cached forms of the step) against engines that only ever ran one form"""
    cfg, eng, vids, ts, ids = tiny
    for sp in (None, SAMPLED[0]):
        a = (vids[:3], ts[:3], ids[:3], [1] * 3, 16)
        seq = [eng.generate(*a, sampling=sp, logprobs=on) for on in (False, True, False, True)]
        f_off, f_on = _engine(cfg), _engine(cfg)
        try:
            want_off = f_off.generate(*a, sampling=sp)
            want_on = f_on.generate(*a, sampling=sp, logprobs=True)
        finally:
            f_off.close(); f_on.close()
        assert seq[0] == want_off and seq[2] == want_off and len(seq[0]) == 2
        for r in (seq[1], seq[3]):
            assert r[0] == want_on[0] and r[1] == want_on[1] and _same_bits(r[2], want_on[2])
        assert want_on[0] == want_off[0]


def test_all_eight_tail_modes_cycled_equal_fresh_engines(tiny):
    """sampling x log-probabilities x logits processors: one engine decodes 16 tokens at B = 3 in all eight modes, twice over, no two consecutive
    batches in one mode - the first visit captures the mode's graph, the second replays it after seven others were captured in between - and
    then B = 1 in the plain and the all-armed mode.  Every result against an engine that only ever ran that one mode: ids and heads equal,
    log-probabilities equal as float bits, the same seed everywhere.  A wrong index into the graph table or a buffer a mode misses shows here."""
    cfg, _, vids, ts, ids = tiny
    sp, lgp = SAMPLED[0], LogitsParams(1.5, 2, 0)

    def run(eng, mode, B):
        return eng.generate(vids[:B], ts[:B], ids[:B], [1] * B, 16, use_graph=True, sampling=sp if mode & 1 else None, logprobs=bool(mode & 2),
                            logits=lgp if mode & 4 else None)
    want = {}
    for mode in range(8):
        fresh = _engine(cfg)
        try:
            want[mode, 3] = run(fresh, mode, 3)
            if mode in (0, 7):
                want[mode, 1] = run(fresh, mode, 1)
        finally:
            fresh.close()
    assert want[0, 3][0] != want[1, 3][0] and want[0, 3][0] != want[4, 3][0] and want[1, 3][0] != want[5, 3][0]    # the modes are not one thing
    order = [0, 7, 1, 6, 2, 5, 3, 4]
    eng = _engine(cfg)
    try:
        for B, modes in ((3, order + order), (1, [0, 7, 0, 7])):
            assert all(a != b for a, b in zip(modes, modes[1:]))
            for visit, mode in enumerate(modes):
                got, w = run(eng, mode, B), want[mode, B]
                assert len(got) == len(w) == (3 if mode & 2 else 2), (B, visit, mode)
                assert got[0] == w[0] and got[1] == w[1], (B, visit, mode)
                assert all(len(r) == 16 for r in got[0])
                if mode & 2:
                    assert _same_bits(got[2], w[2]), (B, visit, mode)
    finally:
        eng.close()


def test_teacher_forced_logprobs_against_the_reference_fixture(golden_dir):
    """tests/golden/tiny_e2e.npz teacher-forced with its forced_ids: 49 steps over all three heads.  For EVERY step the device log-probability of
    the emitted id against the float64 log-softmax of the fixture's tf_logits at that same id: <= 2 LOGIT_TOL = 0.30 (the logit budget once on the
    chosen logit, once on log S).  No step is excluded."""
    cfg = tcfg.tiny(num_frames=4)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    eng = TraceEngine(cfg, max_batch=4, max_ctx=256, max_frames=4, max_new_tokens=64)
    try:
        eng.load_weights(synth.state_dict(cfg).items())
        forced = E["forced_ids"].tolist()
        n = len(forced) + 1
        eng.encode_video(synth.synth_frames(cfg, 0).to(torch.bfloat16), E["timestamps"].tolist())
        eng.prefill(1, eng.splice(E["input_ids"].tolist()))
        eng.set_logprobs(True)
        eng.decode_begin([1], [1], n, eos=-1, forced=[forced])
        eng.decode_steps(n - 1, use_graph=True)
        ids, _ = eng.decode_read()
        lp = eng.decode_read_logprobs([len(ids[0])])[0]
        eng.set_logprobs(False)
    finally:
        eng.close()
    ref = E["tf_logits"].astype(np.float64)
    assert len(ids[0]) == n == ref.shape[0] == 49
    worst, widths = 0.0, []
    for step, t in enumerate(ids[0]):
        fin = np.isfinite(ref[step])
        assert fin[t], f"step {step}: the emitted id {t} is outside the reference's head"
        x = ref[step][fin]
        want = ref[step][t] - x.max() - np.log(np.exp(x - x.max()).sum())
        d = abs(float(lp[step]) - want)
        print(f"step {step:2d} width {int(fin.sum()):3d} id {t:3d}: device {float(lp[step]):+.4f} reference {want:+.4f} diff {d:.4f}")
        worst = max(worst, d)
        widths.append(int(fin.sum()))
        assert d <= 2 * LOGIT_TOL, (step, float(lp[step]), want)
    assert widths.count(13) == 37 and widths.count(321) == 12
    print(f"worst |device - reference| over 49 steps: {worst:.4f}")


# ---- n ranked samples ----
# picked once: T = 1.0, top_k = 50, seed 2024 (SAMPLED[0]) — the tiny model's heads are flat enough that eight Philox rows of one prompt part ways
@pytest.mark.parametrize("use_graph", [True, False])
def test_generate_samples_equals_generate_of_the_repeated_prompt(tiny, use_graph):
    cfg, eng, vids, ts, ids = tiny
    sp = SAMPLED[0]
    want = eng.generate([vids[0]] * 8, [ts[0]] * 8, [ids[0]] * 8, [1] * 8, 20, sampling=sp, use_graph=use_graph, logprobs=True)
    got = eng.generate_samples(vids[0], ts[0], ids[0], 1, 8, 20, sampling=sp, use_graph=use_graph)
    assert got[0] == want[0] and got[1] == want[1] and _same_bits(got[2], want[2])
    assert len({tuple(r) for r in got[0]}) > 1, "the eight rows are all identical"
    with pytest.raises(ValueError):
        eng.generate_samples(vids[0], ts[0], ids[0], 1, 9, 20, sampling=sp)
    with pytest.raises(ValueError):
        eng.generate_samples(vids[0], ts[0], ids[0], 1, 8, 20, sampling=None)


def _model(cfg, eng):
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    return TraceMistralForCausalLM(cfg, eng)


def test_model_generate_samples_sorted(tiny):
    cfg, eng, vids, ts, ids = tiny
    m = _model(cfg, eng)
    kw = dict(images_or_videos=[vids[0]], video_timestamps=[ts[0]], n=8, heads=[1], max_new_tokens=20, temperature=1.0, top_k=50, eos_token_id=-1)
    torch.manual_seed(9)
    res = m.generate_samples(torch.tensor(ids[0]), **kw)
    torch.manual_seed(9)
    raw = m.generate_samples(torch.tensor(ids[0]), best_first=False, **kw)
    torch.manual_seed(9)
    sp = m._sampling_params(True, 1.0, 50, None, None, {})
    want = eng.generate_samples(vids[0], ts[0], ids[0], 1, 8, 20, sampling=sp)
    assert raw.order == list(range(8)) and raw.sequences.tolist() == want[0]
    assert np.array_equal(_bits(raw.logprobs.cpu().numpy()), _bits(np.stack(want[2])))
    scores = [float(np.sum(r, dtype=np.float64)) for r in want[2]]
    assert raw.scores.tolist() == scores
    assert res.order == sorted(range(8), key=lambda r: (-scores[r], r))
    assert all(res.scores[i] >= res.scores[i + 1] for i in range(7))
    for j, r in enumerate(res.order):                             # .order maps the sorted rows back to decode rows
        assert res.sequences[j].tolist() == want[0][r] and np.array_equal(_bits(res.logprobs[j].cpu().numpy()), _bits(want[2][r]))
        assert res.heads[j] == want[1][r]


# ---- model.generate(output_logprobs=True) on every path ----
def test_model_generate_output_logprobs_paths(tiny):
    cfg, eng, vids, ts, ids = tiny
    m = _model(cfg, eng)
    never = [lambda ids_, scores: torch.zeros(ids_.shape[0], dtype=torch.bool)]
    free = m.generate(torch.tensor(ids[:3]), images_or_videos=vids[:3], video_timestamps=ts[:3], heads=[1] * 3, max_new_tokens=20, eos_token_id=-1)
    eos = int(free[0, 6])                                          # a token row 0 emits at step 6: rows then stop at different lengths
    kw = dict(images_or_videos=vids[:3], video_timestamps=ts[:3], max_new_tokens=20, eos_token_id=eos, pad_token_id=0)
    plain = m.generate(torch.tensor(ids[:3]), heads=[1] * 3, **kw)
    main = m.generate(torch.tensor(ids[:3]), heads=[1] * 3, output_logprobs=True, **kw)
    step = m.generate(torch.tensor(ids[:3]), heads=[1] * 3, output_logprobs=True, stopping_criteria=never, **kw)
    step_plain = m.generate(torch.tensor(ids[:3]), heads=[1] * 3, stopping_criteria=never, **kw)
    assert isinstance(plain, torch.Tensor) and torch.equal(main.sequences, plain) and torch.equal(step.sequences, step_plain) and torch.equal(step_plain, plain)
    assert main.logprobs.dtype == torch.float32 and main.logprobs.shape == plain.shape
    assert np.array_equal(_bits(main.logprobs.cpu().numpy()), _bits(step.logprobs.cpu().numpy()))      # greedy: the paths agree bit for bit
    assert main.heads == step.heads
    lens = []
    for b in range(3):
        row = plain[b].tolist()
        n = row.index(eos) + 1 if eos in row else len(row)
        lens.append(n)
        assert (main.logprobs[b, :n] < 0).all() and (main.logprobs[b, n:] == 0).all()        # the EOS entry is included, zero past the length
    assert min(lens) < plain.shape[1], "no row stopped early: the padding was not exercised"
    # prefix-cached path, B = 1: a miss, then a hit (the same tensor object), against the cache being off
    one = dict(images_or_videos=[vids[0]], video_timestamps=[ts[0]], max_new_tokens=20, eos_token_id=eos, pad_token_id=0)
    base = m.generate(torch.tensor(ids[:1]), heads=[1], output_logprobs=True, **one)
    assert torch.equal(base.sequences[0], plain[0, : base.sequences.shape[1]])
    assert np.array_equal(_bits(base.logprobs[0].cpu().numpy()), _bits(main.logprobs[0, : base.logprobs.shape[1]].cpu().numpy()))
    m.enable_prefix_cache(True)
    try:
        rows0 = eng.stats["prefill_rows"]
        miss = m.generate(torch.tensor(ids[:1]), heads=[1], output_logprobs=True, **one)
        rows1 = eng.stats["prefill_rows"]
        hit = m.generate(torch.tensor(ids[:1]), heads=[1], output_logprobs=True, **one)
        rows2 = eng.stats["prefill_rows"]
        hit_plain = m.generate(torch.tensor(ids[:1]), heads=[1], **one)
    finally:
        m.enable_prefix_cache(False)
    assert rows2 - rows1 < rows1 - rows0, "the second call did not reuse the prefix"
    for r in (miss, hit):
        assert torch.equal(r.sequences, base.sequences) and np.array_equal(_bits(r.logprobs.cpu().numpy()), _bits(base.logprobs.cpu().numpy()))
    assert torch.equal(hit_plain, base.sequences)
    # the host-sampled fallback (top_k off with top_p < 1) and the sampled stepwise path: the values are those of the fed tokens
    torch.manual_seed(4)
    hs = m.generate(torch.tensor(ids[:2]), images_or_videos=vids[:2], video_timestamps=ts[:2], heads=[1, 1], max_new_tokens=10, eos_token_id=-1,
                    do_sample=True, top_k=0, top_p=0.7, output_logprobs=True)
    torch.manual_seed(4)
    hs_plain = m.generate(torch.tensor(ids[:2]), images_or_videos=vids[:2], video_timestamps=ts[:2], heads=[1, 1], max_new_tokens=10, eos_token_id=-1,
                          do_sample=True, top_k=0, top_p=0.7)
    assert torch.equal(hs.sequences, hs_plain) and bool((hs.logprobs < 0).all()) and bool(torch.isfinite(hs.logprobs).all())
    torch.manual_seed(6)
    dv = m.generate(torch.tensor(ids[:2]), images_or_videos=vids[:2], video_timestamps=ts[:2], heads=[1, 1], max_new_tokens=10, eos_token_id=-1,
                    do_sample=True, temperature=0.9, top_k=40, output_logprobs=True)
    torch.manual_seed(6)
    sw = m.generate(torch.tensor(ids[:2]), images_or_videos=vids[:2], video_timestamps=ts[:2], heads=[1, 1], max_new_tokens=10, eos_token_id=-1,
                    do_sample=True, temperature=0.9, top_k=40, output_logprobs=True, stopping_criteria=never)
    assert torch.equal(dv.sequences, sw.sequences) and np.array_equal(_bits(dv.logprobs.cpu().numpy()), _bits(sw.logprobs.cpu().numpy()))


def test_legacy_stc_path_output_logprobs():
    """the legacy trace.infer() flow (STC connector, no time tokens, text head only): greedy and sampled"""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), mm_projector_type="stc_connector", vision_image_size=84,
                              vision_hidden_size=256, vision_num_heads=4, mm_hidden_size=256)
    eng = TraceEngine(cfg, device=0, max_batch=1, max_ctx=256, max_frames=4, max_new_tokens=16)
    try:
        eng.load_weights(synth.state_dict(cfg).items())
        m = _model(cfg, eng)
        v = synth.synth_frames(cfg, 0).to(torch.bfloat16).cuda()
        ids = synth.synth_prompt_ids(cfg, n_text=16, video_pos=5).tolist()
        kw = dict(images_or_videos=[v], max_new_tokens=8, eos_token_id=-1)
        plain = m.generate(torch.tensor([ids]), **kw)
        res = m.generate(torch.tensor([ids]), output_logprobs=True, **kw)
        assert torch.equal(res.sequences, plain) and res.logprobs.shape == plain.shape
        assert bool((res.logprobs < 0).all()) and bool(torch.isfinite(res.logprobs).all())
        torch.manual_seed(2)
        sp = m.generate(torch.tensor([ids]), do_sample=True, temperature=1.0, **kw)
        torch.manual_seed(2)
        sl = m.generate(torch.tensor([ids]), do_sample=True, temperature=1.0, output_logprobs=True, **kw)
        assert torch.equal(sl.sequences, sp) and bool((sl.logprobs < 0).all())
    finally:
        eng.close()


# ---- pipeline and evaluate_videos ----
def test_generate_stream_logprobs_equals_generate(tiny):
    cfg, eng, vids, ts, ids = tiny
    for sp in (None, SAMPLED[1]):
        batches = [(vids[0:2], ts[0:2], ids[0:2], [1, 1], None), (vids[2:5], ts[2:5], ids[2:5], [1] * 3, None), (vids[5:8], ts[5:8], ids[5:8], [1] * 3, None)]
        got = list(eng.generate_stream(batches, 16, sampling=sp, logprobs=True))
        assert len(got) == 3
        for (v, t, i, h, _), (out, heads, lp) in zip(batches, got):
            want = eng.generate(v, t, i, h, 16, sampling=sp, logprobs=True)
            assert out == want[0] and heads == want[1] and _same_bits(lp, want[2])
        plain = list(eng.generate_stream(batches, 16, sampling=sp))
        assert [len(r) for r in plain] == [2, 2, 2] and [r[0] for r in plain] == [r[0] for r in got]


def test_evaluate_videos_carries_output_logprobs(tmp_path):
    from trace_amd import evaluate as ev
    from trace_amd.mm_utils import get_model_name_from_path
    from trace_amd.model.builder import load_pretrained_model, save_synthetic_checkpoint
    path = str(tmp_path / "trace-tiny")
    cfg = tcfg.tiny(num_frames=4)
    save_synthetic_checkpoint(path, cfg)
    tok, model, proc, _ = load_pretrained_model(path, None, get_model_name_from_path(path), max_batch=2, max_new_tokens=64)
    rng = np.random.RandomState(11)
    items = [{"id": f"v{i}", "video": rng.randint(0, 255, size=(30, 48, 64, 3), dtype=np.uint8), "fps": 10.0} for i in range(3)]
    orig = ev.build_prompt_ids

    def short_ids(q, t, conv_mode="llama_2"):                      # the byte-level stand-in tokenizer makes the llama_2 system prompt very long
        x = orig(q, tok)
        vp = int(torch.nonzero(x == -201)[0])
        return torch.cat([x[:1], x[vp - 20: vp + 20], x[-3:]])
    ev.build_prompt_ids = short_ids
    try:
        plain = ev.evaluate_videos(model, tok, proc, items, "find events", num_frames=4, max_new_tokens=10, batch_size=2)
        chunked = ev.evaluate_videos(model, tok, proc, items, "find events", num_frames=4, max_new_tokens=10, batch_size=2, logprobs=True)
        piped = ev.evaluate_videos(model, tok, proc, items, "find events", num_frames=4, max_new_tokens=10, batch_size=1, pipeline=True, logprobs=True)
        single = ev.evaluate_videos(model, tok, proc, items, "find events", num_frames=4, max_new_tokens=10, batch_size=1, pipeline=False, logprobs=True)
    finally:
        ev.build_prompt_ids = orig
        model.engine.close()
    assert all("output_logprobs" not in r for r in plain)
    for p, c, q, o in zip(plain, chunked, piped, single):
        assert c["output_ids"] == p["output_ids"] == q["output_ids"] == o["output_ids"]
        for r in (c, q, o):
            assert len(r["output_logprobs"]) == len(r["output_ids"]) > 0 and all(isinstance(v, float) and v < 0 for v in r["output_logprobs"])
        assert q["output_logprobs"] == o["output_logprobs"]           # pipelined == chunk by chunk at the same decode batch size, to the bit
        # (a chunk of two decodes with the batch-2 GEMV partition: the same ids, logits equal to within bf16 rounding, not to the bit)
        assert max(abs(x - y) for x, y in zip(c["output_logprobs"], o["output_logprobs"])) < 2 * LOGIT_TOL


def test_fp8_engine_smoke():
    """the shared head stage serves the fp8 weight path too: log-probabilities on change no id, graph replay == eager, values are log-probabilities"""
    cfg = tcfg.tiny(num_frames=4)
    eng = TraceEngine(cfg, device=0, max_batch=2, max_ctx=192, max_frames=4, max_new_tokens=16, llm_fp8=True)
    try:
        eng.load_weights(synth.state_dict(cfg).items())
        vids = [synth.synth_frames(cfg, i).to(torch.bfloat16).cuda() for i in range(2)]
        ts = [[[j * 2.5] for j in range(4)]] * 2
        ids = [synth.synth_prompt_ids(cfg, n_text=24, video_pos=10, seed=9 + i).tolist() for i in range(2)]
        off = eng.generate(vids, ts, ids, [1, 1], 12)
        g = eng.generate(vids, ts, ids, [1, 1], 12, logprobs=True, use_graph=True)
        e = eng.generate(vids, ts, ids, [1, 1], 12, logprobs=True, use_graph=False)
        assert g[0] == off[0] and g[1] == off[1] and e[0] == g[0] and _same_bits(g[2], e[2])
        assert all(len(r) == 12 and np.isfinite(r).all() and (r < 0).all() for r in g[2])
    finally:
        eng.close()
