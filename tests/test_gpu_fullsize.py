"""Full TRACE-7B geometry (BASELINE config 2: 128 frames x 336^2, prefill 1967, Mistral-7B + CLIP-ViT-L shapes, random-init
weights generated on the device).  The oracle cannot run this size in seconds, so parity is checked through
size-independent properties of the path: hipGraph replay == eager launches (bit-exact ids), a batch of two == each video
alone (paired prefill + batched decode vs single; logits within the bf16 budget, ids equal wherever the top-2 margin
exceeds it), the forced DVC feed walks the three heads, and finite logits with the reference's -inf head mask."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402

LOGIT_TOL = 0.15          # same budget as tests/test_gpu_parity.py


# The single-GPU BASELINE configurations at their full size (bench.py's CONFIGS): frames, text tokens, video position, tokens decoded,
# fp8 decoder projections.  C4's prompt shape: trace/eval/evaluate.py:298-357 + prompts/mr.txt; C5: trace/eval/videomme/evaluate.py:215-258.
FULL = {
    "c2": dict(frames=128, n_text=176, video_pos=150, n_new=24, fp8=False),          # L = 1967
    "c4": dict(frames=64, n_text=191, video_pos=150, n_new=32, fp8=False),           # L = 1086, the 14 + 4 + 14 moment-retrieval answer
    "c5": dict(frames=256, n_text=251, video_pos=200, n_new=16, fp8=False),          # L = 3834, past MAX_FRAMES
    "c5-fp8": dict(frames=256, n_text=251, video_pos=200, n_new=16, fp8=True),
}
# fp8 (W8A8 e4m3) vs bf16 engine at full depth: the a-priori budget of tests/test_gpu_fp8.py (FP8_*_TOL_FN) at 32 layers
from test_gpu_fp8 import fp8_budget  # noqa: E402


def _make(name):
    p = FULL[name]
    cfg = tcfg.trace_7b(p["frames"])
    ids = synth.synth_prompt_ids(cfg, n_text=p["n_text"], video_pos=p["video_pos"]).tolist()
    L = p["n_text"] - 1 + p["frames"] * cfg.tokens_per_frame
    eng = TraceEngine(cfg, max_batch=2, max_ctx=(L + 40 + 63) // 64 * 64, max_frames=p["frames"], max_new_tokens=32, llm_fp8=p["fp8"])
    eng.load_weights(synth.iter_weights(cfg, device="cuda:0"))
    vids = [synth.synth_frames(cfg, b, num_frames=p["frames"]).to(torch.bfloat16).cuda() for b in range(2)]
    ts = [[float(i)] for i in range(p["frames"])]
    return cfg, eng, ids, vids, ts, L


@pytest.fixture(scope="module", params=list(FULL))
def big(request):
    cfg, eng, ids, vids, ts, L = _make(request.param)
    assert L == {"c2": 1967, "c4": 1086, "c5": 3834, "c5-fp8": 3834}[request.param]
    eng.n_new = FULL[request.param]["n_new"]
    eng.tag = request.param
    yield cfg, eng, ids, vids, ts, L
    eng.close()


def _first_logits(eng, cfg, vids, ts, ids, slots):
    for k, b in enumerate(slots):
        eng.encode_video(vids[k], ts)
        eng.prefill(b, eng.splice(ids))
    return eng.decode_begin(slots, [1] * len(slots), eng.n_new, eos=-1, want_logits=True).float().cpu()


def test_graph_equals_eager_and_lengths(big):
    cfg, eng, ids, vids, ts, L = big
    n = eng.n_new
    assert eng.splice(ids) if eng.encode_video(vids[0], ts) is None else True
    a, _ = eng.generate(vids[:1], [ts], [ids], [1], n, eos=-1, use_graph=False)
    b, _ = eng.generate(vids[:1], [ts], [ids], [1], n, eos=-1, use_graph=True)
    assert a == b and len(a[0]) == n
    V = cfg.vocab_size
    assert all(0 <= t < cfg.total_vocab for t in a[0])
    assert V + 1 <= a[0][0] <= V + cfg.time_vocab_size          # heads=[1]: the first token comes from the time head


def test_prefill_last_rows_shortcut_bit_identical_at_full_size(big):
    """the last decoder layer over the last rows only (round 6) vs over all rows, at the configurations' real prompt lengths and widths: first logits and
    the next decode steps bit-identical (bf16 path; the fp8 context keeps the full layer)"""
    from trace_amd.engine import ops
    cfg, eng, ids, vids, ts, L = big
    if eng.llm_fp8:
        pytest.skip("the fp8 weight path runs the full last layer")
    eng.encode_video(vids[0], ts)
    _, e0 = eng.splice(ids, want_output=True)
    e0 = e0.clone()
    eng.encode_video(vids[1], ts)
    _, e1 = eng.splice(ids, want_output=True)
    e1 = e1.clone()
    res = {}
    for mode in (0, 1):
        with ops.tuned(prefill__last_rows=mode):
            eng.prefill_pair(0, e0, e1)
            lg = [eng.decode_begin([0, 1], [1, 1], eng.n_new, eos=-1, want_logits=True).clone()]
            for _ in range(2):
                lg.append(eng.decode_steps(1, use_graph=False, want_logits=True).clone())
            res[mode] = torch.stack(lg)
    assert torch.equal(res[0], res[1]), f"max |d| {(res[0] - res[1])[torch.isfinite(res[0])].abs().max().item()}"


def test_pair_equals_single(big):
    cfg, eng, ids, vids, ts, L = big
    n = eng.n_new
    tol = fp8_budget(cfg.num_hidden_layers)[0] if eng.llm_fp8 else LOGIT_TOL     # (the pair / single GEMMs quantise the same rows: in practice far inside)
    single, margins, solo = [], [], []
    for k in range(2):                             # each video alone, free-running, with every step's logits: step-0 logits + the top-2 margins
        lg0 = _first_logits(eng, cfg, [vids[k]], ts, ids, [0])
        lgs = [lg0[0]] + [eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu()[0] for _ in range(n - 1)]
        single.append(lg0)
        solo.append(eng.decode_read()[0][0])
        top = [torch.topk(torch.where(torch.isfinite(x), x, torch.full_like(x, -1e30)), 2).values for x in lgs]
        margins.append([float(t[0] - t[1]) for t in top])
    a, b = [solo[0]], [solo[1]]
    ab, _ = eng.generate(vids, [ts, ts], [ids, ids], [1, 1], n, eos=-1)          # paired prefill, batch-2 decode
    # step-0 logits of the pair path (prefill_pair) vs the single path
    emb = []
    for k in range(2):
        eng.encode_video(vids[k], ts)
        emb.append(eng.splice(ids, want_output=True)[1].clone())
    eng.prefill_pair(0, emb[0], emb[1])
    lp = eng.decode_begin([0, 1], [1, 1], n, eos=-1, want_logits=True).float().cpu()
    for k in range(2):
        fin = torch.isfinite(single[k][0])
        assert torch.equal(torch.isfinite(lp[k]), fin) and int(fin.sum()) == cfg.time_vocab_size     # -inf outside the time head
        assert (lp[k][fin] - single[k][0][fin]).abs().max().item() < tol
    for got, ref, mg in ((ab[0], a[0], margins[0]), (ab[1], b[0], margins[1])):
        # greedy streams may part only at a near-tie of the run they are compared with (batch 1 and batch 2 sum in different orders): equal ids up
        # to the first step whose own top-2 margin is inside twice the logit budget
        for i, (x, y) in enumerate(zip(got, ref)):
            if mg[i] < 2 * tol:
                break
            assert x == y, (i, mg[i], got, ref)


def test_forced_feed_walks_heads(big):
    """c2 / c5: one dense-captioning event (14 time-, 4 score-head steps, text, text <sync>); c4: the moment-retrieval answer
    (14 + 4 + 14).  The arg-max of every step must come from the head the feed implies."""
    cfg, eng, ids, vids, ts, L = big
    V, Tv = cfg.vocab_size, cfg.time_vocab_size
    n_text = 13 if eng.tag == "c4" else 5 if eng.tag == "c2" else 0
    feed = ([V + 3] * 6 + [V + 2] + [V + 4] * 6 + [V + 1]            # 14 time-head steps, time <sync> -> score head
            + [V + Tv + 3, V + Tv + 13, V + Tv + 5, V + Tv + 1])       # 4 score-head steps, score <sync> -> text head
    feed = (feed + [17, 23, 99, 1234, 7, 8, 9, 10, 11, 12, 13, 14, 15][:n_text - 1] + [V] if n_text else feed[:eng.n_new])   # text, text <sync> -> time head
    feed = feed[:eng.n_new] if eng.tag != "c2" else feed
    out, heads = eng.generate(vids[:1], [ts], [ids], [1], len(feed), eos=-1, forced=[feed])
    last = feed[-1]
    assert heads[0] == (1 if last == V else 2 if last == V + 1 else 0 if last == V + Tv + 1 else heads[0]) and len(out[0]) == len(feed)
    for step, tok in enumerate(out[0]):                                # the arg-max at each step came from the head the feed implies
        if step < 14:
            assert V + 1 <= tok <= V + Tv
        elif step < 18:
            assert V + Tv + 1 <= tok <= V + 2 * Tv
        else:
            assert 0 <= tok <= V


def test_bit_reproducible(big):
    """Same inputs -> the same bits, run after run: video rows, prefill hidden states and decode logits (every reduction in
    the path has a fixed order; an LDS float-atomic combine in the slot pool once broke this by one ulp per run)."""
    cfg, eng, ids, vids, ts, L = big
    enc = [eng.encode_video(vids[0], ts, want_output=True).clone() for _ in range(2)]
    assert torch.equal(enc[0], enc[1])
    hid, lg = [], []
    for _ in range(2):
        eng.encode_video(vids[0], ts)
        hid.append(eng.prefill(0, eng.splice(ids), want_hidden=True)[-8:].clone())
        steps = [eng.decode_begin([0], [1], 8, eos=-1, want_logits=True).clone()]
        for _s in range(5):
            steps.append(eng.decode_steps(1, use_graph=False, want_logits=True).clone())
        lg.append(torch.stack(steps))
    assert torch.equal(hid[0], hid[1])
    assert torch.equal(lg[0], lg[1])


def test_c5_fp8_tracks_bf16_at_full_depth():
    """BASELINE config 5 at its full size, 32 layers: the fp8 engine's teacher-forced logits against the bf16 engine's on the same
    video and feed, inside the a-priori fp8 budget (tests/test_gpu_fp8.py: fp8_budget), plus the fraction of 13-way time / score
    arg-max decisions that flip — written to parity_measured.txt."""
    import os
    res, toks = {}, {}
    V, Tv = None, None
    for name in ("c5", "c5-fp8"):
        cfg, eng, ids, vids, ts, L = _make(name)
        V, Tv = cfg.vocab_size, cfg.time_vocab_size
        feed = ([V + 3, V + 5, V + 7, V + 4, V + 13, V + 9, V + 2, V + 6, V + 3, V + 8, V + 5, V + 13, V + 4, V + 1]
                + [V + Tv + 6, V + Tv + 13])
        eng.encode_video(vids[0], ts)
        eng.prefill(0, eng.splice(ids))
        lg = [eng.decode_begin([0], [1], 16, eos=-1, forced=[feed], want_logits=True).float().cpu()[0]]
        for _ in range(15):
            lg.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu()[0])
        res[name] = torch.stack(lg)
        toks[name] = eng.decode_read()[0][0]
        eng.close()
    fin = torch.isfinite(res["c5"])
    assert torch.equal(fin, torch.isfinite(res["c5-fp8"]))
    d = (res["c5-fp8"][fin] - res["c5"][fin])
    worst, rms, std = d.abs().max().item(), d.pow(2).mean().sqrt().item(), res["c5"][fin].std().item()
    flips = sum(int(a != b) for a, b in zip(toks["c5"], toks["c5-fp8"]))
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "parity_measured.txt"), "a") as f:
            f.write(f"C5 full size (256 frames, L=3834, 32 layers), fp8 vs bf16 engine, 16 teacher-forced 13-way steps: max |dlogit| = {worst:.4f}, "
                    f"rms = {rms:.4f}, logit std {std:.3f}, arg-max flips {flips}/16\n")
    mx, rm = fp8_budget(32)
    assert worst < mx and rms < rm, (worst, rms)


def test_batch_40_equals_singles():
    """40 different videos decoded together (four 16-row MFMA groups, K cut in 4-16 chunks of partial rows, second head pass,
    paired prefill) vs three of them decoded alone: step-0 logits within the bf16 budget, greedy ids equal up to the first
    near-tie (the k-chunk partition, hence the fp32 rounding, depends on the batch size)."""
    cfg = tcfg.trace_7b(128)
    ids = synth.synth_prompt_ids(cfg, n_text=176, video_pos=150).tolist()
    L = 176 - 1 + 128 * cfg.tokens_per_frame
    nb, n_new = 40, 16
    eng = TraceEngine(cfg, max_batch=nb, max_ctx=(L + n_new + 63) // 64 * 64, max_frames=128, max_new_tokens=n_new)
    eng.load_weights(synth.iter_weights(cfg, device="cuda:0"))
    ts = [[float(i)] for i in range(128)]
    vids = [synth.synth_frames(cfg, 100 + b, num_frames=128).to(torch.bfloat16).cuda() for b in range(nb)]
    out, _ = eng.generate(vids, [ts] * nb, [ids] * nb, [1] * nb, n_new, eos=-1)
    # the tower ran over the batch's frame stream 170 frames at a time (whole GEMM rounds): same features as one video alone
    assert eng.vit_batch_frames == 170
    many = eng.vit_forward_many(vids[:3])              # 384 frames = 170 + 170 + 44, every chunk spans a video boundary
    for b in range(3):
        assert torch.equal(many[b], eng.vit_forward(vids[b]))
    del many
    # step-0 logits of the whole batch (all slots are still prefilled)
    lgb = eng.decode_begin(list(range(nb)), [1] * nb, n_new, eos=-1, want_logits=True).float().cpu()
    for b in (0, 17, 39):
        eng.encode_video(vids[b], ts)
        eng.prefill(0, eng.splice(ids))
        lg1 = eng.decode_begin([0], [1], n_new, eos=-1, want_logits=True).float().cpu()[0]
        fin = torch.isfinite(lg1)
        assert torch.equal(torch.isfinite(lgb[b]), fin)
        if b != 0:           # slot 0 was just overwritten by this video's prefill; the batch logits of slot 0 were read before
            assert (lgb[b][fin] - lg1[fin]).abs().max().item() < LOGIT_TOL
        # free-running ids: equal until the single run's own top-2 margin drops inside the logit budget (after a near-tie the two
        # runs may legitimately follow different tokens)
        lgs = [lg1] + [eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu()[0] for _ in range(n_new - 1)]
        single, _ = eng.decode_read()
        for i in range(n_new):
            top = torch.topk(torch.where(torch.isfinite(lgs[i]), lgs[i], torch.full_like(lgs[i], -1e30)), 2).values
            if float(top[0] - top[1]) < 2 * LOGIT_TOL:
                break
            assert out[b][i] == single[0][i], (b, i, out[b], single[0])
    eng.close()


def test_batch_128_equals_singles():
    """The bench's own shape at full geometry (round-3 review: the largest full-size batch-vs-singles check was 40): 128 different 128-frame videos
    through generate() — 170-frame tower stream across video boundaries, prefill in runs of four, the WIDE decode step (small-M MFMA GEMMs, split-K
    partial rows, two head passes) through all 32 layers at ctx ~ 2000 — against rows 0 / 63 / 127 decoded alone (batch-1 fused-norm GEMV path) in a
    spare KV slot: step-0 logits within 0.15, free-running greedy ids equal up to the single run's first near-tie."""
    cfg = tcfg.trace_7b(128)
    ids = synth.synth_prompt_ids(cfg, n_text=176, video_pos=150).tolist()
    L = 176 - 1 + 128 * cfg.tokens_per_frame
    nb, n_new = 128, 24
    eng = TraceEngine(cfg, max_batch=nb + 1, max_ctx=(L + n_new + 63) // 64 * 64, max_frames=128, max_new_tokens=n_new)
    eng.load_weights(synth.iter_weights(cfg, device="cuda:0"))
    ts = [[float(i)] for i in range(128)]
    vids = [synth.synth_frames(cfg, 300 + b, num_frames=128).to(torch.bfloat16).cuda() for b in range(nb)]
    out, heads = eng.generate(vids, [ts] * nb, [ids] * nb, [1] * nb, n_new, eos=-1)
    assert len(out) == nb and all(len(o) == n_new for o in out) and all(h in (0, 1, 2) for h in heads)
    lgb = eng.decode_begin(list(range(nb)), [1] * nb, n_new, eos=-1, want_logits=True).float().cpu()      # step-0 logits of the whole batch
    checked = 0
    for b in (0, 63, 127):
        eng.encode_video(vids[b], ts)
        eng.prefill(nb, eng.splice(ids))                                   # the spare slot: the batch's slots stay as generate() left them
        lg1 = eng.decode_begin([nb], [1], n_new, eos=-1, want_logits=True).float().cpu()[0]
        fin = torch.isfinite(lg1)
        assert torch.equal(torch.isfinite(lgb[b]), fin)
        err = (lgb[b][fin] - lg1[fin]).abs().max().item()
        assert err < LOGIT_TOL, (b, err)
        lgs = [lg1] + [eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu()[0] for _ in range(n_new - 1)]
        single, _ = eng.decode_read()
        for i in range(n_new):
            top = torch.topk(torch.where(torch.isfinite(lgs[i]), lgs[i], torch.full_like(lgs[i], -1e30)), 2).values
            if float(top[0] - top[1]) < 2 * LOGIT_TOL:
                break
            assert out[b][i] == single[0][i], (b, i, out[b], single[0])
            checked += 1
    assert checked >= 3, checked                                           # (random-weight logits: a near-tie usually arrives within a few tokens; 5 measured)
    eng.close()
