"""Device sampling (trace_amd/csrc/sample.h): trace_op_sample against the float32 restatement (trace_amd/sampling.py) and HF's warpers, and
generate(do_sample=True) end to end on the tiny synthetic model — graph replay, eager steps, the stepwise path and the pipeline agree."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine, ops  # noqa: E402
from trace_amd.sampling import head_bounds, philox_uniform, sample_row_ref  # noqa: E402

GEOMS = [(32000, 13, 13), (320, 13, 13), (20, 3, 2)]          # TRACE-7B, the tiny config, a toy


def _rows(B, V, Tv, Sv, rng, kind):
    NV = V + 1 + Tv + Sv
    lg = np.full((B, NV), -np.inf, np.float32)
    heads = rng.randint(0, 3, size=B).astype(np.int32)
    for b in range(B):
        lo, hi = head_bounds(heads[b], V, Tv, Sv)
        x = (rng.randn(hi - lo) * 3).astype(np.float32)
        if kind == "ties" or (kind == "mixed" and b % 4 == 1):
            x = np.round(x * 2) / 2                                    # planted ties everywhere, at the threshold too
        if kind == "flat" or (kind == "mixed" and b % 8 == 3):
            x[:] = np.float32(1.25)                                    # one tie class = the whole head
        lg[b, lo:hi] = x
    return lg, heads


def _check_against_ref(lg, heads, ids, V, Tv, Sv, sp, steps):
    """ids == the restatement; a mismatch is tolerated only where the target lies within 1e-5 (relative) of a running-sum boundary"""
    mism, near = 0, 0
    for b in range(lg.shape[0]):
        lo, hi = head_bounds(heads[b], V, Tv, Sv)
        u = philox_uniform(sp.seed, int(steps[b]), b)
        info = {}
        want = lo + sample_row_ref(lg[b, lo:hi], sp.temperature, sp.top_k, sp.top_p, u, info)
        assert lo <= ids[b] < hi, (b, ids[b], lo, hi)
        if ids[b] != want:
            mism += 1
            close = np.abs(info["cum"] - info["target"]).min() <= 1e-5 * info["total"]
            assert close, (b, ids[b], want, sp)
            near += 1
    return mism, near


@pytest.mark.parametrize("geom", GEOMS)
def test_op_sample_equals_restatement(geom):
    V, Tv, Sv = geom
    rng = np.random.RandomState(sum(geom))
    total, bad = 0, 0
    for T in (0.2, 1.0, 1.7):
        for k in (1, 5, 50, 1024, 0):
            for p in (0.1, 0.8, 1.0):
                if k == 0 and p < 1:
                    continue
                B = 256 if (k, p) in ((50, 1.0), (0, 1.0), (1024, 0.8)) else 48
                kind = ("mixed", "ties", "flat", "plain")[(k + int(p * 10) + int(T * 10)) % 4]
                lg, heads = _rows(B, V, Tv, Sv, rng, kind)
                steps = rng.randint(0, 4000, size=B).astype(np.int32)
                sp = SamplingParams(T, k, p, int(rng.randint(0, 2**62)) * 3 + 1)
                ids = ops.sample(torch.from_numpy(lg).cuda(), torch.from_numpy(heads).cuda(), sp, torch.from_numpy(steps).cuda(), V, Tv, Sv)
                m, _ = _check_against_ref(lg, heads, ids.cpu().numpy(), V, Tv, Sv, sp, steps)
                bad += m
                total += B
    print(f"geometry {geom}: {bad} of {total} rows differ from the restatement (all within 1e-5 of a boundary)")
    assert bad <= total * 1e-3


def test_op_sample_rejects_out_of_domain():
    lg = torch.zeros(1, 34, device="cuda")
    for sp in (SamplingParams(1.0, 0, 0.5), SamplingParams(1.0, 2000, 1.0)):
        with pytest.raises(TraceHipError, match="top_k"):
            ops.sample(lg, [0], sp, [0], 20, 3, 10)


def test_op_sample_is_deterministic_and_flat_row_covers_the_tie_class():
    V, Tv, Sv = 32000, 13, 13
    lg = torch.full((256, V + 1 + Tv + Sv), -float("inf"), device="cuda")
    lg[:, : V + 1] = 0.5
    sp = SamplingParams(1.0, 50, 1.0, 12345)
    steps = torch.arange(256, dtype=torch.int32, device="cuda")
    a = ops.sample(lg, [0] * 256, sp, steps, V, Tv, Sv)
    b = ops.sample(lg, [0] * 256, sp, steps, V, Tv, Sv)
    assert torch.equal(a, b)
    # k = 50 on a flat row keeps the whole tie class: the draws spread over the whole head, in id order
    assert int(a.max()) > 20000 and int(a.min()) < 12000


def _hf_probs(row, T, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = torch.from_numpy(row.copy()).view(1, -1)
    s = TemperatureLogitsWarper(T)(None, s)
    if k:
        s = TopKLogitsWarper(k)(None, s)
    if p < 1:
        s = TopPLogitsWarper(p)(None, s)
    return torch.softmax(s.double(), -1).view(-1).numpy()


# (the total variation of N draws from a distribution over s tokens is ~ s sqrt(2 / (pi s N)) / 2 by chance alone: the kept sets stay small enough
#  — 50 / 20 tokens of the tiny head, the toy head's 21 — for 262 144 draws to sit well below 0.01)
@pytest.mark.parametrize("T,k,p,V", [(1.0, 50, 1.0, 320), (0.7, 20, 0.8, 320), (1.7, 0, 1.0, 20), (1.0, 1024, 0.9, 20)])
def test_distribution_matches_hf_warpers(T, k, p, V):
    Tv, Sv = 13, 13
    rng = np.random.RandomState(5)
    row = (rng.randn(V + 1) * 1.5).astype(np.float32)
    row[rng.randint(0, V + 1, 8)] = row.max()                     # a tie at the top
    lg = torch.full((256, V + 1 + Tv + Sv), -float("inf"), device="cuda")
    lg[:, : V + 1] = torch.from_numpy(row).cuda()
    sp = SamplingParams(T, k, p, 99)
    counts = np.zeros(V + 1, np.int64)
    for c in range(1024):                                          # 262 144 draws: every row, 1024 step counters
        steps = torch.full((256,), c, dtype=torch.int32, device="cuda")
        ids = ops.sample(lg, [0] * 256, sp, steps, V, Tv, Sv).cpu().numpy()
        np.add.at(counts, ids, 1)
    want = _hf_probs(row, T, k, p)
    assert counts[want == 0].sum() == 0, "a draw outside the kept set"
    tv = 0.5 * np.abs(counts / counts.sum() - want).sum()
    print(f"T={T} k={k} p={p}: total variation {tv:.4f} over {counts.sum()} draws")
    assert tv <= 0.01


# ---- end to end ----
@pytest.fixture(scope="module")
def tiny():
    cfg = tcfg.tiny(num_frames=4)
    eng = TraceEngine(cfg, device=0, max_batch=8, max_ctx=192, max_frames=4, max_new_tokens=24)
    eng.load_weights(synth.state_dict(cfg).items())
    vids = [synth.synth_frames(cfg, i).to(torch.bfloat16).cuda() for i in range(4)]
    ts = [[[j * 2.5] for j in range(4)] for _ in range(4)]
    ids = [synth.synth_prompt_ids(cfg, n_text=24, video_pos=10, seed=7 + i).tolist() for i in range(4)]
    yield cfg, eng, vids, ts, ids
    eng.close()


def _model(cfg, eng):
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    return TraceMistralForCausalLM(cfg, eng)


def _check_heads(cfg, rows, heads0):
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    for row, h in zip(rows, heads0):
        for t in row:
            lo, hi = head_bounds(h, V, Tv, Sv)
            assert lo <= t < hi, (t, h)
            h = {V: 1, V + 1: 2, V + Tv + 1: 0}.get(t, h)


def test_graph_eager_and_stepwise_agree(tiny):
    cfg, eng, vids, ts, ids = tiny
    sp = SamplingParams(1.3, 0, 1.0, 2024)
    g, hg = eng.generate(vids, ts, ids, [1] * 4, 20, sampling=sp, use_graph=True)
    e, he = eng.generate(vids, ts, ids, [1] * 4, 20, sampling=sp, use_graph=False)
    assert g == e and hg == he
    _check_heads(cfg, g, [1] * 4)
    assert len({tuple(r) for r in g}) > 1                      # rows draw from their own counters
    m = _model(cfg, eng)
    kw = dict(images_or_videos=vids, video_timestamps=ts, max_new_tokens=20, do_sample=True, temperature=0.9, top_k=40, top_p=0.9, eos_token_id=-1)
    torch.manual_seed(3)
    a = m.generate(torch.tensor(ids), heads=[1] * 4, **kw)
    torch.manual_seed(3)
    b = m.generate(torch.tensor(ids), heads=[1] * 4, **kw)
    torch.manual_seed(3)
    c = m.generate(torch.tensor(ids), heads=[1] * 4, stopping_criteria=[lambda ids_, scores: torch.zeros(4, dtype=torch.bool)], **kw)
    d = m.generate(torch.tensor(ids), heads=[1] * 4, **kw)
    assert torch.equal(a, b) and torch.equal(a, c), (a, c)
    assert not torch.equal(a, d)                               # the next call draws a new seed
    _check_heads(cfg, a.tolist(), [1] * 4)


def test_top_k_one_equals_greedy(tiny):
    cfg, eng, vids, ts, ids = tiny
    m = _model(cfg, eng)
    kw = dict(images_or_videos=vids[:2], video_timestamps=ts[:2], max_new_tokens=16, eos_token_id=-1)
    g = m.generate(torch.tensor(ids[:2]), heads=[1, 1], do_sample=False, **kw)
    s = m.generate(torch.tensor(ids[:2]), heads=[1, 1], do_sample=True, temperature=1.0, top_k=1, **kw)
    assert torch.equal(g, s)


def test_eos_lengths_consistent(tiny):
    cfg, eng, vids, ts, ids = tiny
    sp = SamplingParams(1.5, 0, 1.0, 77)
    free, _ = eng.generate(vids, ts, ids, [1] * 4, 20, sampling=sp)
    eos = free[0][5]
    got, _ = eng.generate(vids, ts, ids, [1] * 4, 20, eos=eos, sampling=sp)
    for f, r in zip(free, got):
        n = f.index(eos) + 1 if eos in f else len(f)
        assert r == f[:n]


def test_host_path_outside_device_domain(tiny):
    cfg, eng, vids, ts, ids = tiny
    sp = SamplingParams(1.0, 0, 0.7, 5)                             # top_k off with top_p < 1: the host statement of the same rules
    a, _ = eng.generate(vids[:2], ts[:2], ids[:2], [1, 1], 12, sampling=sp)
    b, _ = eng.generate(vids[:2], ts[:2], ids[:2], [1, 1], 12, sampling=sp)
    assert a == b
    _check_heads(cfg, a, [1, 1])


def test_generate_stream_equals_generate(tiny):
    cfg, eng, vids, ts, ids = tiny
    sp = SamplingParams(0.8, 50, 0.95, 31337)
    batches = [(vids[:2], ts[:2], ids[:2], [1, 1], None), (vids[2:], ts[2:], ids[2:], [1, 1], None)]
    got = list(eng.generate_stream(batches, 16, sampling=sp))
    for (v, t, i, h, _), (out, heads) in zip(batches, got):
        want, wh = eng.generate(v, t, i, h, 16, sampling=sp)
        assert out == want and heads == wh


def test_fp16_library_samples():
    cfg = tcfg.tiny(num_frames=4)
    eng = TraceEngine(cfg, device=0, max_batch=2, max_ctx=192, max_frames=4, max_new_tokens=16, dtype=torch.float16)
    try:
        eng.load_weights(synth.state_dict(cfg).items())
        vids = [synth.synth_frames(cfg, i).to(torch.float16).cuda() for i in range(2)]
        ts = [[[j * 2.5] for j in range(4)]] * 2
        ids = [synth.synth_prompt_ids(cfg, n_text=24, video_pos=10, seed=9 + i).tolist() for i in range(2)]
        sp = SamplingParams(1.2, 50, 0.9, 4)
        a, _ = eng.generate(vids, ts, ids, [1, 1], 12, sampling=sp, use_graph=True)
        b, _ = eng.generate(vids, ts, ids, [1, 1], 12, sampling=sp, use_graph=False)
        assert a == b
        _check_heads(cfg, a, [1, 1])
        V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
        lg, heads = _rows(64, V, Tv, Sv, np.random.RandomState(1), "mixed")
        steps = np.arange(64, dtype=np.int32)
        got = ops.sample(torch.from_numpy(lg).cuda(), torch.from_numpy(heads).cuda(), sp, torch.from_numpy(steps).cuda(), V, Tv, Sv,
                         element="f16").cpu().numpy()
        m, _ = _check_against_ref(lg, heads, got, V, Tv, Sv, sp, steps)
        assert m == 0
    finally:
        eng.close()
