"""Scoring given continuations without a GPU: the float32 restatement of the scoring kernels (trace_amd/sampling.py score_logprob_ref) against a
float64 log-softmax on every teacher-forced step of the reference fixtures, the head chain and the embedding map against the oracle, the row
alignment (one forward over [prompt, c[:-1]] gives the rows the step-by-step decode gives), padding / ignore / out-of-head handling, the
grouping, and the argument errors of model.score and TraceEngine.score_continuations."""
import os

import numpy as np
import pytest
import torch

from oracle import trace_oracle as O
from trace_amd import config as tcfg, scoring, synth
from trace_amd.sampling import SCORE_TILE, head_bounds, score_logprob_ref, score_tile_partials, token_logprob_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = {"tiny_e2e": 48, "deep_llm": 48, "long_ctx": 24, "charades_ctx": 31, "videomme_ctx": 15}
REF_BOUND = 5e-5


def _head_of(row):
    fin = np.nonzero(np.isfinite(row))[0]
    return int(fin[0]), int(fin[-1]) + 1


def test_restatement_against_float64_on_every_fixture_step():
    """|score_logprob_ref - float64 log-softmax| <= 5e-5 for the forced id of EVERY step of the five fixtures (48 / 48 / 24 / 31 / 15 steps; heads
    13 and 321 wide: V = 320).  Derived before running, from sample.h's stated errors and fp32 summation over the head's width:
      * a half tile is a sequential sum of <= 64 weights and h0 + h1 one more addition: <= 64 roundings, 64 * 2^-24 = 3.8e-6 relative on s_j;
      * every weight carries sample_exp's 2e-7, every merge term one more sample_exp and one product (2e-7 + 6e-8), and the merge adds <= 3
        tiles (321 / 128): 4e-6 + 5e-7 + 2e-7 < 5e-6 relative on S, i.e. absolute on log S;
      * sample_log: the dropped term 2e-9 plus about ten individually rounded operations on values <= 6: ~1e-6;
      * x_t - M and the final subtraction: one rounding each at magnitudes < 64, <= 2^-19 = 1.9e-6 each.
    About 1e-5 in all; the bound allows five times that, as test_logprob_cpu.py does for token_logprob_ref.  Also checked: every forced id lies
    inside its step's head, the first four fixtures visit all three heads, videomme_ctx only the time and score heads."""
    worst = 0.0
    for name, steps in FIXTURES.items():
        E = np.load(os.path.join(GOLDEN, name + ".npz"))
        tf, forced = E["tf_logits"], E["forced_ids"]
        assert len(forced) == steps and tf.shape[0] == steps + 1
        seen = set()
        for i, t in enumerate(forced):
            lo, hi = _head_of(tf[i])
            assert lo <= t < hi, (name, i, t)
            seen.add((lo, hi))
            x = tf[i].astype(np.float64)[lo:hi]
            want = x[t - lo] - x.max() - np.log(np.exp(x - x.max()).sum())
            got = score_logprob_ref(tf[i], lo, hi, int(t))
            assert got.dtype == np.float32
            worst = max(worst, abs(float(got) - want))
        widths = sorted(hi - lo for lo, hi in seen)
        assert widths == ([13, 13] if name == "videomme_ctx" else [13, 13, 321]), (name, widths)
    print(f"worst |restatement - float64| over {sum(FIXTURES.values())} steps: {worst:.3g}")
    assert worst <= REF_BOUND


def test_restatement_tiles_halves_and_special_ids():
    """the tile rule on absolute columns: a head that straddles a tile boundary is two tiles, one inside a tile a single one whose halves split at
    the tile's middle column; -1 -> 0.0, outside the head -> -inf; a one-id head scores 0 exactly; wide heads stay within the derived bound
    (251 tiles: 64 + 251 roundings ~ 2e-5 relative on S, allowed 1e-4)"""
    rng = np.random.RandomState(5)
    x = (rng.randn(33000) * 3).astype(np.float32)
    assert SCORE_TILE == 128
    for lo, hi, ntile in ((0, 32001, 251), (32001, 32014, 1), (4500, 4513, 1), (120, 140, 2), (0, 4500, 36), (64, 128, 1), (127, 129, 2)):
        m, s = score_tile_partials(x, lo, hi)
        assert len(m) == len(s) == ntile and m.dtype == s.dtype == np.float32 and (s >= 1).all()
        x64 = x[lo:hi].astype(np.float64)
        ls = x64.max() + np.log(np.exp(x64 - x64.max()).sum())
        for t in (lo, hi - 1, lo + int(x[lo:hi].argmax()), (lo + hi) // 2):
            assert abs(float(score_logprob_ref(x, lo, hi, t)) - (float(x[t]) - ls)) <= 1e-4
        assert score_logprob_ref(x, lo, hi, -1) == 0.0 and score_logprob_ref(x, lo, hi, hi) == -np.inf
        if lo:
            assert score_logprob_ref(x, lo, hi, lo - 1) == -np.inf
    # a one-id head: S = 1, log 1 = 0 exactly
    assert score_logprob_ref(x, 7, 8, 7) == 0.0
    # a decoy outside the head changes nothing; -inf inside the head weighs 0
    y = x.copy()
    y[4513] = 1e9
    assert score_logprob_ref(y, 4500, 4513, 4505).view(np.uint32) == score_logprob_ref(x, 4500, 4513, 4505).view(np.uint32)
    z = x.copy()
    z[4501] = -np.inf
    ref = np.delete(z[4500:4513], 1).astype(np.float64)
    assert abs(float(score_logprob_ref(z, 4500, 4513, 4505)) - (float(z[4505]) - ref.max() - np.log(np.exp(ref - ref.max()).sum()))) <= REF_BOUND
    assert score_logprob_ref(z, 4500, 4513, 4501) == -np.inf
    # the same distribution as the decode step's restatement, to within both bounds (the two sum in different orders)
    assert abs(float(score_logprob_ref(x, 0, 4500, 77)) - float(token_logprob_ref(x[:4500], 77))) <= 2e-4


@pytest.fixture(scope="module")
def tiny_oracle():
    cfg = tcfg.tiny(num_frames=4)
    sd = {k: v.float() for k, v in synth.state_dict(cfg).items()}
    return cfg, O.Oracle(cfg, sd, emulate_bf16=False)


def test_head_chain_against_the_oracle(tiny_oracle):
    cfg, _ = tiny_oracle
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    rng = np.random.RandomState(1)
    special = [V, V + 1, V + Tv + 1]
    for h0 in (0, 1, 2):
        ids = [int(t) for t in rng.randint(0, V + 1 + Tv + Sv, 200)]
        for k in range(0, 200, 7):
            ids[k] = special[(k // 7) % 3]
        want, h = [], h0
        for t in ids:
            want.append(h)
            h = O.swap_head(cfg, t, h)
        assert scoring.head_chain(cfg, ids, h0) == want
        assert set(want) == {0, 1, 2}
    for name in ("tiny_e2e", "charades_ctx"):                      # the fixtures' own streams: the chain names the head whose range is finite
        E = np.load(os.path.join(GOLDEN, name + ".npz"))
        chain = scoring.head_chain(cfg, E["forced_ids"].tolist(), 1)
        for i, h in enumerate(chain):
            assert head_bounds(h, V, Tv, Sv) == _head_of(E["tf_logits"][i]) == O.head_range(cfg, h), (name, i)


def test_embedding_map_against_decode_embed(tiny_oracle):
    """ids -> placeholders + tower rows, resolved by the rule of trace_embed_rows, gives oracle.decode_embed's row for every kind of id"""
    cfg, ora = tiny_oracle
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    ids = [0, 5, V - 1, V, V + 1, V + 7, V + Tv, V + Tv + 1, V + Tv + 4, V + Tv + Sv, 17, V]
    out, tr, sr = scoring.embed_placeholders(cfg, ids)
    assert len(out) == len(ids) and out.count(-203) == len(tr) and out.count(-204) == len(sr) and out.count(-205) == 2
    W, ti, si = ora.W, 0, 0
    for t, p in zip(ids, out):
        if p == -205:
            row = W["model.sync_tower.embed_tokens.weight"][0]
        elif p == -203:
            row = W["model.time_tower.embed_tokens.weight"][tr[ti]]
            ti += 1
        elif p == -204:
            row = W["model.score_tower.embed_tokens.weight"][sr[si]]
            si += 1
        else:
            assert 0 <= p < V
            row = W["model.embed_tokens.weight"][p]
        assert torch.equal(row, ora.decode_embed(t)), t
    assert all(0 <= r < Tv for r in tr) and all(0 <= r < Sv for r in sr)


def test_one_forward_gives_the_rows_the_decode_gives(tiny_oracle):
    """Alignment, on the oracle in fp32: llm_forward over [prompt, embed(c[:-1])] — rows P - 1 .. P - 2 + n — gives, under head_chain(c), the
    logits generate(forced_ids=c, return_logits=True) gives step by step.  Tolerance 1e-3: the same fp32 arithmetic in another blocking (a
    100-row matmul against one-row matmuls over a cache), logits of magnitude ~3."""
    cfg, ora = tiny_oracle
    E = np.load(os.path.join(GOLDEN, "tiny_e2e.npz"))
    c = E["forced_ids"].tolist()[:22]
    assert {0, 1, 2} <= set(scoring.head_chain(cfg, c, 1))
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16).float()
    ids, ts = torch.from_numpy(E["input_ids"]), E["timestamps"].tolist()
    _, step_logits = ora.generate(ids, frames, ts, head=1, max_new_tokens=len(c), forced_ids=c, return_logits=True)
    emb = ora.splice(ids, ora.encode_video(frames, ts))
    P = emb.shape[0]
    fed = torch.stack([ora.r(ora.decode_embed(t)) for t in c[:-1]])
    hidden, _ = ora.llm_forward(torch.cat([emb, fed], 0))
    chain = scoring.head_chain(cfg, c, 1)
    for i, h in enumerate(chain):
        row = ora.logits(hidden[P - 1 + i], h)
        fin = torch.isfinite(step_logits[i])
        assert torch.equal(fin, torch.isfinite(row)), i
        assert float((row[fin] - step_logits[i][fin]).abs().max()) <= 1e-3, i
        lo, hi = O.head_range(cfg, h)
        a = score_logprob_ref(row.numpy(), lo, hi, c[i])
        b = score_logprob_ref(step_logits[i].numpy(), lo, hi, c[i])
        assert abs(float(a) - float(b)) <= 2e-3


def test_padding_targets_and_groups():
    cfg = tcfg.tiny(num_frames=4)
    c = [3, 4, cfg.vocab_size, cfg.vocab_size + 2]
    assert scoring.fed_ids(c, 4) == [3, 4, cfg.vocab_size]
    assert scoring.fed_ids(c, 7, pad_id=9) == [3, 4, cfg.vocab_size, 9, 9, 9]
    assert scoring.fed_ids([5], 1) == []
    chain = scoring.head_chain(cfg, c, 0)
    assert chain == [0, 0, 0, 1]
    tg, hd = scoring.targets(c, chain, 7)
    assert tg == c + [-1, -1, -1] and hd == chain + [0, 0, 0]
    row = np.zeros(347, np.float32)
    assert [float(score_logprob_ref(row, *head_bounds(h, 320, 13, 13), t)) for t, h in zip(tg, hd)][4:] == [0.0, 0.0, 0.0]
    # groups: at most 8, in order, each group's padded size within the cap
    assert scoring.groups_of([3] * 9, 1000) == [list(range(8)), [8]]
    assert scoring.groups_of([10, 10, 10], 25) == [[0, 1], [2]]
    assert scoring.groups_of([5, 20, 5], 40) == [[0, 1], [2]]            # (2 x 20 fits, 3 x 20 does not)
    assert scoring.groups_of([4, 4, 4], 100, group_max=2) == [[0, 1], [2]]
    with pytest.raises(ValueError):
        scoring.groups_of([50], 40)
    with pytest.raises(ValueError):
        scoring.check_continuation(cfg, [], 1)
    with pytest.raises(ValueError):
        scoring.check_continuation(cfg, [347], 1)
    with pytest.raises(ValueError):
        scoring.check_continuation(cfg, [-1], 1)
    with pytest.raises(ValueError):
        scoring.check_continuation(cfg, [1], 3)


# ---- argument plumbing on a fake engine ----
class _FakeEngine:
    device, dtype = "cpu", None
    max_batch, decode_batch_max = 8, 8

    def __init__(self):
        self.calls = []

    def host_mode(self, on):
        pass

    def prefix_entry(self):
        return None

    def _drop_prefix(self):
        pass

    def encode_video(self, v, ts):
        self.calls.append("encode")

    def splice(self, ids, want_output=False):
        self.calls.append("splice")
        return 6, torch.zeros(6, 8)

    def prefill(self, slot, L, embeds=None):
        self.calls.append(("prefill", slot, L))

    def score_continuations(self, slot0, P, tail, conts, head):
        self.calls.append(("score", slot0, P, tuple(tail.shape), [list(c) for c in conts], list(head)))
        lps = [np.full(len(c), -0.5 * (b + 1), np.float32) for b, c in enumerate(conts)]
        return lps, [[1] * len(c) for c in conts], np.array([np.sum(x, dtype=np.float64) for x in lps])


def _model():
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    eng = _FakeEngine()
    return TraceMistralForCausalLM(tcfg.tiny(num_frames=4), eng), eng


def test_model_score_arguments_and_result():
    m, eng = _model()
    v, ts = [torch.zeros(4, 3, 8, 8)], [[[0.0]] * 4]
    ok = dict(images_or_videos=v, video_timestamps=ts)
    with pytest.raises(ValueError, match="one prompt"):
        m.score(torch.tensor([[1, -201], [3, -201]]), images_or_videos=v * 2, video_timestamps=ts * 2, continuations=[[1]])
    with pytest.raises(ValueError, match="at least one continuation"):
        m.score(torch.tensor([1, -201, 4]), continuations=[], **ok)
    with pytest.raises(ValueError, match="timestamps"):
        m.score(torch.tensor([1, -201, 4]), images_or_videos=v, continuations=[[1]])
    with pytest.raises(ValueError, match="empty"):
        m.score(torch.tensor([1, -201, 4]), continuations=[[1], []], **ok)
    with pytest.raises(ValueError, match="global vocabulary"):
        m.score(torch.tensor([1, -201, 4]), continuations=[[400]], **ok)
    with pytest.raises(ValueError, match="head must be"):
        m.score(torch.tensor([1, -201, 4]), continuations=[[4]], heads=[5], **ok)
    with pytest.raises(ValueError, match="one per continuation"):
        m.score(torch.tensor([1, -201, 4]), continuations=[[4], [5], [6]], heads=[1, 0], **ok)
    with pytest.raises(TypeError):
        m.score(torch.tensor([1, -201, 4]), continuations=[[4]], max_new_tokens=4, **ok)
    assert not eng.calls, "an argument error came after device work"
    res = m.score(torch.tensor([1, -201, 4]), continuations=[[4, 5], torch.tensor([6]), [7, 8, 9]], **ok)
    assert eng.calls[:3] == ["encode", "splice", ("prefill", 0, 5)]
    assert eng.calls[3] == ("score", 0, 6, (1, 8), [[4, 5], [6], [7, 8, 9]], [1, 1, 1])
    assert res.scores.dtype == np.float64 and res.scores.tolist() == [-1.0, -1.0, -4.5]
    assert res.order == [0, 1, 2] and [len(x) for x in res.logprobs] == [2, 1, 3] and res.heads[2] == [1, 1, 1]
    with pytest.raises(NotImplementedError):                       # the training loss is still outside the accelerated path
        m.forward(input_ids=torch.tensor([[1, -201]]), labels=torch.tensor([[1, 2]]))


def test_engine_score_continuations_argument_errors():
    from trace_amd.engine import TraceEngine
    eng = TraceEngine.__new__(TraceEngine)                     # argument checks only: they come before any device work
    eng.cfg, eng.max_batch, eng.max_ctx, eng.device, eng.dtype = tcfg.tiny(num_frames=4), 4, 64, "cpu", torch.bfloat16
    row = torch.zeros(4096, dtype=torch.bfloat16)
    for conts, kw, msg in (([], {}, "no continuation"), ([[1], []], {}, "empty"), ([[999]], {}, "global vocabulary"), ([[1]], {"head": 7}, "head must be"),
                           ([[1], [2]], {"head": [1]}, "one per continuation"), ([[1]], {"pad_id": 320}, "text id"), ([[1] * 60], {}, "max_ctx")):
        with pytest.raises(ValueError, match=msg):
            eng.score_continuations(0, 10, row, conts, **kw)
    with pytest.raises(ValueError, match="past_rows"):
        eng.score_continuations(0, 1, torch.zeros(2, 4096, dtype=torch.bfloat16), [[1]])
    with pytest.raises(ValueError, match="hidden"):
        eng.score_continuations(0, 10, torch.zeros(7, dtype=torch.bfloat16), [[1]])


def test_score_kernels_have_no_scratch_and_fit_two_workgroups_per_cu(tmp_path):
    """score.hip compiled for gfx950, both element types: ScratchSize 0 for both kernels, and the GEMM within 128 registers of the unified file
    (VGPRs + AGPRs): four waves per SIMD, so the two workgroups per CU its 66.8 KB of LDS allow are not cut down by registers.  Cost: two
    device-only compiles of one file, about 5 s together — the way test_kernel_resources.py and test_logprob_cpu.py guard their kernels (the objects
    the build leaves carry no remarks, so there is nothing cheaper to read them from)."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "trace_amd", "csrc")
    for f16 in (False, True):
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(csrc, "score.hip"), "-I", csrc,
               "-o", str(tmp_path / "score.o"), "-Rpass-analysis=kernel-resource-usage"] + (["-DTRACE_F16"] if f16 else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        res, cur = {}, None
        for line in r.stderr.splitlines():
            mm = re.search(r"Function Name: (\S+)", line)
            if mm:
                cur = res.setdefault(mm.group(1), {})
            mm = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
            if mm and cur is not None:
                cur[mm.group(1).split(" ")[0]] = int(mm.group(2))
        head = [v for k, v in res.items() if "score_head_kernel" in k]
        merge = [v for k, v in res.items() if "score_merge_kernel" in k]
        assert len(head) == 1 and len(merge) == 1, list(res)
        assert head[0]["ScratchSize"] == 0 and merge[0]["ScratchSize"] == 0, res
        assert head[0]["VGPRs"] + head[0].get("AGPRs", 0) <= 128, head[0]
