"""Per-token log-probabilities without a GPU: the float32 restatement (trace_amd/sampling.py token_logprob_ref) against a float64
log-softmax, the kernel's register budget, the argument plumbing of generate(output_logprobs=True) / generate_samples on a fake engine, and
the packed ids + float bits of the one all-gather (round trip, 2-rank gloo)."""
import os
import re
import shutil
import socket
import subprocess

import numpy as np
import pytest

from trace_amd.sampling import SamplingParams, head_bounds, token_logprob_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trace_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
GEOMS = [(32000, 13, 13), (320, 13, 13), (20, 3, 2)]          # TRACE-7B, the tiny config, a toy (the sampler's three)


def _row(n, rng, kind, scale):
    x = (rng.randn(n) * scale).astype(np.float32)
    if kind == "ties":
        x = (np.round(x * 2) / 2).astype(np.float32)
    if kind == "flat":
        x[:] = np.float32(1.25)
    return x


@pytest.mark.parametrize("geom", GEOMS)
def test_restatement_against_float64_log_softmax(geom):
    """|token_logprob_ref - float64 log-softmax| <= 1e-4 on every head of the three geometries, plain / tied / flat rows at logit scales
    0.5, 3 and 10.  The bound is derived, not measured: a run of <= 126 terms plus 8 scan levels gives <= 134 * 2^-24 ~ 8e-6 relative on S
    (absolute on log S); sample_exp adds 2e-7; sample_log (the odd atanh series to t^9 on m in (sqrt 1/2, sqrt 2], first dropped term
    < 2e-9, about ten individually rounded operations on values <= 11) adds ~1e-6; one rounding of x - M and one of the result at
    magnitudes <= 64 add <= 8e-6: about 2e-5 in all, and the bound allows five times that."""
    V, Tv, Sv = geom
    rng = np.random.RandomState(sum(geom) + 1)
    worst, checked = 0.0, 0
    for head in (0, 1, 2):
        lo, hi = head_bounds(head, V, Tv, Sv)
        n = hi - lo
        for kind in ("plain", "ties", "flat"):
            for scale in (0.5, 3.0, 10.0):
                x = _row(n, rng, kind, scale)
                x64 = x.astype(np.float64)
                want = x64 - x64.max() - np.log(np.exp(x64 - x64.max()).sum())
                picks = {int(x.argmax()), int(x.argmin()), 0, n - 1, *rng.randint(0, n, 6).tolist()}
                for i in picks:
                    got = token_logprob_ref(x, i)
                    assert got.dtype == np.float32
                    worst = max(worst, abs(float(got) - want[i]))
                    checked += 1
                assert token_logprob_ref(x, -1) == -np.inf and token_logprob_ref(x, n) == -np.inf
    print(f"geometry {geom}: worst |restatement - float64| = {worst:.3g} over {checked} tokens")
    assert worst <= 1e-4


def test_restatement_is_a_log_probability():
    rng = np.random.RandomState(3)
    x = (rng.randn(13) * 2).astype(np.float32)
    p = np.exp(np.array([token_logprob_ref(x, i) for i in range(13)], np.float64))
    assert abs(p.sum() - 1.0) < 1e-5 and int(p.argmax()) == int(x.argmax())
    assert token_logprob_ref(np.array([2.5], np.float32), 0) == 0.0                   # one token: S = 1, log 1 = 0 exactly


@pytest.mark.skipif(HIPCC is None, reason="hipcc not available")
def test_logprob_kernel_has_no_scratch(tmp_path):
    """the new kernel: ScratchSize 0 in the bf16 and the fp16 build; and the function-name counts the sampling test relies on still hold (one
    sample_rows_kernel in sample.hip, the three forms of select_next_kernel in select.hip and nowhere else: the log-probability is a kernel of
    its own, no new instantiation)"""
    for name, pat, want in (("sample", "token_logprob_kernel", 1), ("sample", "sample_rows_kernel", 1), ("select", "select_next_kernel", 3),
                            ("decode", "select_next_kernel", 0), ("decode", "token_logprob_kernel", 0), ("select", "token_logprob_kernel", 0)):
        for f16 in (False, True):
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", os.path.join(CSRC, name + ".hip"), "-I", CSRC,
                   "-o", str(tmp_path / (name + ".o")), "-Rpass-analysis=kernel-resource-usage"] + (["-DTRACE_F16"] if f16 else [])
            r = subprocess.run(cmd, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            found, cur = 0, None
            for line in r.stderr.splitlines():
                mm = re.search(r"Function Name: (\S+)", line)
                if mm:
                    cur = mm.group(1)
                mm = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
                if mm and cur and pat in cur:
                    found += 1
                    assert int(mm.group(1)) == 0, (cur, line)
            assert found == want, (name, pat, found)


# ---- argument plumbing on a fake engine ----
class _FakeEngine:
    device, dtype = "cpu", None
    max_batch, decode_batch_max = 8, 8

    def __init__(self):
        self.calls = []
        self.lps = None

    def host_mode(self, on):
        pass

    def generate(self, vids, ts, ids, heads, max_new, eos=-1, sampling=None, logprobs=False, **kw):
        self.calls.append(("generate", logprobs, sampling))
        out = [[5, 6, 7][: 3 - b % 2] for b in range(len(vids))]
        hd = [0] * len(vids)
        return (out, hd, [np.arange(len(r), dtype=np.float32) * -0.5 - 0.25 for r in out]) if logprobs else (out, hd)

    def generate_samples(self, video, ts, prompt_ids, head, n, max_new, eos=-1, sampling=None, use_graph=True):
        self.calls.append(("generate_samples", n, head, sampling, list(prompt_ids)))
        lps = self.lps[:n]
        return [[10 + r] * len(lps[r]) for r in range(n)], [r % 3 for r in range(n)], lps


def _model():
    from trace_amd.config import tiny
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    eng = _FakeEngine()
    return TraceMistralForCausalLM(tiny(num_frames=4), eng), eng


def test_output_logprobs_reaches_the_engine_and_default_is_a_tensor():
    torch = pytest.importorskip("torch")
    m, eng = _model()
    vids = [torch.zeros(4, 3, 8, 8), torch.zeros(4, 3, 8, 8)]
    kw = dict(images_or_videos=vids, video_timestamps=[[[0.0]] * 4] * 2, heads=[1, 1], max_new_tokens=4, eos_token_id=-1)
    plain = m.generate(torch.tensor([[1, 2], [3, 4]]), **kw)
    assert isinstance(plain, torch.Tensor) and eng.calls[-1][:2] == ("generate", False)
    kw["heads"] = [1, 1]
    res = m.generate(torch.tensor([[1, 2], [3, 4]]), output_logprobs=True, **kw)
    assert eng.calls[-1][:2] == ("generate", True)
    assert torch.equal(res.sequences, plain)
    assert res.logprobs.dtype == torch.float32 and tuple(res.logprobs.shape) == tuple(plain.shape)
    assert res.logprobs.tolist() == [[-0.25, -0.75, -1.25], [-0.25, -0.75, 0.0]]      # zero padded past the row's length
    assert res.heads == [0, 0]
    with pytest.raises(NotImplementedError):                                          # n-best is not a generate() keyword
        m.generate(torch.tensor([[1, 2], [3, 4]]), do_sample=True, num_return_sequences=2, output_logprobs=True, **kw)


def test_generate_samples_arguments_and_ranking():
    torch = pytest.importorskip("torch")
    m, eng = _model()
    v, ts = [torch.zeros(4, 3, 8, 8)], [[[0.0]] * 4]
    ok = dict(images_or_videos=v, video_timestamps=ts, heads=[1], max_new_tokens=4, eos_token_id=-1)
    with pytest.raises(ValueError, match="one prompt"):
        m.generate_samples(torch.tensor([[1, 2], [3, 4]]), images_or_videos=v * 2, video_timestamps=ts * 2, n=2, temperature=1.0)
    for bad_n in (0, -1):
        with pytest.raises(ValueError, match="n must be"):
            m.generate_samples(torch.tensor([1, 2]), n=bad_n, temperature=1.0, **ok)
    with pytest.raises(ValueError, match="greedy"):
        m.generate_samples(torch.tensor([1, 2]), n=2, temperature=0.0, **ok)
    with pytest.raises(NotImplementedError):
        m.generate_samples(torch.tensor([1, 2]), n=2, temperature=1.0, num_beams=2, **ok)
    assert not eng.calls
    # hand-made log-probabilities: sums -3, -1, -3, -0.5, -1 -> best first 3, 1, 4, 0, 2 (ties to the lower decode row)
    f = lambda *a: np.array(a, np.float32)
    eng.lps = [f(-1, -2), f(-0.5, -0.5), f(-3,), f(-0.25, -0.25), f(-0.5, -0.25, -0.25)]
    torch.manual_seed(5)
    res = m.generate_samples(torch.tensor([1, 2]), n=5, temperature=0.7, top_k=20, top_p=0.8, **ok)
    name, n, head, sp, prompt = eng.calls[-1]
    assert (name, n, head, prompt) == ("generate_samples", 5, 1, [1, 2])
    assert (sp.temperature, sp.top_k, sp.top_p) == (0.7, 20, 0.8)
    torch.manual_seed(5)
    assert m._sampling_params(True, 0.7, 20, 0.8, None, {}).seed == sp.seed            # the seed comes as in generate(do_sample=True)
    assert res.order == [3, 1, 4, 0, 2]
    assert res.scores.dtype == torch.float64 and res.scores.tolist() == [-0.5, -1.0, -1.0, -3.0, -3.0]
    assert res.sequences[:, 0].tolist() == [13, 11, 14, 10, 12]
    assert res.logprobs.dtype == torch.float32 and res.logprobs[2].tolist() == [-0.5, -0.25, -0.25] and res.logprobs[4].tolist() == [-3.0, 0.0, 0.0]
    assert res.heads == [0, 1, 1, 0, 2]
    keep = m.generate_samples(torch.tensor([1, 2]), n=5, temperature=0.7, best_first=False, **ok)
    assert keep.order == [0, 1, 2, 3, 4] and keep.scores.tolist() == [-3.0, -1.0, -3.0, -0.5, -1.0]
    # the float64 accumulation: 2^24 + 1 + 1 is not representable step by step in float32
    eng.lps = [f(-16777216.0, -1.0, -1.0), f(-16777216.0, -1.0)]
    r2 = m.generate_samples(torch.tensor([1, 2]), n=2, temperature=1.0, **ok)
    assert r2.scores.tolist() == [-16777217.0, -16777218.0] and r2.order == [1, 0]


def test_engine_generate_samples_refuses_greedy_and_bad_n():
    from trace_amd.engine import TraceEngine
    eng = TraceEngine.__new__(TraceEngine)                    # argument checks only: they come before any device work
    eng.max_batch, eng.llm_fp8 = 4, True                      # decode_batch_max = min(max_batch, 64) without touching the library
    for n in (0, 5):
        with pytest.raises(ValueError, match="n = "):
            eng.generate_samples(None, None, [1], 1, n, 4, sampling=SamplingParams(1.0, 50, 1.0, 1))
    for sp in (None, SamplingParams(0.0, 50, 1.0, 1)):
        with pytest.raises(ValueError, match="greedy"):
            eng.generate_samples(None, None, [1], 1, 2, 4, sampling=sp)


# ---- the one all-gather: ids and float bits in one packed int32 tensor ----
def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def test_pack_roundtrip_of_ids_and_float_bits():
    torch = pytest.importorskip("torch")
    from trace_amd import dist as tdist
    ids = [[1, 2, 3, 4, 5], [], [32026] * 3]
    lps = [np.array([-np.inf, -0.0, 1e-42, -1.4e-45, -3.25], np.float32), np.zeros(0, np.float32), np.array([-0.1, -2.0, -7.5], np.float32)]
    packed = tdist.pack_ids_logprobs(ids, lps, 8)
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (3, 17)
    got_ids, got_lps = tdist.unpack_ids_logprobs(packed)
    assert got_ids == ids
    for a, b in zip(got_lps, lps):
        assert a.dtype == np.float32 and _bits(a) == _bits(b)                           # -inf, -0.0 and the denormals exactly
    assert _bits(got_lps[0])[:2] == [0xFF800000, 0x80000000] and got_lps[0][2] != 0
    g_ids, g_lps = tdist.gather_outputs_logprobs(ids, lps, 8, 4)                        # no process group: one "rank", padded with empties
    assert g_ids == [ids + [[]]] and [_bits(x) for x in g_lps[0]] == [_bits(x) for x in lps] + [[]]
    with pytest.raises(ValueError):
        tdist.pack_ids_logprobs([[1, 2]], [np.zeros(1, np.float32)], 8)
    assert tdist.unpack_ids(tdist.pack_ids(ids, 8)) == ids                              # the id-only helpers keep their behaviour


def _fake(video_idx, max_new):
    n = 3 + (video_idx * 7) % (max_new - 3)
    ids = [(video_idx * 31 + i) % 32027 for i in range(n)]
    lp = (-np.arange(1, n + 1, dtype=np.float32) / np.float32(video_idx + 3)).astype(np.float32)
    lp[0] = -np.inf if video_idx % 3 == 0 else np.float32(-1e-41)
    return ids, lp


def _worker(rank, world, port, n_videos, max_new, q):
    import torch
    import torch.distributed as dist
    from trace_amd import dist as tdist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    r, _, w = tdist.init_from_env("gloo")
    mine = tdist.shard_indices(n_videos, r, w)
    per_rank = (n_videos + w - 1) // w
    local = [_fake(i, max_new) for i in mine]
    g_ids, g_lps = tdist.gather_outputs_logprobs([x[0] for x in local], [x[1] for x in local], max_new, per_rank, torch.device("cpu"))
    ids = tdist.merge_round_robin(g_ids, n_videos)
    lps = tdist.merge_round_robin(g_lps, n_videos)
    q.put((rank, ids, [_bits(x) for x in lps]))
    dist.destroy_process_group()


def test_two_rank_gather_carries_the_float_bits():
    mp = pytest.importorskip("torch.multiprocessing")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    n_videos, max_new = 7, 16
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_videos, max_new, q)) for r in range(2)]
    [p.start() for p in procs]
    res = [q.get(timeout=120) for _ in procs]
    [p.join(timeout=60) for p in procs]
    want = [_fake(i, max_new) for i in range(n_videos)]
    for rank, ids, bits in res:
        assert ids == [w[0] for w in want], rank
        assert bits == [_bits(w[1]) for w in want], rank
