"""min_p, typical_p, epsilon_cutoff and eta_cutoff on the device (trace_amd/csrc/sample.h sample_warp): trace_op_sample_ex against the float32
restatement (trace_amd/sampling.py) and HF's own warpers, the four-off path against the old entry point, and generate() end to end on the tiny
synthetic model — graph replay, eager steps, the stepwise host loop and the host path agree."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine, _ptr, _stream, ops  # noqa: E402
from trace_amd.sampling import head_bounds, philox_uniform, sample_row_ref, sample_rows_host  # noqa: E402

ARMED = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=2e-2)
CASES = [{name: v} for name, v in ARMED.items()] + [ARMED, dict(min_p=0.3, typical_p=0.3, epsilon_cutoff=0.05, eta_cutoff=0.3)]


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
    """ids == the restatement; a mismatch is tolerated only where a decision of the restatement lies within 1e-5 (relative) of its threshold: a
    warper's keep-or-drop (info['margin']) or the draw's target against a running sum"""
    mism = 0
    for b in range(lg.shape[0]):
        lo, hi = head_bounds(heads[b], V, Tv, Sv)
        u = philox_uniform(sp.seed, int(steps[b]), b)
        info = {}
        want = lo + sample_row_ref(lg[b, lo:hi], sp.temperature, sp.top_k, sp.top_p, u, info, *sp.warpers)
        assert lo <= ids[b] < hi, (b, ids[b], lo, hi)
        if ids[b] != want:
            mism += 1
            close = info["margin"] <= 1e-5 or np.abs(info["cum"] - info["target"]).min() <= 1e-5 * info["total"]
            assert close, (b, ids[b], want, sp, info["margins"])
    return mism


@pytest.mark.parametrize("geom,ks", [((20, 3, 10), (5, 50)), ((320, 13, 13), (50, 1024)), ((1500, 13, 13), (1024,))])
def test_op_sample_equals_restatement(geom, ks):
    V, Tv, Sv = geom
    rng = np.random.RandomState(sum(geom))
    total = bad = 0
    for T in (0.2, 1.0, 1.7):
        for k in ks:
            for ci, case in enumerate(CASES):
                p = 1.0 if len(case) == 1 else (0.9, 0.6)[ci % 2]
                B = 256 if case is ARMED and k == ks[-1] else 48
                kind = ("mixed", "ties", "flat", "plain")[(ci + k + int(T * 10)) % 4]
                lg, heads = _rows(B, V, Tv, Sv, rng, kind)
                steps = rng.randint(0, 4000, size=B).astype(np.int32)
                sp = SamplingParams(T, k, p, int(rng.randint(0, 2**62)) * 3 + 1, **case)
                ids = ops.sample(torch.from_numpy(lg).cuda(), torch.from_numpy(heads).cuda(), sp, torch.from_numpy(steps).cuda(), V, Tv, Sv)
                bad += _check_against_ref(lg, heads, ids.cpu().numpy(), V, Tv, Sv, sp, steps)
                total += B
    print(f"geometry {geom}: {bad} of {total} rows differ from the restatement (all within 1e-5 of a boundary)")
    assert bad <= total * 1e-3


def _old_entry(lg, heads, sp, steps, V, Tv, Sv):
    """trace_op_sample, the entry point without the four"""
    lib = _lib.load()
    B, ld = lg.shape
    hd = torch.tensor(list(heads), dtype=torch.int32, device=lg.device)
    out = torch.empty(B, dtype=torch.int32, device=lg.device)
    _lib.check(lib.trace_op_sample(_ptr(lg), ld, B, _ptr(hd), V, Tv, Sv, float(sp.temperature), int(sp.top_k), float(sp.top_p), int(sp.seed),
                                   _ptr(steps), _ptr(out), _stream()))
    return out


def test_four_off_is_the_old_entry_point():
    rng = np.random.RandomState(11)
    for (V, Tv, Sv), kind in (((320, 13, 13), "mixed"), ((20, 3, 10), "ties"), ((1500, 13, 13), "plain")):
        for T, k, p in ((0.2, 50, 1.0), (1.0, 5, 0.8), (1.7, 1024, 0.1), (1.0, 0, 1.0), (0.7, 1024, 0.9)):
            lg_np, heads = _rows(128, V, Tv, Sv, rng, kind)
            lg = torch.from_numpy(lg_np).cuda()
            steps = torch.from_numpy(rng.randint(0, 4000, size=128).astype(np.int32)).cuda()
            sp = SamplingParams(T, k, p, int(rng.randint(0, 2**62)) * 3 + 1)
            assert torch.equal(ops.sample(lg, heads.tolist(), sp, steps, V, Tv, Sv), _old_entry(lg, heads.tolist(), sp, steps, V, Tv, Sv)), (V, T, k, p)
    V, Tv, Sv = 32000, 13, 13                                            # the flat 32 001-wide row: one tie class = the whole head
    lg = torch.full((256, V + 1 + Tv + Sv), -float("inf"), device="cuda")
    lg[:, : V + 1] = 0.5
    steps = torch.arange(256, dtype=torch.int32, device="cuda")
    for k, p in ((50, 1.0), (50, 0.3), (0, 1.0)):
        sp = SamplingParams(1.0, k, p, 12345)
        a = ops.sample(lg, [0] * 256, sp, steps, V, Tv, Sv)
        assert torch.equal(a, _old_entry(lg, [0] * 256, sp, steps, V, Tv, Sv))
    assert int(a.max()) > 20000 and int(a.min()) < 12000


def test_typical_p_never_draws_the_dropped_arg_max():
    # one token at p = 0.3 beside 70 at 0.01, typical_p = 0.6: the 70 stay, the top one goes (tests/test_sampling_warpers_cpu.py has the arithmetic)
    V, Tv, Sv = 70, 3, 10
    row = np.log(np.array([0.01] * 30 + [0.3] + [0.01] * 40)).astype(np.float32)
    for variant in ("tie block", "candidates"):
        if variant == "candidates":                                       # the 70 all different: an interval of the sorted candidates
            row[np.arange(71) != 30] += np.linspace(-0.05, 0.05, 70).astype(np.float32)
        lg = torch.full((256, V + 1 + Tv + Sv), -float("inf"), device="cuda")
        lg[:, : V + 1] = torch.from_numpy(row).cuda()
        sp = SamplingParams(1.0, 1024, 1.0, 4242, typical_p=0.6)
        counts = np.zeros(V + 1, np.int64)
        for c in range(64):
            steps = torch.full((256,), c, dtype=torch.int32, device="cuda")
            np.add.at(counts, ops.sample(lg, [0] * 256, sp, steps, V, Tv, Sv).cpu().numpy(), 1)
        assert counts[30] == 0, (variant, counts[30])
        info = {}
        sample_row_ref(row, 1.0, 1024, 1.0, np.float32(0.5), info, typical_p=0.6)
        kept = np.sort(info["kept"])                                      # all 70 of the tie block; of the 70 different ones those that reach 0.6
        assert (len(kept) == 70 if variant == "tie block" else 60 <= len(kept) < 70) and 30 not in kept
        assert counts.sum() == counts[kept].sum()
        # 16 384 draws over the kept tokens, within 5 % of equally probable: mean = 16 384 / len(kept), sigma = sqrt(mean); five and a half sigma either way
        mean = counts.sum() / len(kept)
        assert counts[kept].min() > 0.95 * mean - 5.5 * mean ** 0.5 and counts[kept].max() < 1.05 * mean + 5.5 * mean ** 0.5, (variant, counts[kept])


def _hf_probs(row, T, k, p, min_p, typical_p, epsilon_cutoff, eta_cutoff):
    from transformers.generation import logits_process as lp
    s = torch.from_numpy(row.copy()).view(1, -1)
    for w in (lp.TemperatureLogitsWarper(T), lp.TopKLogitsWarper(k), lp.TopPLogitsWarper(p), lp.MinPLogitsWarper(min_p),
              lp.TypicalLogitsWarper(typical_p), lp.EpsilonLogitsWarper(epsilon_cutoff), lp.EtaLogitsWarper(eta_cutoff)):
        s = w(None, s)
    return torch.softmax(s.double(), -1).view(-1).numpy()


def test_distribution_matches_hf_warpers_all_armed():
    """the bound and the reasoning of tests/test_gpu_sampling.py test_distribution_matches_hf_warpers: the total variation of N draws over s tokens
    is ~ s sqrt(2 / (pi s N)) / 2 by chance alone; s <= 50 and N = 262 144 sit well below 0.01"""
    V, Tv, Sv = 320, 13, 13
    rng = np.random.RandomState(5)
    row = (rng.randn(V + 1) * 1.5).astype(np.float32)
    row[rng.randint(0, V + 1, 8)] = row.max()                     # a tie at the top
    # top_k leaves 50, top_p 44, typical_p 36, epsilon 33, eta 26 (every decision at least 1e-3 from its threshold by the restatement's margins)
    T, k, p = 0.9, 50, 0.97
    warp = dict(min_p=0.02, typical_p=0.95, epsilon_cutoff=8e-3, eta_cutoff=0.06)
    want = _hf_probs(row, T, k, p, **warp)
    assert (want > 0).sum() == 26
    lg = torch.full((256, V + 1 + Tv + Sv), -float("inf"), device="cuda")
    lg[:, : V + 1] = torch.from_numpy(row).cuda()
    sp = SamplingParams(T, k, p, 99, **warp)
    counts = np.zeros(V + 1, np.int64)
    for c in range(1024):                                          # 262 144 draws: every row, 1024 step counters
        steps = torch.full((256,), c, dtype=torch.int32, device="cuda")
        np.add.at(counts, ops.sample(lg, [0] * 256, sp, steps, V, Tv, Sv).cpu().numpy(), 1)
    assert counts[want == 0].sum() == 0, "a draw outside HF's kept set"
    tv = 0.5 * np.abs(counts / counts.sum() - want).sum()
    print(f"all four armed: {(want > 0).sum()} tokens kept, total variation {tv:.4f} over {counts.sum()} draws")
    assert tv <= 0.01


def test_armed_warper_with_top_k_off_is_out_of_domain():
    lg = torch.zeros(1, 34, device="cuda")
    for name, v in ARMED.items():
        with pytest.raises(TraceHipError, match="top_k"):
            ops.sample(lg, [0], SamplingParams(1.0, 0, 1.0, **{name: v}), [0], 20, 3, 10)
    bad = _lib.TraceSamplingC(C.sizeof(_lib.TraceSamplingC) - 4, 1.0, 50, 1.0, 0, 0.0, 1.0, 0.0, 0.0)
    out, hd, st = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3))
    with pytest.raises(TraceHipError, match="size"):
        _lib.load().trace_op_sample_ex(_ptr(lg), 34, 1, _ptr(hd), 20, 3, 10, C.byref(bad), _ptr(st), _ptr(out), _stream())


def test_fp16_library_draws_the_same_ids():
    V, Tv, Sv = 320, 13, 13
    lg, heads = _rows(96, V, Tv, Sv, np.random.RandomState(1), "mixed")
    steps = np.arange(96, dtype=np.int32)
    for case in CASES:
        sp = SamplingParams(1.2, 50, 0.9, 4, **case)
        args = (torch.from_numpy(lg).cuda(), torch.from_numpy(heads).cuda(), sp, torch.from_numpy(steps).cuda(), V, Tv, Sv)
        assert torch.equal(ops.sample(*args, element="f16"), ops.sample(*args, element="bf16")), case


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


def test_generate_graph_eager_and_stepwise_agree(tiny):
    cfg, eng, vids, ts, ids = tiny
    sp = SamplingParams(1.3, 50, 0.95, 2024, min_p=0.05, typical_p=0.8, epsilon_cutoff=1e-3, eta_cutoff=5e-3)
    g, hg = eng.generate(vids, ts, ids, [1] * 4, 20, sampling=sp, use_graph=True)
    e, he = eng.generate(vids, ts, ids, [1] * 4, 20, sampling=sp, use_graph=False)
    assert g == e and hg == he
    assert len({tuple(r) for r in g}) > 1                      # rows draw from their own counters
    for b in range(4):                                         # the stepwise host loop (what stopping criteria take): ids picked by trace_op_sample_ex
        eng.encode_video(vids[b], ts[b])
        eng.prefill(b, eng.splice(ids[b]))
    s = eng.decode_stepwise(range(4), [1] * 4, 20, sampling=sp)
    assert s[0] == g and s[1] == hg
    # min_p = 1 keeps the tokens as probable as the top one: the sampled run is the greedy run, so the warper does run inside the captured step
    greedy, _ = eng.generate(vids[:2], ts[:2], ids[:2], [1, 1], 16)
    assert greedy == eng.generate(vids[:2], ts[:2], ids[:2], [1, 1], 16, sampling=SamplingParams(1.5, 50, 1.0, 9, min_p=1.0))[0]
    # the model level: HF's arguments, the seed from torch's generator; graph replay twice and the stepwise host loop (stopping criteria)
    m = _model(cfg, eng)
    kw = dict(images_or_videos=vids, video_timestamps=ts, max_new_tokens=20, do_sample=True, temperature=0.9, top_k=40, top_p=0.9,
              min_p=0.1, typical_p=0.7, eos_token_id=-1)
    for extra in ({}, dict(epsilon_cutoff=0.01, eta_cutoff=0.05)):
        torch.manual_seed(3)
        a = m.generate(torch.tensor(ids), heads=[1] * 4, **kw, **extra)
        torch.manual_seed(3)
        b = m.generate(torch.tensor(ids), heads=[1] * 4, **kw, **extra)
        torch.manual_seed(3)
        c = m.generate(torch.tensor(ids), heads=[1] * 4, stopping_criteria=[lambda ids_, scores: torch.zeros(4, dtype=torch.bool)], **kw, **extra)
        assert torch.equal(a, b) and torch.equal(a, c), (extra, a, c)
        torch.manual_seed(3)
        sp = m._sampling_params(True, 0.9, 40, 0.9, None, dict(min_p=0.1, typical_p=0.7, **extra))
        assert a.tolist() == eng.generate(vids, ts, ids, [1] * 4, 20, sampling=sp)[0]          # and the engine call with the same parameters and seed
    # min_p = 1 through generate() is the greedy call; a generation_config brings typical_p in as well
    kw = dict(images_or_videos=vids[:2], video_timestamps=ts[:2], max_new_tokens=16, eos_token_id=-1)
    greedy = m.generate(torch.tensor(ids[:2]), heads=[1, 1], do_sample=False, **kw)
    assert torch.equal(greedy, m.generate(torch.tensor(ids[:2]), heads=[1, 1], do_sample=True, temperature=1.5, top_k=50, min_p=1.0, **kw))
    gc = {"do_sample": True, "temperature": 1.2, "top_k": 50, "typical_p": 0.5, "min_p": 0.02}
    torch.manual_seed(8)
    x = m.generate(torch.tensor(ids[:2]), heads=[1, 1], generation_config=gc, **kw)
    torch.manual_seed(8)
    y = m.generate(torch.tensor(ids[:2]), heads=[1, 1], do_sample=True, temperature=1.2, top_k=50, typical_p=0.5, min_p=0.02, **kw)
    assert torch.equal(x, y)


def test_host_path_equals_device_path_and_sample_rows_host(tiny):
    cfg, eng, vids, ts, ids = tiny
    V, Tv, Sv = cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size
    host = SamplingParams(1.1, 0, 1.0, 5, min_p=0.05, typical_p=0.9)                # top_k off with a warper armed: the host statement of the rules
    assert not host.on_device
    a, _ = eng.generate(vids[:2], ts[:2], ids[:2], [1, 1], 12, sampling=host)
    # top_k = 1024 keeps the whole of every head of the tiny model as well: the same rules, on the device
    b, _ = eng.generate(vids[:2], ts[:2], ids[:2], [1, 1], 12, sampling=dataclasses.replace(host, top_k=1024))
    assert a == b
    lg, heads = _rows(32, V, Tv, Sv, np.random.RandomState(3), "mixed")
    steps = list(range(32))
    assert eng.sample(torch.from_numpy(lg).cuda(), heads.tolist(), host, steps) == sample_rows_host(lg, heads.tolist(), V, Tv, Sv, host, steps)


def test_generate_samples_equals_generate_of_the_repeated_prompt(tiny):
    cfg, eng, vids, ts, ids = tiny
    sp = SamplingParams(1.2, 50, 1.0, 77, min_p=0.08)
    want = eng.generate([vids[0]] * 4, [ts[0]] * 4, [ids[0]] * 4, [1] * 4, 16, sampling=sp)
    got = eng.generate_samples(vids[0], ts[0], ids[0], 1, 4, 16, sampling=sp)
    assert got[0] == want[0] and got[1] == want[1]
