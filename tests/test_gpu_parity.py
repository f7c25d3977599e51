"""End-to-end parity of the HIP path (through the C ABI) against the oracle and the golden vectors captured
from the reference, at the tiny geometry the oracle finishes in seconds.

Tolerances (stated here once): the GPU path stores bf16 between kernels (2^-8 relative per rounding) and
accumulates in fp32.  Against the bf16-emulating oracle (same rounding points) activations agree to a few
bf16 ulps: atol 3e-2 / rtol 3e-2 on O(1) activations; against the fp32 reference fixtures the budget is the
accumulated bf16 noise of the whole stack: logits within 0.15 absolute (logit std ~1.3).  Token ids: the greedy
arg-max must equal the reference's wherever the reference's own top-2 margin exceeds that logit budget; the
13-way time/score heads are additionally checked bit-exact against the bf16-emulating oracle at every step."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from oracle import trace_oracle as O  # noqa: E402  (checker only)
from trace_amd import config as tcfg, synth  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402

ACT_ATOL, ACT_RTOL = 3e-2, 3e-2
LOGIT_TOL = 0.15


def report(name, got, ref, atol, rtol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    frac = bad.float().mean().item()
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    # allow a tiny fraction of 1-ulp flips of bf16 roundings that amplify through later layers
    assert frac < 2e-3 and err.max().item() < 20 * (atol + rtol * ref.abs().max().item()), (
        f"{name}: {frac:.4%} elements off, max err {err.max().item():.4g}, ref max {ref.abs().max().item():.4g}, "
        f"first bad {torch.nonzero(bad)[0].tolist() if bad.any() else None}")


@pytest.fixture(scope="module")
def setup(golden_dir):
    cfg = tcfg.tiny(num_frames=4)
    sd = synth.state_dict(cfg)
    eng = TraceEngine(cfg, max_batch=4, max_ctx=256, max_frames=4, max_new_tokens=64)
    eng.load_weights(sd.items())
    ora = O.Oracle(cfg, sd, emulate_bf16=True)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    return cfg, eng, ora, E, frames


def test_vit_features(setup):
    cfg, eng, ora, E, frames = setup
    got = eng.vit_forward(frames)
    report("vit vs oracle(bf16)", got, ora.vit_forward(frames.float()), ACT_ATOL, ACT_RTOL)
    report("vit vs reference fixture", got, torch.from_numpy(E["vit_feats"]), 6e-2, 6e-2)


def test_slot_pool(setup):
    cfg, eng, ora, E, frames = setup
    feats = ora.vit_forward(frames.float())
    got = eng.slot_pool(feats.to(torch.bfloat16), frames.shape[0])
    report("slot pool vs oracle(bf16)", got, ora.slot_pool(feats), ACT_ATOL, ACT_RTOL)
    eng.vit_forward(frames)
    got2 = eng.slot_pool(None, frames.shape[0])
    report("slot pool (internal feats) vs reference fixture", got2, torch.from_numpy(E["slots"]), 6e-2, 6e-2)


def test_encode_splice_prefill(setup):
    cfg, eng, ora, E, frames = setup
    ts = E["timestamps"].tolist()
    vid = eng.encode_video(frames, ts, want_output=True)
    ref_vid = ora.encode_video(frames.float(), ts)
    report("video rows", vid, ref_vid, ACT_ATOL, ACT_RTOL)
    # time-token rows are pure gathers: bit exact
    T, S = frames.shape[0], cfg.num_slots
    v3 = vid.view(T, cfg.tokens_per_frame, -1).float().cpu()
    r3 = ref_vid.view(T, cfg.tokens_per_frame, -1)
    assert torch.equal(v3[:, S:], r3[:, S:].to(torch.bfloat16).float())
    ids = E["input_ids"].tolist()
    L, emb = eng.splice(ids, want_output=True)
    assert L == int(E["prefill_len"])
    ref_emb = ora.splice(torch.tensor(ids), ref_vid)
    report("spliced embeds", emb, ref_emb, ACT_ATOL, ACT_RTOL)
    text_rows = [i for i in range(L) if not (10 <= i < 10 + T * cfg.tokens_per_frame)]
    assert torch.equal(emb[text_rows].float().cpu(), ref_emb[text_rows].to(torch.bfloat16).float())
    hid = eng.prefill(0, L, want_hidden=True)
    ref_hid, _ = ora.llm_forward(ref_emb)
    report("prefill hidden", hid, ref_hid, 5e-2, 5e-2)
    report("prefill hidden vs reference fixture", hid[-4:], torch.from_numpy(E["hidden_last_rows"]), 0.12, 0.1)


def _run_forced(eng, cfg, E, frames, forced, use_graph):
    ts = E["timestamps"].tolist()
    eng.encode_video(frames, ts)
    L = eng.splice(E["input_ids"].tolist())
    eng.prefill(1, L)
    n = len(forced) + 1
    logits = [eng.decode_begin([1], [1], n, eos=-1, forced=[forced], want_logits=True).cpu()]
    if use_graph:
        eng.decode_steps(n - 1, use_graph=True)
    else:
        for _ in range(n - 1):
            logits.append(eng.decode_steps(1, use_graph=False, want_logits=True).cpu())
    ids, heads = eng.decode_read()
    return ids[0], (torch.cat(logits) if len(logits) > 1 else None)


def test_teacher_forced_logits_and_ids(setup):
    cfg, eng, ora, E, frames = setup
    forced = E["forced_ids"].tolist()
    ids, lg = _run_forced(eng, cfg, E, frames, forced, use_graph=False)
    ref_lg = torch.from_numpy(E["tf_logits"])
    ref_ids = E["tf_argmax"].tolist()
    assert len(ids) == len(ref_ids)
    fin = torch.isfinite(ref_lg)
    assert torch.equal(torch.isfinite(lg), fin), "head mask (-inf pattern) differs from the reference"
    err = (lg[fin] - ref_lg[fin]).abs().max().item()
    assert err < LOGIT_TOL, f"logits differ from the reference fixture by {err}"
    # ids: must match wherever the reference margin exceeds the logit budget
    srt = torch.sort(torch.where(fin, ref_lg, torch.full_like(ref_lg, -1e30)), dim=-1, descending=True).values
    margin = (srt[:, 0] - srt[:, 1]).tolist()
    checked = 0
    for i, (a, b, m) in enumerate(zip(ids, ref_ids, margin)):
        if m > 2 * LOGIT_TOL:
            assert a == b, f"step {i}: id {a} != reference {b} (margin {m:.3f})"
            checked += 1
    assert checked >= len(ref_ids) // 2
    # bf16-emulating oracle: time/score-head steps must be bit-exact token ids
    o_ids, o_lg = ora.generate(torch.from_numpy(E["input_ids"]), frames.float(), E["timestamps"].tolist(), head=1,
                               max_new_tokens=len(forced) + 1, forced_ids=forced, return_logits=True)
    V = cfg.vocab_size
    osrt = torch.sort(torch.where(torch.isfinite(o_lg), o_lg, torch.full_like(o_lg, -1e30)), dim=-1, descending=True).values
    for i, (a, b) in enumerate(zip(ids, o_ids)):
        if b > V and (osrt[i, 0] - osrt[i, 1]) > 0.02:
            assert a == b, f"step {i}: time/score id {a} != oracle {b}"
    e2 = (lg[fin] - o_lg[fin]).abs().max().item()
    assert e2 < 0.08, f"logits differ from the bf16-emulating oracle by {e2}"


def test_prefill_last_layer_rows_shortcut_is_bit_identical(setup):
    """Round 6: with no hidden rows requested, the last decoder layer computes K / V for every row but q, attention, o-proj and the MLP only for each
    prompt's last row (engine.hip prefill_impl; the reference runs all L rows, trace_mistral.py:190-200, and keeps logits[:, -1]).  Same kernels, same
    K order: the first logits AND the decode steps that follow (they read the layer's K / V rows) must be bit-identical to the full layer, for a
    single prompt, a pair and a run of four."""
    from trace_amd.engine import ops
    cfg, _, ora, E, frames = setup
    eng = TraceEngine(cfg, max_batch=4, max_ctx=256, max_frames=4, max_new_tokens=16)       # (its own engine: it prefills all four KV slots)
    eng.load_weights(synth.state_dict(cfg).items())
    ts = E["timestamps"].tolist()
    eng.encode_video(frames, ts)
    L, emb = eng.splice(E["input_ids"].tolist(), want_output=True)
    embs = [emb.clone(), (emb.float() * 0.5).to(emb.dtype), (emb.float() * -0.25).to(emb.dtype), (emb.float() * 0.75).to(emb.dtype)]
    res = {}
    for mode in (0, 1):
        with ops.tuned(prefill__last_rows=mode):
            out = []
            for nb in (1, 2, 4):
                if nb == 1:
                    eng.prefill(0, L, embeds=embs[0])
                elif nb == 2:
                    eng.prefill_pair(0, embs[0], embs[1])
                else:
                    eng.prefill_multi(0, embs)
                lg = [eng.decode_begin(list(range(nb)), [1] * nb, 8, eos=-1, want_logits=True).clone()]
                for _ in range(3):
                    lg.append(eng.decode_steps(1, use_graph=False, want_logits=True).clone())
                out.append(torch.stack(lg))
            res[mode] = out
    eng.close()
    for a, b in zip(res[0], res[1]):
        assert torch.isfinite(a[torch.isfinite(b)]).all()
        assert torch.equal(a, b), f"last-rows prefill differs from the full last layer: max |d| {(a - b)[torch.isfinite(a)].abs().max().item()}"


def test_prefill_run_of_eight_equals_each_prompt_alone(setup):
    """Round 6: trace_llm_prefill_multi takes up to 8 equal-length prompts while n x L fits the prefill workspaces (max(4 max_ctx, min(8192, 8 max_ctx)) rows).
    A prompt's result must not depend on how many neighbours share its pass: the first logits and three decode steps of a run of eight, of seven and of five are
    bit-identical to each prompt prefilled alone.  One prompt too many for the workspace is a TRACE_ERR_ARG, not a crash; the host's choice of the run length
    (TraceEngine.prefill_group) is 4 at the C2 prompt length and 7 at the C4 one."""
    from trace_amd import _lib
    cfg, _, ora, E, frames = setup
    eng = TraceEngine(cfg, max_batch=8, max_ctx=256, max_frames=4, max_new_tokens=16)
    eng.load_weights(synth.state_dict(cfg).items())
    eng.encode_video(frames, E["timestamps"].tolist())
    L, emb = eng.splice(E["input_ids"].tolist(), want_output=True)
    assert eng.prefill_rows == 2048 and 8 * L <= eng.prefill_rows
    embs = [(emb.float() * f).to(emb.dtype) for f in (1.0, 0.5, -0.25, 0.75, -1.0, 0.3, 1.25, -0.6)]

    def run(slots):
        lg = [eng.decode_begin(slots, [1] * len(slots), 8, eos=-1, want_logits=True).clone()]
        for _ in range(3):
            lg.append(eng.decode_steps(1, use_graph=False, want_logits=True).clone())
        return torch.stack(lg)                     # [4 steps, len(slots), NV]

    alone = []
    for b in range(8):
        eng.prefill(0, L, embeds=embs[b])
        alone.append(run([0])[:, 0])
    for n in (8, 7, 5):
        eng.prefill_multi(0, embs[:n])
        got = run(list(range(n)))
        for b in range(n):
            assert torch.equal(got[:, b], alone[b]), (n, b)
    big = TraceEngine(cfg, max_batch=8, max_ctx=2048, max_frames=4, max_new_tokens=8)       # 4 x 2048 = 8192 rows: four 2000-row prompts fit, five do not
    try:
        big.load_weights(synth.state_dict(cfg).items())
        assert big.prefill_rows == 8192
        long_embs = [(torch.randn(2000, cfg.hidden_size, device="cuda") * 0.02).to(emb.dtype) for _ in range(5)]
        big.prefill_multi(0, long_embs[:4])
        with pytest.raises(AssertionError):
            big.prefill_multi(0, long_embs)                                                  # the host wrapper refuses ...
        import ctypes as C
        ptrs = (C.c_void_p * 5)(*[e.data_ptr() for e in long_embs])
        with pytest.raises(_lib.TraceHipError, match="prefill workspace"):                   # ... and so does the library (TRACE_ERR_ARG through errcheck)
            big.lib.trace_llm_prefill_multi(big.h, 0, ptrs, 5, 2000, None)
    finally:
        big.close()
    eng.close()
    # the host's rule at the benchmark prompt lengths (7B widths; no device work)
    class _E(TraceEngine):
        def __init__(self, cfg_, max_ctx):
            self.cfg, self.max_ctx = cfg_, max_ctx
        def __del__(self):
            pass
    c7 = tcfg.trace_7b(128)
    assert _E(c7, 2240).prefill_group(1967) == 4 and _E(c7, 1152).prefill_group(1086) == 7 and _E(c7, 3904).prefill_group(3834) == 4


def test_graph_replay_equals_eager(setup):
    cfg, eng, ora, E, frames = setup
    forced = E["forced_ids"].tolist()
    ids_e, _ = _run_forced(eng, cfg, E, frames, forced, use_graph=False)
    ids_g, _ = _run_forced(eng, cfg, E, frames, forced, use_graph=True)
    assert ids_e == ids_g


def test_free_run_matches_reference(setup):
    cfg, eng, ora, E, frames = setup
    ref_ids = E["free_ids"].tolist()
    ref_lg = torch.from_numpy(E["free_logits"])
    out, heads = eng.generate([frames], [E["timestamps"].tolist()], [E["input_ids"].tolist()], [1], len(ref_ids))
    ids = out[0]
    fin = torch.isfinite(ref_lg)
    srt = torch.sort(torch.where(fin, ref_lg, torch.full_like(ref_lg, -1e30)), dim=-1, descending=True).values
    margin = (srt[:, 0] - srt[:, 1]).tolist()
    for i, (a, b, m) in enumerate(zip(ids, ref_ids, margin)):
        if m <= 2 * LOGIT_TOL:
            break          # past a low-margin step the two greedy streams may legitimately diverge
        assert a == b, f"step {i}: {a} != {b}"
    assert i >= 8


def test_batched_decode_equals_single(setup):
    """Two different videos decoded together (B=2) give the same ids as each alone (B=1)."""
    cfg, eng, ora, E, frames = setup
    f2 = synth.synth_frames(cfg, 1).to(torch.bfloat16)
    ts, ids = E["timestamps"].tolist(), E["input_ids"].tolist()
    n = 24
    a, _ = eng.generate([frames], [ts], [ids], [1], n)
    b, _ = eng.generate([f2], [ts], [ids], [1], n)
    ab, _ = eng.generate([frames, f2], [ts, ts], [ids, ids], [1, 1], n)
    assert ab[0] == a[0] and ab[1] == b[0]
    E1 = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_video1.npz"))
    ref = E1["free_ids"].tolist()
    assert b[0][:4] == ref[:4]


def test_errors_are_python_exceptions(setup):
    cfg, eng, ora, E, frames = setup
    from trace_amd._lib import TraceHipError
    with pytest.raises(TraceHipError, match="only have one video"):
        eng.splice([1, 5, 6, -205])
    with pytest.raises(TraceHipError):
        eng.decode_begin([3], [1], 8)          # slot never prefilled
    with pytest.raises(AssertionError):
        eng.time_ids([[1.0], [2.0, 3.0]])       # unequal time-token length (trace_arch.py:285)


@pytest.mark.parametrize("nb", [20, 40, 64, 65, 100, 128, 200, 256])
def test_big_batch_equals_single(setup, nb):
    """B > 16 / B > 32 exercise the two- and four-group decode GEMV (NB = 2, 4) and the second head pass; B > 64 the wide decode step
    (projections as small-M MFMA GEMMs: gate|up with the SwiGLU epilogue, qkv / o / down as split-K partial rows; four head passes at
    128, two row panels of GEMM tiles and eight head passes at 256): nb sequences (two distinct videos, alternating) must reproduce the B = 1
    streams — through the captured hipGraph (one per batch size, up to the 256-row maximum) and through eager launches."""
    cfg, eng, ora, E, frames = setup
    f2 = synth.synth_frames(cfg, 1).to(torch.bfloat16)
    ts, ids = E["timestamps"].tolist(), E["input_ids"].tolist()
    n = 16
    a, _ = eng.generate([frames], [ts], [ids], [1], n)
    b, _ = eng.generate([f2], [ts], [ids], [1], n)
    big = TraceEngine(cfg, max_batch=nb, max_ctx=192, max_frames=4, max_new_tokens=32)
    big.load_weights(synth.state_dict(cfg).items())
    vids = [frames if i % 2 == 0 else f2 for i in range(nb)]
    out, _ = big.generate(vids, [ts] * nb, [ids] * nb, [1] * nb, n, use_graph=True)
    for i in range(nb):
        assert out[i] == (a[0] if i % 2 == 0 else b[0]), i
    out_e, _ = big.generate(vids, [ts] * nb, [ids] * nb, [1] * nb, n, use_graph=False)
    assert out_e == out
    big.close()


def test_tower_over_frame_stream_equals_per_video(setup):
    """Several videos' frames pushed through the ViT `vit_batch_frames` at a time, chunks spanning video boundaries (4 + 2 + 4
    frames in chunks of 5): features, and the [slots | time] rows built from them, are bit-identical to per-video calls."""
    from trace_amd._lib import TraceHipError
    cfg, eng, ora, E, frames = setup
    e3 = TraceEngine(cfg, max_batch=3, max_ctx=192, max_frames=4, max_new_tokens=16, vit_batch_frames=5)
    e3.load_weights(synth.state_dict(cfg).items())
    vids = [frames, synth.synth_frames(cfg, 1, num_frames=2).to(torch.bfloat16), synth.synth_frames(cfg, 2).to(torch.bfloat16)]
    tss = [[[float(i) * 2.5] for i in range(v.shape[0])] for v in vids]
    many = e3.vit_forward_many(vids)
    for v, f, ts in zip(vids, many, tss):
        assert f.shape[0] == v.shape[0]
        assert torch.equal(f, e3.vit_forward(v))
        a = e3.encode_video(v, ts, want_output=True).clone()
        b = e3.encode_features(f.contiguous(), ts, want_output=True)
        assert torch.equal(a, b)
    with pytest.raises(TraceHipError, match="max_frames"):
        e3.encode_video(torch.cat([frames, frames[:1]]), [[0.0]] * 5)       # 5 frames fit the tower batch but not one video
    e3.close()


def test_ragged_batch_and_context_limits(setup):
    """Ragged batch: videos with different frame counts (2 vs 4 -> 28 vs 56 visual rows) and different prompt lengths decode
    together exactly as they do alone, and match the bf16-emulating oracle on the 13-way heads.  Context edge: a prompt
    whose prefill + max_new lands exactly on max_ctx is accepted; one token more is rejected with a Python exception."""
    cfg, eng, ora, E, frames = setup
    from trace_amd._lib import TraceHipError
    ids_a = E["input_ids"].tolist()
    ids_b = synth.synth_prompt_ids(cfg, n_text=37, video_pos=5, seed=11).tolist()
    fa, fb = frames, synth.synth_frames(cfg, 3).to(torch.bfloat16)[:2]
    ts_a, ts_b = E["timestamps"].tolist(), [[0.5], [7.25]]
    n = 12
    a, _ = eng.generate([fa], [ts_a], [ids_a], [1], n)
    b, _ = eng.generate([fb], [ts_b], [ids_b], [1], n)
    ab, heads = eng.generate([fa, fb], [ts_a, ts_b], [ids_a, ids_b], [1, 1], n)
    assert ab[0] == a[0] and ab[1] == b[0]
    o_ids, o_lg = ora.generate(torch.tensor(ids_b), fb.float(), ts_b, head=1, max_new_tokens=n, return_logits=True)
    srt = torch.sort(torch.where(torch.isfinite(o_lg), o_lg, torch.full_like(o_lg, -1e30)), dim=-1, descending=True).values
    for i, (x, y) in enumerate(zip(b[0], o_ids)):
        if (srt[i, 0] - srt[i, 1]) <= 0.05:
            break                                   # a near-tie: the two greedy streams may legitimately part here
        assert x == y, f"ragged video, step {i}: {x} != oracle {y}"
    assert i >= 3
    # context limit on an engine whose cache is exactly prompt + 8 tokens long
    L = int(E["prefill_len"])
    small = TraceEngine(cfg, max_batch=1, max_ctx=L + 8, max_frames=4, max_new_tokens=16)
    small.load_weights(synth.state_dict(cfg).items())
    small.encode_video(fa, ts_a)
    assert small.splice(ids_a) == L
    small.prefill(0, L)
    small.decode_begin([0], [1], 8, eos=-1)                        # exactly fills the cache
    small.decode_steps(7, use_graph=False)
    out, _ = small.decode_read()
    assert out[0] == a[0][:8]
    small.prefill(0, L)
    with pytest.raises(TraceHipError, match="exceeds max_ctx"):
        small.decode_begin([0], [1], 9, eos=-1)
    small.close()


def test_vit_large_geometry_three_distinct_frames_vs_reference_fixture(golden_dir):
    """Real CLIP-ViT-L/14-336 geometry, THREE DISTINCT frames (tests/golden/medium_vit_multi.npz: the reference's own tower + slot pool on them in one call): the HIP
    tower on the three frames, and on a 24-frame stream that holds each of them eight times in a shuffled order (the 256 x 256 GEMM tiles and the 192-row
    attention: the path the product runs).  Every copy inside the one-frame test's budget against the reference; the copies of a frame bit-identical wherever
    they sit in the stream and whatever their neighbours are."""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=3), vision_hidden_size=1024, vision_intermediate_size=4096, vision_num_layers=24,
                              vision_num_heads=16, vision_image_size=336, vision_patch_size=14, mm_hidden_size=1024)
    M = np.load(os.path.join(golden_dir, "medium_vit_multi.npz"))
    rows = torch.from_numpy(M["feat_rows"]).long()
    ref = torch.from_numpy(M["vit_feats_rows"].astype(np.float32))           # [3, 24, 1024]
    ref_norm = torch.from_numpy(M["feat_norm"])
    rs = torch.from_numpy(M["slots"].astype(np.float32))                     # [3, 8, 4096]
    amean = float(M["feat_abs_mean"])
    sd = synth.state_dict(cfg)
    frames = synth.synth_frames(cfg, int(M["video_idx"]), num_frames=3).to(torch.bfloat16)
    eng = TraceEngine(cfg, max_batch=1, max_ctx=512, max_frames=24, max_new_tokens=8)
    eng.load_weights(sd.items())

    def check(f, tag):
        e = (f[:, rows] - ref).abs()
        # relative L2 over the sampled rows (the full-tensor norms of the reference are in the fixture: the sampled rows are a 24th of each frame)
        rl2 = ((f[:, rows] - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max().item()
        print(f"{tag}: max {e.max().item():.4f} mean {e.mean().item():.5f} rel L2 {rl2:.5f}")
        assert torch.isfinite(f).all()
        assert e.max().item() < 0.5 and e.mean().item() < 0.02 * amean and rl2 < 0.02, (tag, e.max().item(), e.mean().item(), rl2)
        assert torch.allclose(f.flatten(1).norm(dim=1), ref_norm, rtol=2e-2)

    f3 = eng.vit_forward(frames).float().cpu()
    check(f3, "three frames")
    slots = eng.slot_pool(None, 3).float().cpu().reshape(3, 8, -1)
    es = (slots - rs).abs()
    print("slots: max err", es.max().item(), "ref max", rs.abs().max().item())
    assert es.max().item() < 0.05 * max(1.0, rs.abs().max().item()), (es.max().item(), rs.abs().max().item())
    order = torch.tensor([0, 1, 2, 2, 0, 1, 1, 2, 0, 0, 0, 1, 2, 2, 1, 1, 0, 2, 2, 1, 0, 1, 0, 2])
    f24 = eng.vit_forward(frames[order].contiguous()).float().cpu()
    for k in range(3):
        idx = (order == k).nonzero().flatten().tolist()
        assert len(idx) == 8 and all(torch.equal(f24[idx[0]], f24[i]) for i in idx[1:]), k
    check(torch.stack([f24[(order == k).nonzero()[0, 0]] for k in range(3)]), "24-frame shuffled stream")
    eng.close()


def test_vit_large_geometry_vs_reference_fixture(golden_dir):
    """The real CLIP-ViT-L/14-336 geometry (1024 wide, 23 of 24 layers, 16 heads, 577 tokens) for one frame: HIP ViT + slot
    pool against the fixture captured from the reference's own vision tower + SpatialSlotPool (tests/golden/medium_vit.npz)
    and against the bf16-emulating oracle.  Features are O(2) (max 12.7); 46 bf16-rounded residual updates put the HIP path
    within 0.5 abs / 2 % mean (relative L2 < 2 %) of the fp32 reference."""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=1), vision_hidden_size=1024, vision_intermediate_size=4096, vision_num_layers=24,
                              vision_num_heads=16, vision_image_size=336, vision_patch_size=14, mm_hidden_size=1024)
    M = np.load(os.path.join(golden_dir, "medium_vit.npz"))
    sd = synth.state_dict(cfg)
    eng = TraceEngine(cfg, max_batch=1, max_ctx=256, max_frames=1, max_new_tokens=8)
    eng.load_weights(sd.items())
    frames = synth.synth_frames(cfg, int(M["video_idx"]), num_frames=1).to(torch.bfloat16)
    feats = eng.vit_forward(frames).float().cpu()[0]
    ref = torch.from_numpy(M["vit_feats"].astype(np.float32))
    err = (feats - ref).abs()
    assert torch.isfinite(feats).all()
    print("vs fp32 reference: max", err.max().item(), "mean", err.mean().item(), "ref abs mean", ref.abs().mean().item())
    assert err.max().item() < 0.5 and err.mean().item() < 0.02 * ref.abs().mean().item(), (err.max().item(), err.mean().item())
    ora = O.Oracle(cfg, {k: v for k, v in sd.items() if "vision_tower" in k or "mm_projector" in k}, emulate_bf16=True)
    of = ora.vit_forward(frames.float())
    e2 = (feats - of.reshape(ref.shape)).abs()
    print("vs bf16 oracle: max", e2.max().item(), "mean", e2.mean().item())
    # two bf16 implementations that sum in different orders round differently at every layer: after 23 layers they are as far
    # from each other as from the fp32 reference (measured: mean 0.025 = 1.2 %, max 0.25-0.32), so the same budget applies
    assert e2.max().item() < 0.5 and e2.mean().item() < 0.02 * ref.abs().mean().item(), (e2.max().item(), e2.mean().item())
    rel_l2 = (feats - ref).norm().item() / ref.norm().item()
    assert rel_l2 < 0.02, rel_l2
    slots = eng.slot_pool(None, 1).float().cpu()[0]
    rs = torch.from_numpy(M["slots"])
    es = (slots - rs).abs()
    print("slots: max err", es.max().item(), "ref max", rs.abs().max().item())
    assert es.max().item() < 0.05 * max(1.0, rs.abs().max().item()), (es.max().item(), rs.abs().max().item())
    eng.close()
    # From ~20 frames up every shape of the tower runs on the 256x256 kernels (persistent GEMMs, the big-tile attention blocks).  The fixture's
    # frame 24 times over takes that path: every copy must stay inside the same budget against the reference's fp32 features, and the copies of a
    # frame agree with each other bit for bit (per-frame arithmetic: no result may depend on where in the stream a frame sits).
    eng = TraceEngine(cfg, max_batch=1, max_ctx=512, max_frames=24, max_new_tokens=8)
    eng.load_weights(sd.items())
    many = frames.expand(24, -1, -1, -1).contiguous()
    f = eng.vit_forward(many).float().cpu()
    assert all(torch.equal(f[0], f[i]) for i in range(1, 24))
    e = (f[0] - ref).abs()
    rl2 = (f[0] - ref).norm().item() / ref.norm().item()
    print(f"24 frames: max {e.max().item():.4f} mean {e.mean().item():.5f} rel L2 {rl2:.5f}")
    assert e.max().item() < 0.5 and e.mean().item() < 0.02 * ref.abs().mean().item() and rl2 < 0.02, (e.max().item(), e.mean().item(), rl2)
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "parity_measured.txt"), "a") as fh:
            fh.write(f"ViT-L/14-336 real geometry, 24 frames: rel L2 vs reference {rl2:.5f}, max {e.max().item():.4f}\n")
    eng.close()


def test_real_width_decoder_layer_vs_reference_fixture(golden_dir):
    """One decoder layer at the real Mistral-7B widths (hidden 4096, intermediate 14336): teacher-forced decode through the
    HIP path (K = 14336 down-projection in 4-16 chunks of partial rows, 28672-wide gate|up) against logits captured from the
    reference (tests/golden/medium_llm.npz) — alone (B = 1) and inside batches of 20 and 40 copies (two and four MFMA row groups)."""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), intermediate_size=14336, num_hidden_layers=1)
    M = np.load(os.path.join(golden_dir, "medium_llm.npz"))
    eng = TraceEngine(cfg, max_batch=128, max_ctx=192, max_frames=4, max_new_tokens=64)
    eng.load_weights(synth.state_dict(cfg).items())
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    forced, ref_lg, ref_ids = M["forced_ids"].tolist(), torch.from_numpy(M["tf_logits"]), M["tf_argmax"].tolist()
    n = len(forced) + 1
    fin = torch.isfinite(ref_lg)
    srt = torch.sort(torch.where(fin, ref_lg, torch.full_like(ref_lg, -1e30)), dim=-1, descending=True).values
    margin = (srt[:, 0] - srt[:, 1]).tolist()
    for nb in (1, 20, 40, 128):        # 128: the wide decode step (K = 14336 down-projection as an 8-chunk split-K GEMM, fused-SwiGLU gate|up GEMM)
        for b in range(nb):
            eng.encode_video(frames, M["timestamps"].tolist())
            eng.prefill(b, eng.splice(M["input_ids"].tolist()))
        lgs = [eng.decode_begin(list(range(nb)), [1] * nb, n, eos=-1, forced=[forced] * nb, want_logits=True).float().cpu()]
        for _ in range(n - 1):
            lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
        ids, _ = eng.decode_read()
        for b in (0, nb - 1):
            lg = torch.stack([x[b] for x in lgs])
            assert torch.equal(torch.isfinite(lg), fin)
            err = (lg[fin] - ref_lg[fin]).abs().max().item()
            assert err < LOGIT_TOL, (nb, b, err)
            for i, (a, r, m) in enumerate(zip(ids[b], ref_ids, margin)):
                if m > 2 * LOGIT_TOL:
                    assert a == r, (nb, b, i, a, r, m)
    eng.close()


def test_deep_real_width_stack_vs_reference_fixture(golden_dir):
    """Depth: eight decoder layers at the real Mistral-7B widths (1.7 B parameters, a quarter of the real stack), teacher-forced
    decode against logits captured from the reference (tests/golden/deep_llm.npz), at B = 1 and inside a batch of 40.  Shows the
    bf16 noise of the HIP path (bf16 weights, activations and KV cache; fp32 accumulation) stays inside the logit tolerance as
    layers stack, and that wherever the reference's top-2 margin exceeds twice the tolerance the greedy id is the reference's."""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), intermediate_size=14336, num_hidden_layers=8)
    M = np.load(os.path.join(golden_dir, "deep_llm.npz"))
    eng = TraceEngine(cfg, max_batch=100, max_ctx=192, max_frames=4, max_new_tokens=64)
    eng.load_weights(synth.iter_weights(cfg))
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    forced, ref_lg, ref_ids = M["forced_ids"].tolist(), torch.from_numpy(M["tf_logits"]), M["tf_argmax"].tolist()
    n = len(forced) + 1
    fin = torch.isfinite(ref_lg)
    srt = torch.sort(torch.where(fin, ref_lg, torch.full_like(ref_lg, -1e30)), dim=-1, descending=True).values
    margin = (srt[:, 0] - srt[:, 1]).tolist()
    for nb in (1, 40, 100):            # 100: the wide decode step (batches above 64) through eight layers
        for b in range(nb):
            eng.encode_video(frames, M["timestamps"].tolist())
            eng.prefill(b, eng.splice(M["input_ids"].tolist()))
        lgs = [eng.decode_begin(list(range(nb)), [1] * nb, n, eos=-1, forced=[forced] * nb, want_logits=True).float().cpu()]
        for _ in range(n - 1):
            lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
        ids, _ = eng.decode_read()
        for b in (0, nb - 1):
            lg = torch.stack([x[b] for x in lgs])
            assert torch.equal(torch.isfinite(lg), fin)
            err = (lg[fin] - ref_lg[fin]).abs().max().item()
            print("deep stack nb=%d b=%d max |dlogit| %.4f" % (nb, b, err))
            assert err < LOGIT_TOL, (nb, b, err)
            for i, (a, r, m) in enumerate(zip(ids[b], ref_ids, margin)):
                if m > 2 * LOGIT_TOL:
                    assert a == r, (nb, b, i, a, r, m)
            if b == 0:        # the reference's own bf16 run of this stream (deep_llm.npz:tf_logits_ref_bf16): 0.265 max / 0.057 rms from its fp32 run
                from conftest import bf16_anchor_report
                r8 = bf16_anchor_report(lg, M, f"8 real-width layers, batch {nb}, bf16 anchor")
                assert r8["hip_rms"] <= r8["ref_bf16_rms"] and r8["hip_max"] <= r8["ref_bf16_max"], r8
                assert r8["hip_flips_13way"] <= r8["ref_bf16_flips_13way"] + 2, r8
    eng.close()


def test_c2_context_length_vs_reference_fixture(golden_dir):
    """The C2 context: 128 frames -> prefill L = 1967, one real-width decoder layer, teacher-forced decode at contexts
    1968.. against logits captured from the reference (tests/golden/long_ctx.npz).  Exercises the causal prefill attention
    and the 256x256-tile GEMMs at M ~ 2k (single and paired prefill), and the decode attention over a 2k-token cache with
    the split counts of batch 1 and batch 20."""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=128), intermediate_size=14336, num_hidden_layers=1)
    M = np.load(os.path.join(golden_dir, "long_ctx.npz"))
    eng = TraceEngine(cfg, max_batch=20, max_ctx=2048, max_frames=128, max_new_tokens=32)
    eng.load_weights(synth.state_dict(cfg).items())
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    ts, ids = M["timestamps"].tolist(), M["input_ids"].tolist()
    forced, ref_lg = M["forced_ids"].tolist(), torch.from_numpy(M["tf_logits"])
    n = len(forced) + 1
    fin = torch.isfinite(ref_lg)
    for nb in (1, 20):
        eng.encode_video(frames, ts)
        L, emb = eng.splice(ids, want_output=True)
        assert L == int(M["prefill_len"]) == 1967
        if nb == 1:
            eng.prefill(0, L)
        else:
            for b in range(0, nb, 2):
                eng.prefill_pair(b, emb, emb)                      # paired prefill: M = 3934
        lgs = [eng.decode_begin(list(range(nb)), [1] * nb, n, eos=-1, forced=[forced] * nb, want_logits=True).float().cpu()]
        for _ in range(n - 1):
            lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
        for b in (0, nb - 1):
            lg = torch.stack([x[b] for x in lgs])
            assert torch.equal(torch.isfinite(lg), fin)
            err = (lg[fin] - ref_lg[fin]).abs().max().item()
            assert err < LOGIT_TOL, (nb, b, err)
    eng.close()


def test_real_vocabulary_vs_reference_fixture(golden_dir):
    """The real vocabulary: 32000-row lm_head (2002 head tiles), <sync> at 32000, time ids 32001.., score ids 32014..: teacher-
    forced decode against the reference's logits (tests/golden/real_vocab.npz: sampled columns, top-2, finite counts), alone
    and in a batch of 40 (two passes of the head kernel)."""
    import dataclasses
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), vocab_size=32000)
    M = np.load(os.path.join(golden_dir, "real_vocab.npz"))
    eng = TraceEngine(cfg, max_batch=40, max_ctx=192, max_frames=4, max_new_tokens=64)
    eng.load_weights(synth.state_dict(cfg).items())
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    ts, ids, forced = M["timestamps"].tolist(), M["input_ids"].tolist(), M["forced_ids"].tolist()
    cols = torch.from_numpy(M["cols"])
    ref_s, ref_top, ref_idx = torch.from_numpy(M["sampled"]), torch.from_numpy(M["top_val"]), M["top_idx"]
    n = len(forced) + 1
    for nb in (1, 40):
        for b in range(nb):
            eng.encode_video(frames, ts)
            eng.prefill(b, eng.splice(ids))
        lgs = [eng.decode_begin(list(range(nb)), [1] * nb, n, eos=-1, forced=[forced] * nb, want_logits=True).float().cpu()]
        for _ in range(n - 1):
            lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
        out, _ = eng.decode_read()
        for b in (0, nb - 1):
            lg = torch.stack([x[b] for x in lgs])
            assert torch.isfinite(lg).sum(-1).tolist() == M["finite_count"].tolist()          # 13 / 32001 active ids per step
            s = lg[:, cols]
            fin = torch.isfinite(ref_s)
            assert torch.equal(torch.isfinite(s), fin)
            assert (s[fin] - ref_s[fin]).abs().max().item() < LOGIT_TOL
            top = torch.topk(torch.where(torch.isfinite(lg), lg, torch.full_like(lg, -1e30)), 2, dim=-1)
            assert (top.values[:, 0] - ref_top[:, 0]).abs().max().item() < LOGIT_TOL
            for i in range(n):                                       # arg-max (the emitted id) wherever the reference margin allows
                if ref_top[i, 0] - ref_top[i, 1] > 2 * LOGIT_TOL:
                    assert out[b][i] == int(ref_idx[i, 0]), (nb, b, i)
    eng.close()


def test_batch1_swiglu_fold_is_bit_identical(golden_dir):
    """Round 4: at batch 1 the down GEMV does the SwiGLU combine itself while it parks its activations (decode.hip, SkinnyPro PRO = 2).  Same sums in
    the same order, same fp32 silu * up, one bf16 rounding: the logits of every teacher-forced step must equal the two-kernel form's bit for bit —
    at the real Mistral-7B MLP width (K = 14336 cut in chunks, two layers) and at the tiny geometry (one chunk)."""
    import dataclasses
    from trace_amd.engine import ops
    for cfg in (dataclasses.replace(tcfg.tiny(num_frames=4), intermediate_size=14336, num_hidden_layers=2), tcfg.tiny(num_frames=4)):
        M = np.load(os.path.join(golden_dir, "medium_llm.npz"))
        eng = TraceEngine(cfg, max_batch=1, max_ctx=192, max_frames=4, max_new_tokens=64)
        eng.load_weights(synth.iter_weights(cfg))
        frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
        forced = M["forced_ids"].tolist()[:20]
        n = len(forced) + 1
        runs = {}
        for fold in (1, 0):
            with ops.tuned(decode__fuse_swiglu=fold):
                eng.encode_video(frames, M["timestamps"].tolist())
                eng.prefill(0, eng.splice(M["input_ids"].tolist()))
                lgs = [eng.decode_begin([0], [1], n, eos=-1, forced=[forced], want_logits=True).float().cpu()]
                for _ in range(n - 1):
                    lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
                runs[fold] = (torch.stack(lgs), eng.decode_read()[0])
        assert torch.equal(runs[1][0], runs[0][0]), (runs[1][0] - runs[0][0]).abs().max()
        assert runs[1][1] == runs[0][1]
        eng.close()


@pytest.mark.parametrize("geometry", ["vit_l_14_336", "tiny"])
def test_fused_patch_embed_matches_three_pass_front_end(geometry):
    """Round 4: the ViT front end as one kernel — patches read straight from the frame tensor (no im2col matrix), MFMA GEMM, CLS / position
    embeddings and pre_layrnorm in the epilogue (patch_embed.hip) — against the round-1 path it replaces (im2col -> GEMM -> assemble,
    vit.patch_fused = 0).  Same rounding points, another fp32 summation order: through ONE encoder layer the features agree to a bf16
    ulp here and there.  Both frame dtypes the ABI takes (16-bit, fp32), a small call (128-wide tiles) and a 24-frame call (the 256-wide kernels)."""
    import dataclasses
    from trace_amd.engine import ops
    if geometry == "tiny":
        cfg = dataclasses.replace(tcfg.tiny(num_frames=24), vision_num_layers=2)
    else:
        cfg = dataclasses.replace(tcfg.tiny(num_frames=24), vision_hidden_size=1024, vision_intermediate_size=4096, vision_num_layers=2,
                                  vision_num_heads=16, vision_image_size=336, vision_patch_size=14, mm_hidden_size=1024)
    sd = synth.state_dict(cfg)
    eng = TraceEngine(cfg, max_batch=1, max_ctx=512, max_frames=24, max_new_tokens=8)
    eng.load_weights(sd.items())
    frames = torch.cat([synth.synth_frames(cfg, 50 + i, num_frames=8) for i in range(3)]).to(torch.bfloat16)          # 24 different frames
    ora = O.Oracle(cfg, {k: v for k, v in sd.items() if "vision_tower" in k}, emulate_bf16=True)
    want = ora.vit_forward(frames[:3].float()).reshape(3, cfg.vision_patches, cfg.vision_hidden_size)
    for n in (3, 24):
        got = {}
        for fused in (1, 0):
            with ops.tuned(vit__patch_fused=fused):
                got[fused] = eng.vit_forward(frames[:n]).float().cpu()
                if fused:
                    got["fp32 frames"] = eng.vit_forward(frames[:n].float()).float().cpu()
        assert torch.isfinite(got[1]).all()
        assert torch.equal(got[1], got["fp32 frames"]), n                    # bf16-representable pixels: the fp32 path rounds them back to the same bits
        d = (got[1] - got[0]).abs()
        scale = got[0].abs().mean().item()
        print(f"{geometry}, {n} frames: fused vs three-pass front end: max {d.max().item():.4f} mean {d.mean().item():.6f} (|x| mean {scale:.3f}), "
              f"identical {float((d == 0).float().mean()):.3f}")
        assert d.mean().item() < 2e-3 * max(scale, 1e-3) and d.max().item() < 0.1 * max(1.0, got[0].abs().max().item()), (n, d.max().item(), d.mean().item())
        e = (got[1][:3] - want).abs()
        assert (e > 3e-2 + 3e-2 * want.abs()).float().mean().item() < 2e-3, (n, e.max().item())
    eng.close()
