"""The engine with an e4m3 KV cache (TraceEngine(kv_cache="fp8"), trace_ctx_create_opts) next to the 16-bit-cache engine built from the same
synthetic weights: what is identical (a prefill of whole prompts, the bytes the cache then holds, the first appended row), what is deterministic
(graph replay, batches, slot copies, the public generate calls), what the cache costs in memory, and how far the logits may move.

Parity budget — stated BEFORE measuring, derived the way tests/test_gpu_fp8.py's docstring derives its own:
  * E8 = 3.6 % relative rms rounding error per e4m3 element (3 mantissa bits, upper end);
  * the scores are sums over 128 products with one quantised factor (K), the output a sum over the context with one quantised factor (V): each injects at
    most E8 of the attention branch's rms; q, the probabilities, the weights and the whole MLP branch are untouched: EPS_LAYER_KV = sqrt(2) E8 = 5.1 %;
  * as there: rms(L) = sigma_logit x EPS_LAYER_KV x sqrt(L) x AMP with sigma_logit = 1.3, AMP = 1.5, and max(L) = 4.5 x rms(L)
    -> 0.099 / 0.45 after one layer, 0.28 / 1.26 after eight;
  * underneath sits the 16-bit path's own noise, budgeted at LOGIT_TOL = 0.15 (max) by tests/test_gpu_parity.py: it is added to the max bound, and as
    0.15 / 4.5 to the rms bound (the same max-to-rms factor).
Arg-max flips on the 13-way heads: margin-gated id equality would skip nearly every step here (2 % of deep_llm's steps have a reference margin above twice
the budget), so the flips against the reference's fp32 run are COUNTED, no step left out, and held to the 99th percentile of the flips that i.i.d. Gaussian
noise of rms sqrt(anchor_rms^2 + rms(8)^2) causes on the fixture's own fp32 logits (2000 draws, fixed seed; anchor = the reference's own bf16 run)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import _lib, config as tcfg, kv8, synth  # noqa: E402
from trace_amd.engine import TraceEngine  # noqa: E402
from trace_amd.sampling import SamplingParams  # noqa: E402

E8, SIGMA_LOGIT, AMP, MAX_OVER_RMS, LOGIT_TOL = 0.036, 1.3, 1.5, 4.5, 0.15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kv8_budget(layers):
    """(max, rms) logit budget of the e4m3 KV cache after `layers` layers, the 16-bit path's own allowance included — derived above, not measured"""
    rms = SIGMA_LOGIT * (2.0 ** 0.5) * E8 * (layers ** 0.5) * AMP
    return MAX_OVER_RMS * rms + LOGIT_TOL, rms + LOGIT_TOL / MAX_OVER_RMS, rms


RECORD = os.path.join(ROOT, "profiles", "kv8_parity_measured.txt")
_recorded = []


def record(line):
    """the measured figures of this run, printed and kept in profiles/kv8_parity_measured.txt (rewritten from the run's first line on, so a run of the
    whole module leaves the whole record; a tree that cannot be written to only prints)"""
    print(line)
    _recorded.append(line)
    try:
        with open(RECORD, "w") as f:
            f.write("kv8 parity against the reference's fp32 logits, as tests/test_gpu_kv8_engine.py measured it (budgets: the module's docstring)\n")
            f.write("\n".join(_recorded) + "\n")
    except OSError:
        pass


class _Dev:                       # a flat view of device memory for torch
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 3}


def cache16_views(eng, nslots):
    """(K [layers, slots, kv heads, ctx_pad, hd], V^T [layers, slots, kv heads, hd, ctx_pad]) int16 views of a 16-bit-cache engine"""
    kc, vc, xl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    _lib.check(eng.lib.trace_debug_buffers(eng.h, C.byref(kc), C.byref(vc), C.byref(xl), st))
    layer_stride, slot_stride, head_stride, ctx_pad, NL, NKV, HD, H = [int(x) for x in st]
    K = torch.as_tensor(_Dev(kc.value, layer_stride * NL, "<i2"), device="cuda").view(NL, nslots, NKV, ctx_pad, HD)
    VT = torch.as_tensor(_Dev(vc.value, layer_stride * NL, "<i2"), device="cuda").view(NL, nslots, NKV, HD, ctx_pad)
    return K, VT


def cache8_views(eng, nslots):
    """(K8 [layers, slots, kv heads, ctx_pad, 128], V8 [layers, slots, kv heads, ctx_pad / 32, 128, 32], ks, vs [layers, slots, kv heads, ctx_pad])"""
    p = [C.c_void_p() for _ in range(4)]
    st = (C.c_int64 * 8)()
    _lib.check(eng.lib.trace_debug_kv8_buffers(eng.h, *[C.byref(x) for x in p], st))
    layer_stride, slot_stride, head_stride, ctx_pad, NL, NKV, HD, H = [int(x) for x in st]
    assert layer_stride == nslots * slot_stride and slot_stride == NKV * head_stride and head_stride == ctx_pad * HD and HD == 128
    k8 = torch.as_tensor(_Dev(p[0].value, layer_stride * NL, "|u1"), device="cuda").view(NL, nslots, NKV, ctx_pad, HD)
    v8 = torch.as_tensor(_Dev(p[1].value, layer_stride * NL, "|u1"), device="cuda").view(NL, nslots, NKV, ctx_pad // 32, HD, 32)
    ks = torch.as_tensor(_Dev(p[2].value, layer_stride // HD * NL, "<f4"), device="cuda").view(NL, nslots, NKV, ctx_pad)
    vs = torch.as_tensor(_Dev(p[3].value, layer_stride // HD * NL, "<f4"), device="cuda").view(NL, nslots, NKV, ctx_pad)
    return k8, v8, ks, vs


def rows_of(k8, v8, ks, vs, slot, lo, hi):
    """canonical (K bytes, V bytes [layers, kv heads, hi - lo, 128], ks, vs [layers, kv heads, hi - lo]) of one slot, on the CPU"""
    vb = v8[:, slot].transpose(3, 4).reshape(v8.shape[0], v8.shape[2], -1, 128)
    return k8[:, slot, :, lo:hi].cpu(), vb[:, :, lo:hi].cpu(), ks[:, slot, :, lo:hi].cpu(), vs[:, slot, :, lo:hi].cpu()


def assert_codes(got, ref, what):
    """the bytes equal the torch statement's, every one"""
    diff = got != ref
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} bytes differ"


def run(eng, slots, head=1, steps=3, use_graph=False):
    """[1 + steps, len(slots), NV] fp32 masked logits of decode_begin and `steps` decode steps, and the ids"""
    lg = [eng.decode_begin(list(slots), [head] * len(slots), 16, eos=-1, want_logits=True).clone()]
    for _ in range(steps):
        lg.append(eng.decode_steps(1, use_graph=use_graph, want_logits=True).clone())
    ids, _ = eng.decode_read()
    return torch.stack(lg), [list(r)[:steps + 1] for r in ids]


NSLOTS = 104


@pytest.fixture(scope="module")
def pair(golden_dir):
    """(cfg, 16-bit-cache engine, kv8 engine, spliced rows [79, hidden]): the tiny geometry, 104 KV slots, the same synthetic weights"""
    cfg = tcfg.tiny(num_frames=4)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    sd = synth.state_dict(cfg)
    engs = []
    for kv in (None, "fp8"):
        eng = TraceEngine(cfg, max_batch=NSLOTS, max_ctx=256, max_frames=4, max_new_tokens=64, kv_cache=kv)
        eng.load_weights(sd.items())
        engs.append(eng)
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    engs[0].encode_video(frames, E["timestamps"].tolist())
    L, emb = engs[0].splice(E["input_ids"].tolist(), want_output=True)
    assert L == 79
    yield cfg, engs[0], engs[1], emb.clone(), E, frames
    for e in engs:
        e.close()


def test_keyword_and_context_type(pair):
    cfg, e16, e8, emb, E, frames = pair
    assert e16.kv_cache is None and e8.kv_cache == "fp8"
    assert e16.lib.trace_ctx_kv_cache_type(e16.h) == 0 and e8.lib.trace_ctx_kv_cache_type(e8.h) == 1
    for bad in ("int8", "e4m3", True, 8):
        with pytest.raises(ValueError, match="kv_cache must be"):
            TraceEngine(cfg, kv_cache=bad)
    with pytest.raises(ValueError, match="kv_cache='fp8' with llm_fp8"):
        TraceEngine(cfg, kv_cache="fp8", llm_fp8="w8a8")
    p = [C.c_void_p() for _ in range(4)]
    st = (C.c_int64 * 8)()
    with pytest.raises(_lib.TraceHipError, match="error -3 in trace_debug_buffers"):
        e8.lib.trace_debug_buffers(e8.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), st)
    with pytest.raises(_lib.TraceHipError, match="error -3 in trace_debug_kv8_buffers"):
        e16.lib.trace_debug_kv8_buffers(e16.h, *[C.byref(x) for x in p], st)


def test_memory(pair):
    """trace_ctx_device_bytes shrinks by the cache difference minus the staging (one layer's 16-bit K / V^T of 8 slots) and the slot-index array"""
    cfg, e16, e8, emb, E, frames = pair
    NL, NKV, ctx_pad = cfg.num_hidden_layers, cfg.num_key_value_heads, 256
    pos = NL * NSLOTS * ctx_pad
    want = pos * (kv8.cache_bytes_per_position(NKV, False) - kv8.cache_bytes_per_position(NKV, True)) - 2 * 8 * NKV * ctx_pad * 128 * 2 - 512 * 4
    got = e16.device_bytes() - e8.device_bytes()
    assert abs(got - want) <= 8 * 256, (got, want)                   # every allocation is rounded up to 256 bytes
    assert got > 0


@pytest.mark.parametrize("L", [33, 79])
def test_prefill_identity(pair, L):
    """A past == 0 prefill: hidden rows and step-0 logits bit-identical between the two engines, with and without the hidden rows requested (without
    them the last layer runs for the last row only), alone and as a run of two; for EVERY layer the kv8 arrays hold the row rule's bytes and scales of
    the 16-bit engine's cache rows."""
    cfg, e16, e8, emb, E, frames = pair
    K, VT = cache16_views(e16, NSLOTS)
    a8 = cache8_views(e8, NSLOTS)
    emb2 = (emb.float() * 0.5).to(emb.dtype)
    for want_hidden in (True, False):
        h16 = e16.prefill(0, L, embeds=emb[:L], want_hidden=want_hidden)
        h8 = e8.prefill(0, L, embeds=emb[:L], want_hidden=want_hidden)
        if want_hidden:
            assert torch.equal(h16, h8), "hidden rows"
        lg16 = e16.decode_begin([0], [1], 8, eos=-1, want_logits=True).clone()
        lg8 = e8.decode_begin([0], [1], 8, eos=-1, want_logits=True).clone()
        assert torch.equal(lg16, lg8), "step-0 logits"
    e16.prefill_multi(1, [emb[:L].contiguous(), emb2[:L].contiguous()])
    e8.prefill_multi(1, [emb[:L].contiguous(), emb2[:L].contiguous()])
    assert torch.equal(e16.decode_begin([1, 2], [1, 1], 8, eos=-1, want_logits=True), e8.decode_begin([1, 2], [1, 1], 8, eos=-1, want_logits=True))
    torch.cuda.synchronize()
    elem = torch.bfloat16                                            # the fixture's engines are the bf16 library's
    for slot in (0, 1, 2):
        k16 = K[:, slot, :, :L].view(elem).cpu()
        v16 = VT[:, slot, :, :, :L].view(elem).transpose(2, 3).contiguous().cpu()
        kb, ksr = kv8.quantize_rows_ref(k16)
        vb, vsr = kv8.quantize_rows_ref(v16)
        gk, gv, gks, gvs = rows_of(*a8, slot, 0, L)
        assert torch.equal(gks, ksr) and torch.equal(gvs, vsr), f"L {L} slot {slot}: scales"
        assert_codes(gk, kb, f"L {L} slot {slot}: K8")
        assert_codes(gv, vb, f"L {L} slot {slot}: V8")


@pytest.mark.parametrize("B", [1, 3])
def test_first_append(pair, B):
    """After one decode step, layer 0's appended row (its input does not depend on the cache) is the row rule applied to the 16-bit engine's layer-0
    appended row: two device paths compared exactly through the CPU statement."""
    cfg, e16, e8, emb, E, frames = pair
    L = emb.shape[0]
    K, VT = cache16_views(e16, NSLOTS)
    a8 = cache8_views(e8, NSLOTS)
    embs = [(emb.float() * f).to(emb.dtype) for f in (1.0, 0.5, -0.25)][:B]
    for eng in (e16, e8):
        for b in range(B):
            eng.prefill(b, L, embeds=embs[b])
        eng.decode_begin(list(range(B)), [1] * B, 8, eos=-1)
        eng.decode_steps(1, use_graph=False)
    torch.cuda.synchronize()
    for b in range(B):
        k16 = K[0, b, :, L].view(torch.bfloat16).cpu()
        v16 = VT[0, b, :, :, L].view(torch.bfloat16).cpu()
        kb, ksr = kv8.quantize_rows_ref(k16)
        vb, vsr = kv8.quantize_rows_ref(v16)
        gk, gv, gks, gvs = rows_of(*a8, b, L, L + 1)
        assert torch.equal(gks[0, :, 0], ksr) and torch.equal(gvs[0, :, 0], vsr), f"B {B} row {b}: scales"
        assert_codes(gk[0, :, 0], kb, f"B {B} row {b}: K8 row")
        assert_codes(gv[0, :, 0], vb, f"B {B} row {b}: V8 column")


def test_graph_replay_equals_eager(pair):
    """Five decode steps as one graph replay against five eager launches: the ids, every token's log-probability (fp32, computed in the step from its
    raw logits: a replayed step hands out no logits of its own) and the logits of a sixth, eager step that attends the rows the five appended — all
    bit-equal."""
    cfg, e16, e8, emb, E, frames = pair
    L = emb.shape[0]
    e8.set_logprobs(True)
    try:
        for B in (1, 3):
            res = []
            for g in (False, True):
                for b in range(B):
                    e8.prefill(b, L, embeds=(emb.float() * (1.0 - 0.25 * b)).to(emb.dtype))
                lg0 = e8.decode_begin(list(range(B)), [1] * B, 16, eos=-1, want_logits=True).clone()
                if g:
                    e8.decode_steps(5, use_graph=True)
                else:
                    for _ in range(5):
                        e8.decode_steps(1, use_graph=False)
                lg6 = e8.decode_steps(1, use_graph=False, want_logits=True).clone()
                ids, _ = e8.decode_read()
                res.append((ids, e8.decode_read_logprobs(), lg0, lg6))
            assert res[0][0] == res[1][0] and all(len(r) == 7 for r in res[0][0]), (B, res[0][0], res[1][0])
            assert np.array_equal(res[0][1], res[1][1]) and np.isfinite(res[0][1]).all(), B
            assert torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3]), B
    finally:
        e8.set_logprobs(False)


def test_a_row_inside_batches_of_8_and_100_equals_the_row_alone(pair):
    """ids of slot 0 decoded alone, inside a batch of 8 (skinny step) and of 100 (wide step), as tests/test_gpu_parity.py demands of the 16-bit engine
    (ids; the steps' logits differ in summation order)"""
    cfg, e16, e8, emb, E, frames = pair
    L = emb.shape[0]
    for b in range(100):
        e8.prefill(b, L, embeds=(emb.float() * (1.0 - 0.005 * b)).to(emb.dtype))
    _, alone = run(e8, [0], steps=7)
    for nb in (8, 100):
        for b in range(nb):
            e8.prefill(b, L, embeds=(emb.float() * (1.0 - 0.005 * b)).to(emb.dtype))
        _, ids = run(e8, range(nb), steps=7)
        assert ids[0] == alone[0], (nb, ids[0], alone[0])


def test_kv_copy(pair):
    """kv_copy of all rows: the copy decodes as the source does (logits bit-equal); of a prefix: the four arrays agree below P, an append on the copy
    equals the append on the source; a slot nobody named is untouched"""
    cfg, e16, e8, emb, E, frames = pair
    L = emb.shape[0]
    a8 = cache8_views(e8, NSLOTS)
    e8.prefill(0, L, embeds=emb)
    want, ids = run(e8, [0])
    e8.prefill(0, L, embeds=emb)
    e8.prefill(4, 120, embeds=(torch.randn(120, cfg.hidden_size, device="cuda") * 0.05).to(emb.dtype))
    before4 = [a[:, 4].clone() for a in a8]
    e8.kv_copy(0, [5, 7], L)
    got, ids5 = run(e8, [5])
    assert torch.equal(got, want) and ids5 == ids
    for P in (66, 33, 1):
        e8.prefill(0, P, embeds=emb[:P])
        e8.kv_copy(0, [3, 5], P)
        for d in (3, 5):
            for x, y in zip(rows_of(*a8, d, 0, P), rows_of(*a8, 0, 0, P)):
                assert torch.equal(x, y), (P, d)
        e8.prefill_append(0, P, emb[P:])
        want_p, _ = run(e8, [0])
        e8.prefill_append(3, P, emb[P:])
        got_p, _ = run(e8, [3])
        assert torch.equal(got_p, want_p), P
    for a, b in zip(a8, before4):
        assert torch.equal(a[:, 4], b), "a slot outside the copy changed"


def test_prefill_append_is_deterministic_and_attends_the_quantised_past(pair):
    """prefill_append(past > 0) under kv8 is held to determinism (call to call, with stale rows in between, alone and in a run of slots), not to
    equality with an uncut prefill: the new rows attend the dequantised past.  The past itself is left alone, bit for bit."""
    cfg, e16, e8, emb, E, frames = pair
    L = emb.shape[0]
    a8 = cache8_views(e8, NSLOTS)
    for P in (66, 32, 7):
        outs = []
        for rep in range(2):
            e8.prefill(0, 200, embeds=(torch.randn(200, cfg.hidden_size, device="cuda") * 0.05).to(emb.dtype))       # stale rows everywhere first
            e8.prefill(0, P, embeds=emb[:P])
            past = [x.clone() for x in rows_of(*a8, 0, 0, P)]
            hid = e8.prefill_append(0, P, emb[P:], want_hidden=True).clone()
            for x, y in zip(rows_of(*a8, 0, 0, P), past):
                assert torch.equal(x, y), f"P {P}: the append changed rows below P"
            outs.append((hid, run(e8, [0])[0]))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), P
        e8.prefill(0, P, embeds=emb[:P])
        e8.kv_copy(0, [1, 2], P)
        e8.prefill_append(0, P, [emb[P:].contiguous()] * 3)
        got = run(e8, [0, 1, 2])[0]
        for b in range(3):
            assert torch.equal(got[:, b], outs[0][1][:, 0]), (P, b)


def test_public_generate_calls_run_and_repeat(pair):
    """generate, generate_samples and generate_questions under kv8: reproducible call to call"""
    cfg, e16, e8, emb, E, frames = pair
    ts, ids = E["timestamps"].tolist(), E["input_ids"].tolist()
    a = e8.generate([frames], [ts], [ids], [1], 12)
    b = e8.generate([frames], [ts], [ids], [1], 12)
    assert a[0] == b[0] and len(a[0][0]) > 0
    sp = SamplingParams(temperature=0.8, top_k=20, top_p=0.95, seed=7)
    s1 = e8.generate_samples(frames, ts, ids, 1, 5, 10, sampling=sp)
    s2 = e8.generate_samples(frames, ts, ids, 1, 5, 10, sampling=sp)
    assert s1[0] == s2[0] and all(np.array_equal(x, y) for x, y in zip(s1[2], s2[2]))
    prompts = [ids + [5, 6, 7], ids + [9, 8, 7], ids + [11, 12]]
    q1 = e8.generate_questions(frames, ts, prompts, [1, 1, 1], 10)
    q2 = e8.generate_questions(frames, ts, prompts, [1, 1, 1], 10)
    assert q1[0] == q2[0]


def test_enable_prefix_cache_runs_and_repeats(pair):
    """model.enable_prefix_cache() under kv8: a miss and the hits after it (the same tensor object) give the same ids and log-probabilities, bit for
    bit and round after round, and a hit prefills fewer rows.  Held to determinism, not to the cache being off: with it on the rows after <video>
    attend the quantised prefix."""
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    cfg, e16, e8, emb, E, frames = pair
    m = TraceMistralForCausalLM(cfg, e8)
    ids = torch.tensor([E["input_ids"].tolist()])
    kw = dict(images_or_videos=[frames], video_timestamps=[E["timestamps"].tolist()], heads=[1], max_new_tokens=12, eos_token_id=-1, output_logprobs=True)
    rounds = []
    for _ in range(2):
        m.enable_prefix_cache(True)                                 # (also forgets the entry: the first call of a round is a miss)
        try:
            rows0 = e8.stats["prefill_rows"]
            miss = m.generate(ids, **kw)
            rows1 = e8.stats["prefill_rows"]
            hit = m.generate(ids, **kw)
            rows2 = e8.stats["prefill_rows"]
        finally:
            m.enable_prefix_cache(False)
        assert rows2 - rows1 < rows1 - rows0, "the second call did not reuse the prefix"
        rounds += [miss, hit]
    for r in rounds[1:]:
        assert torch.equal(r.sequences, rounds[0].sequences) and torch.equal(r.logprobs, rounds[0].logprobs)
    assert rounds[0].sequences.shape[1] == 12 and bool(torch.isfinite(rounds[0].logprobs).all())


# ---- parity against the reference's fp32 logits -----------------------------------------------------------------------------------------------
def teacher_forced(eng, M, frames, nb, pair_prefill=False):
    ts, ids = M["timestamps"].tolist(), M["input_ids"].tolist()
    forced = M["forced_ids"].tolist()
    n = len(forced) + 1
    eng.encode_video(frames, ts)
    L, emb = eng.splice(ids, want_output=True)
    if pair_prefill and nb > 1:
        for b in range(0, nb, 2):
            eng.prefill_pair(b, emb, emb)
    else:
        for b in range(nb):
            eng.prefill(b, L, embeds=emb)
    lgs = [eng.decode_begin(list(range(nb)), [1] * nb, n, eos=-1, forced=[forced] * nb, want_logits=True).float().cpu()]
    for _ in range(n - 1):
        lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).float().cpu())
    return lgs


def check_budget(lg, M, layers, tag):
    ref = torch.from_numpy(M["tf_logits"])
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(lg), fin), tag
    e = (lg[fin] - ref[fin]).abs()
    mx, rms = float(e.max()), float(e.pow(2).mean().sqrt())
    bmax, brms, _ = kv8_budget(layers)
    record(f"{tag}: kv8 vs reference fp32 logits — max {mx:.3f} (budget {bmax:.3f}) rms {rms:.4f} (budget {brms:.4f})")
    assert mx <= bmax and rms <= brms, (tag, mx, bmax, rms, brms)


def test_parity_long_context(golden_dir):
    """long_ctx.npz: one real-width layer, prefill 1967, decode at contexts 1968..: batch 1 (16 splits) and 20 (2 splits)"""
    cfg = dataclasses.replace(tcfg.tiny(num_frames=128), intermediate_size=14336, num_hidden_layers=1)
    M = np.load(os.path.join(golden_dir, "long_ctx.npz"))
    eng = TraceEngine(cfg, max_batch=20, max_ctx=2048, max_frames=128, max_new_tokens=32, kv_cache="fp8")
    try:
        eng.load_weights(synth.state_dict(cfg).items())
        frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
        for nb in (1, 20):
            lgs = teacher_forced(eng, M, frames, nb, pair_prefill=True)
            for b in sorted({0, nb - 1}):
                check_budget(torch.stack([x[b] for x in lgs]), M, 1, f"long_ctx (1 layer, ctx 1968..), batch {nb} row {b}")
    finally:
        eng.close()


def flip_threshold(M, noise_rms, draws=2000, seed=0, narrow_width=13):
    """99th percentile of the 13-way arg-max flips that i.i.d. Gaussian noise of `noise_rms` causes on the fixture's own fp32 logits"""
    ref = torch.from_numpy(M["tf_logits"]).double()
    fin = torch.isfinite(ref)
    narrow = fin.sum(-1) == narrow_width
    r = torch.where(fin, ref, torch.full_like(ref, -1e30))[narrow]                  # [steps, NV]
    g = torch.Generator().manual_seed(seed)
    base = r.argmax(-1)
    flips = []
    for _ in range(draws):
        noisy = r + noise_rms * torch.randn(r.shape, generator=g, dtype=torch.float64)
        flips.append(int((noisy.argmax(-1) != base).sum()))
    return int(np.percentile(np.array(flips), 99)), int(narrow.sum())


def test_parity_eight_layers_and_flips(golden_dir):
    """deep_llm.npz: eight real-width layers, batch 1 and 100 (the wide step): the logit budget, and the 13-way arg-max flips against the reference's
    fp32 run counted over every step"""
    from conftest import bf16_anchor_report
    cfg = dataclasses.replace(tcfg.tiny(num_frames=4), intermediate_size=14336, num_hidden_layers=8)
    M = np.load(os.path.join(golden_dir, "deep_llm.npz"))
    eng = TraceEngine(cfg, max_batch=100, max_ctx=192, max_frames=4, max_new_tokens=64, kv_cache="fp8")
    try:
        eng.load_weights(synth.iter_weights(cfg))
        frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
        for nb in (1, 100):
            lgs = teacher_forced(eng, M, frames, nb)
            for b in sorted({0, nb - 1}):
                lg = torch.stack([x[b] for x in lgs])
                check_budget(lg, M, 8, f"deep_llm (8 layers), batch {nb} row {b}")
                if b == 0:
                    r = bf16_anchor_report(lg, M, f"kv8, 8 real-width layers, batch {nb}")
                    thr, steps = flip_threshold(M, (r["ref_bf16_rms"] ** 2 + kv8_budget(8)[2] ** 2) ** 0.5)
                    record(f"deep_llm batch {nb}: kv8 flips {r['hip_flips_13way']} of {steps} 13-way steps (bound {thr}; reference-bf16 anchor "
                           f"{r['ref_bf16_flips_13way']}); kv8 max {r['hip_max']:.3f} rms {r['hip_rms']:.4f}; anchor max {r['ref_bf16_max']:.3f} rms "
                           f"{r['ref_bf16_rms']:.4f}")
                    assert r["hip_flips_13way"] <= thr, (r, thr)
    finally:
        eng.close()
