"""Prompt-prefix reuse on the device: trace_llm_prefill_append (a prefill that continues a slot), trace_kv_copy, trace_embed_rows,
TraceEngine.generate_questions and the model's prefix cache.

The claim under test is an identity, not a tolerance: a row's K / V^T cache contents, its final-norm hidden row and every logit computed
from them are the SAME BITS whether the prompt was prefilled in one pass or cut at any row P and continued, alone or next to other slots, on
the source slot or on a copy.  "Equal" below is torch.equal on the fp32 masked logits of decode_begin and three eager decode steps, on hidden
rows, and on the raw 16-bit cache contents read through trace_debug_buffers.  The only tolerance is test 6's, which is the existing one of
tests/test_gpu_parity.py against the reference's fp32 logits (tiny_e2e.npz).

Tiny geometry as in test_gpu_parity.py: 10 text rows, 56 video rows, 13 rows after them, L = 79; the prefix through <video> is P = 66 rows."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

from trace_amd import _lib, config as tcfg, synth  # noqa: E402
from trace_amd._lib import TraceHipError  # noqa: E402
from trace_amd.engine import SamplingParams, TraceEngine  # noqa: E402
from trace_amd.model.trace_mistral import TraceMistralForCausalLM  # noqa: E402

LOGIT_TOL = 0.15          # tests/test_gpu_parity.py's budget against the reference's fp32 logits
P_VIDEO = 66              # rows through <video>
CUTS = [1, 7, 10, 31, 32, 33, 64, 66, 78]
KINDS = {"bf16": dict(dtype=torch.bfloat16), "f16": dict(dtype=torch.float16), "fp8": dict(dtype=torch.bfloat16, llm_fp8="w8a8")}


class _Dev:                       # a [n] int16 view of device memory for torch
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i2", "data": (ptr, False), "version": 3}


def cache_views(eng, nslots):
    """(K [layers, slots, kv heads, ctx_pad, hd], V^T [layers, slots, kv heads, hd, ctx_pad]) as int16 views of the engine's caches"""
    kc, vc, xl = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = (C.c_int64 * 8)()
    _lib.check(eng.lib.trace_debug_buffers(eng.h, C.byref(kc), C.byref(vc), C.byref(xl), st))
    layer_stride, slot_stride, head_stride, ctx_pad, NL, NKV, HD, H = [int(x) for x in st]
    assert layer_stride == nslots * slot_stride and slot_stride == NKV * head_stride and head_stride == ctx_pad * HD
    K = torch.as_tensor(_Dev(kc.value, layer_stride * NL), device="cuda").view(NL, nslots, NKV, ctx_pad, HD)
    VT = torch.as_tensor(_Dev(vc.value, layer_stride * NL), device="cuda").view(NL, nslots, NKV, HD, ctx_pad)
    return K, VT


def run(eng, slots, head=1, steps=3):
    """[1 + steps, len(slots), NV] fp32 masked logits: decode_begin and `steps` eager decode steps"""
    lg = [eng.decode_begin(list(slots), [head] * len(slots), 8, eos=-1, want_logits=True).clone()]
    for _ in range(steps):
        lg.append(eng.decode_steps(1, use_graph=False, want_logits=True).clone())
    return torch.stack(lg)


def same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        ne = a != b
        fin = torch.isfinite(a.float()) & torch.isfinite(b.float())
        d = (a.float() - b.float())[fin & ne].abs()
        raise AssertionError(f"{what}: {int(ne.sum())} of {ne.numel()} elements differ, first at {torch.nonzero(ne)[0].tolist()}, "
                             f"max |d| {d.max().item() if d.numel() else float('nan')}")


_engines = {}


@pytest.fixture(scope="module")
def tiny(golden_dir):
    """get(kind) -> (cfg, engine with 8 KV slots, spliced rows [79, hidden], K view, V^T view), one engine per kind, made on first use"""
    cfg = tcfg.tiny(num_frames=4)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))

    def get(kind):
        if kind not in _engines:
            kw = KINDS[kind]
            eng = TraceEngine(cfg, max_batch=8, max_ctx=256, max_frames=4, max_new_tokens=64, **kw)
            eng.load_weights(synth.state_dict(cfg).items())
            frames = synth.synth_frames(cfg, 0).to(kw["dtype"])
            eng.encode_video(frames, E["timestamps"].tolist())
            L, emb = eng.splice(E["input_ids"].tolist(), want_output=True)
            assert L == 79 and E["input_ids"].tolist().index(-201) + 1 + 56 - 1 == P_VIDEO
            _engines[kind] = (cfg, eng, emb.clone(), *cache_views(eng, 8))
        return _engines[kind]
    yield get, E
    for v in _engines.values():
        v[1].close()
    _engines.clear()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", list(KINDS))
def test_append_equals_full_prefill(tiny, kind):
    """Every cut P: prefill(0, P) of the first P rows + prefill_append(0, P, rows[P:]) == prefill(0, L) of all rows — in the logits, in the
    final-norm hidden rows P .. L-1 and in K rows / V^T columns [0, L) of every layer; with and without the hidden rows requested (without
    them the bf16 / fp16 paths run the last layer for the last row only).  past = 0 is prefill_multi.  The fp8 engine (W8A8, activations
    quantised per token row) is held to the same identity."""
    get, _ = tiny
    cfg, eng, emb, K, VT = get(kind)
    L = emb.shape[0]
    hid_full = eng.prefill(0, L, embeds=emb, want_hidden=True).clone()
    lg_full = run(eng, [0])
    k_full, vt_full = K[:, 0, :, :L].clone(), VT[:, 0, :, :, :L].clone()
    assert torch.isfinite(hid_full.float()).all() and torch.isfinite(lg_full[torch.isfinite(lg_full)]).all()
    eng.prefill(0, L, embeds=emb)                              # (the last-row shortcut of the last layer: same logits, existing test)
    same(run(eng, [0]), lg_full, f"{kind}: full prefill with / without hidden rows")
    for P in CUTS:
        for want_hidden in (True, False):
            eng.prefill(0, 200, embeds=(torch.randn(200, cfg.hidden_size, device="cuda") * 0.05).to(emb.dtype))      # stale rows everywhere first
            eng.prefill(0, P, embeds=emb[:P])
            hid = eng.prefill_append(0, P, emb[P:], want_hidden=want_hidden)
            tag = f"{kind}: cut at {P}, want_hidden={want_hidden}"
            same(K[:, 0, :, :L], k_full, tag + ": K rows")
            same(VT[:, 0, :, :, :L], vt_full, tag + ": V^T columns")
            if want_hidden:
                same(hid, hid_full[P:], tag + ": hidden rows")
            same(run(eng, [0]), lg_full, tag + ": logits")
    # past = 0 is prefill_multi
    emb2 = (emb.float() * 0.5).to(emb.dtype)
    eng.prefill_multi(0, [emb, emb2])
    want = run(eng, [0, 1])
    k2, vt2 = K[:, :2, :, :L].clone(), VT[:, :2, :, :, :L].clone()
    eng.prefill(0, 200, embeds=(torch.randn(200, cfg.hidden_size, device="cuda") * 0.05).to(emb.dtype))
    eng.prefill_append(0, 0, [emb, emb2])
    same(K[:, :2, :, :L], k2, f"{kind}: past = 0: K")
    same(VT[:, :2, :, :, :L], vt2, f"{kind}: past = 0: V^T")
    same(run(eng, [0, 1]), want, f"{kind}: past = 0 vs prefill_multi")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_append_leaves_the_past_alone(tiny, kind):
    """After an append at P, K rows and V^T columns < P hold the bits they held before (P in the middle of a 16-byte V^T chunk included),
    and the V^T columns from P + L to the end of that 64-position block are zero (the decode attention reads them: finite values needed)."""
    get, _ = tiny
    cfg, eng, emb, K, VT = get(kind)
    L = emb.shape[0]
    f16 = torch.float16 if kind == "f16" else torch.bfloat16
    for P in CUTS:
        eng.prefill(0, 200, embeds=(torch.randn(200, cfg.hidden_size, device="cuda") * 0.05).to(emb.dtype))          # non-zero everywhere below 200
        eng.prefill(0, P, embeds=emb[:P])
        k0, vt0 = K[:, 0, :, :P].clone(), VT[:, 0, :, :, :P].clone()
        for n_new in (L - P, 1):
            eng.prefill_append(0, P, emb[P:P + n_new])
            same(K[:, 0, :, :P], k0, f"{kind}: P={P} +{n_new}: K rows below P")
            same(VT[:, 0, :, :, :P], vt0, f"{kind}: P={P} +{n_new}: V^T columns below P")
            end = (P + n_new + 63) // 64 * 64
            tail = VT[:, 0, :, :, P + n_new:end]
            assert torch.isfinite(tail.view(f16).float()).all() and not tail.any(), f"{kind}: P={P} +{n_new}: V^T tail {P + n_new}..{end} not zero"
            assert VT[:, 0, :, :, P:P + n_new].any()


# ---------------------------------------------------------------------------------------------------------------- 3
def test_rewind_to_the_prefix(tiny):
    """Append suffix A, decode four steps (rows P + len(A) ..), append suffix B at the same `past`: equals B appended to a fresh prefix."""
    get, _ = tiny
    cfg, eng, emb, K, VT = get("bf16")
    P = P_VIDEO
    suf_a, suf_b = emb[P:], (emb[P:P + 9].float() * -0.5).to(emb.dtype)
    eng.prefill(0, P, embeds=emb[:P])
    eng.prefill_append(0, P, suf_b)
    want = run(eng, [0])
    eng.prefill(0, P, embeds=emb[:P])
    eng.prefill_append(0, P, suf_a)
    run(eng, [0], steps=3)                                     # begin + 3 steps = 4 tokens, rows 79 .. 82
    eng.prefill_append(0, P, suf_b)
    same(run(eng, [0]), want, "suffix B after suffix A + decode")
    eng.prefill_append(0, P, suf_b)                            # and once more straight after a decode of B itself
    same(run(eng, [0]), want, "suffix B twice")


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_kv_copy(tiny, kind):
    """kv_copy(0, [2, 3], P): rows [0, P) equal in K and V^T, slot 1 untouched; an append on a copy equals the append on the source; a
    copy of ALL rows decodes as its source does."""
    get, _ = tiny
    cfg, eng, emb, K, VT = get(kind)
    L = emb.shape[0]
    for P in (P_VIDEO, 61, 8, 1):
        for s in (1, 2, 3):
            eng.prefill(s, 120, embeds=(torch.randn(120, cfg.hidden_size, device="cuda") * 0.05).to(emb.dtype))
        k1, vt1, k2, vt2 = K[:, 1].clone(), VT[:, 1].clone(), K[:, 2].clone(), VT[:, 2].clone()
        eng.prefill(0, P, embeds=emb[:P])
        eng.kv_copy(0, [2, 3], P)
        same(K[:, 1], k1, f"{kind}: P={P}: slot 1 K")
        same(VT[:, 1], vt1, f"{kind}: P={P}: slot 1 V^T")
        for d in (2, 3):
            same(K[:, d, :, :P], K[:, 0, :, :P], f"{kind}: P={P}: K of copy {d}")
            same(VT[:, d, :, :, :P], VT[:, 0, :, :, :P], f"{kind}: P={P}: V^T of copy {d}")
        P8 = (P + 7) // 8 * 8                                  # (the V^T side may round the copy up to 8 positions)
        same(K[:, 2, :, P:], k2[:, :, P:], f"{kind}: P={P}: K rows of a copy at and above P")
        same(VT[:, 2, :, :, P8:], vt2[:, :, :, P8:], f"{kind}: P={P}: V^T columns of a copy above P")
        eng.prefill_append(0, P, emb[P:])
        want = run(eng, [0])
        eng.prefill_append(3, P, emb[P:])
        same(run(eng, [3]), want, f"{kind}: P={P}: append on a copy")
        same(K[:, 3, :, :L], K[:, 0, :, :L], f"{kind}: P={P}: K after the append on a copy")
        same(VT[:, 3, :, :, :L], VT[:, 0, :, :, :L], f"{kind}: P={P}: V^T after the append on a copy")
    eng.prefill(0, L, embeds=emb)
    want = run(eng, [0])
    eng.prefill(0, L, embeds=emb)
    eng.kv_copy(0, [5], L)
    same(run(eng, [5]), want, f"{kind}: a copy of all rows decodes as its source")


# ---------------------------------------------------------------------------------------------------------------- 5
def test_neighbours_do_not_matter(tiny):
    """Runs of 2, 5 and 8 slots appended in one pass (different suffixes of one length) each equal the slot appended alone; the prefix rows
    the copies got once survive every append and decode in between."""
    get, _ = tiny
    cfg, eng, emb, K, VT = get("bf16")
    P = P_VIDEO
    sufs = [(emb[P:].float() * f).to(emb.dtype) for f in (1.0, 0.5, -0.25, 0.75, -1.0, 0.3, 1.25, -0.6)]
    alone = []
    for b in range(8):
        eng.prefill(0, P, embeds=emb[:P])
        eng.prefill_append(0, P, sufs[b])
        alone.append(run(eng, [0])[:, 0])
    eng.prefill(0, P, embeds=emb[:P])
    eng.kv_copy(0, list(range(1, 8)), P)
    for n in (2, 5, 8):
        eng.prefill_append(0, P, sufs[:n])
        got = run(eng, list(range(n)))
        for b in range(n):
            same(got[:, b], alone[b], f"run of {n}, slot {b}")
    eng.prefill_append(3, P, sufs[6:8])                        # a run that starts at another slot
    got = run(eng, [3, 4])
    same(got[:, 0], alone[6], "run at slot 3")
    same(got[:, 1], alone[7], "run at slot 4")


# ---------------------------------------------------------------------------------------------------------------- 6
def test_prefix_plus_append_against_the_reference_fixture(tiny):
    """Anchored on the reference: the rows through <video> (P = 66), the 13 rows after them appended (embedded by trace_embed_rows), then the
    teacher-forced stream of tiny_e2e.npz: logits within test_gpu_parity.py's LOGIT_TOL of the reference's fp32 logits, same -inf pattern."""
    get, E = tiny
    cfg, eng, emb, K, VT = get("bf16")
    ids = E["input_ids"].tolist()
    cut = ids.index(-201) + 1
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    eng.encode_video(frames, E["timestamps"].tolist())
    P = eng.splice(ids[:cut])
    assert P == P_VIDEO
    eng.prefill(0, P)
    suf = eng.embed_rows(ids[cut:], want_output=True)
    same(suf, emb[P:], "embed_rows vs the spliced rows after <video>")
    eng.embed_rows(ids[cut:])
    eng.prefill_append(0, P, None, L=len(ids) - cut)           # the internal buffer
    forced = E["forced_ids"].tolist()
    n = len(forced) + 1
    lgs = [eng.decode_begin([0], [1], n, eos=-1, forced=[forced], want_logits=True).cpu()]
    for _ in range(n - 1):
        lgs.append(eng.decode_steps(1, use_graph=False, want_logits=True).cpu())
    lg = torch.cat(lgs)
    ref = torch.from_numpy(E["tf_logits"])
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(lg), fin), "head mask (-inf pattern) differs from the reference"
    err = (lg[fin] - ref[fin]).abs().max().item()
    print(f"prefix + append vs reference fp32 logits: max |d| {err:.4f} (budget {LOGIT_TOL})")
    assert err < LOGIT_TOL, err


# ---------------------------------------------------------------------------------------------------------------- 7
def test_model_prefix_cache_and_generate_questions(tiny):
    """Three prompts differing after <video>, one tensor: ids and heads with the cache on equal those with it off, call by call (B = 1
    three times) and as one B = 3 call; with it on the tower runs once (4 frames) and only 66 + the suffix rows are prefilled.  Another
    video in between, an in-place edit of the tensor and enable_prefix_cache(False) each force a miss with unchanged ids.  Sampling with a
    torch seed gives the same ids on and off.  generate_questions with suffixes of different lengths equals generate."""
    get, E = tiny
    cfg, eng, emb, K, VT = get("bf16")
    model = TraceMistralForCausalLM(cfg, eng)
    assert model.prefix_cache_enabled is False
    base = torch.from_numpy(E["input_ids"]).long()
    cut = base.tolist().index(-201) + 1
    prompts = []
    for q in range(3):
        p = base.clone()
        p[cut:-1] = (p[cut:-1] + 17 * q) % (cfg.vocab_size - 3) + 3
        prompts.append(p)
    n_suf = len(base) - cut
    ts = E["timestamps"].tolist()
    fa = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    fb = synth.synth_frames(cfg, 1).to(torch.bfloat16)
    st = eng.stats

    def gen(ps, vids, head=1, **kw):
        heads = [head] * len(ps)
        out = model.generate(torch.stack(ps), images_or_videos=vids, modal_list=["video"] * len(ps), video_timestamps=[ts] * len(ps), heads=heads,
                             max_new_tokens=12, **kw)
        return out.tolist(), heads

    def delta(fn):
        v0, r0 = st["vit_frames"], st["prefill_rows"]
        res = fn()
        return res, st["vit_frames"] - v0, st["prefill_rows"] - r0

    off1, dv, dr = delta(lambda: [gen([p], [fa]) for p in prompts])
    assert (dv, dr) == (12, 3 * 79)
    off3, dv, dr = delta(lambda: gen(prompts, [fa, fa, fa]))
    assert (dv, dr) == (12, 3 * 79)

    off_text = [gen([p], [fa], head=0) for p in prompts] + [gen(prompts, [fa, fa, fa], head=0)]      # the text head: a 321-way arg-max per token

    model.enable_prefix_cache()
    on_text = [gen([p], [fa], head=0) for p in prompts] + [gen(prompts, [fa, fa, fa], head=0)]
    print("text-head ids of the three questions:", [o[0][0] for o in on_text[:3]])
    assert on_text == off_text
    model.enable_prefix_cache()                                # (forget the entry: the next call is a miss again)
    on1, dv, dr = delta(lambda: [gen([p], [fa]) for p in prompts])
    assert on1 == off1
    assert (dv, dr) == (4, P_VIDEO + 3 * n_suf), (dv, dr)
    again, dv, dr = delta(lambda: gen([prompts[1]], [fa]))
    assert again == off1[1] and (dv, dr) == (0, n_suf)
    on3, dv, dr = delta(lambda: gen(prompts, [fa, fa, fa]))
    assert on3 == off3
    assert (dv, dr) == (4, P_VIDEO + 3 * n_suf), (dv, dr)
    hit, dv, dr = delta(lambda: gen([prompts[2]], [fa]))       # the B = 3 call left the shared rows in slot 0
    assert hit == off1[2] and (dv, dr) == (0, n_suf)
    mixed, dv, dr = delta(lambda: gen(prompts[:2], [fa, fb]))  # two different tensors: today's path
    assert dv == 8 and dr == 2 * 79 and eng.prefix_entry() is None
    # a call with another video between two questions
    offb = gen([prompts[0]], [fb])
    res, dv, dr = delta(lambda: [gen([prompts[0]], [fa]), gen([prompts[0]], [fb]), gen([prompts[1]], [fa])])
    assert res == [off1[0], offb, off1[1]] and dv == 12
    # an equal but different tensor object is another video as far as the cache can know
    res, dv, dr = delta(lambda: gen([prompts[2]], [fa.clone()]))
    assert res == off1[2] and dv == 4
    # an in-place edit of the tensor
    fc = fa.clone()
    r0 = gen([prompts[0]], [fc])
    fc.mul_(0.5)
    r1, dv, dr = delta(lambda: gen([prompts[1]], [fc]))
    assert dv == 4 and r0 == off1[0]
    r2, dv, dr = delta(lambda: gen([prompts[2]], [fc]))
    assert dv == 0
    # any engine call that rewrites slot 0 or encodes a video drops the entry
    assert eng.prefix_entry() is not None
    eng.prefill(0, 79, embeds=emb)
    assert eng.prefix_entry() is None
    r3, dv, dr = delta(lambda: gen([prompts[2]], [fc]))
    assert dv == 4 and r3 == r2
    # sampling: the same draws on and off
    kw = dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.95)
    torch.manual_seed(11)
    s_on1 = gen([prompts[0]], [fa], **kw)
    torch.manual_seed(11)
    s_hit = gen([prompts[0]], [fa], **kw)
    torch.manual_seed(12)
    s_on3 = gen(prompts, [fa, fa, fa], **kw)
    # switching the cache off drops the entry and its tensor reference
    model.enable_prefix_cache(False)
    assert eng.prefix_entry() is None and model.prefix_cache_enabled is False
    r1_off = gen([prompts[1]], [fc])
    r2_off, dv, dr = delta(lambda: gen([prompts[2]], [fc]))
    assert (r1, r2) == (r1_off, r2_off) and (dv, dr) == (4, 79)
    torch.manual_seed(11)
    s_off1 = gen([prompts[0]], [fa], **kw)
    torch.manual_seed(12)
    s_off3 = gen(prompts, [fa, fa, fa], **kw)
    assert s_on1 == s_off1 and s_hit == s_off1 and s_on3 == s_off3
    greedy = gen([prompts[0]], [fa])
    assert greedy == off1[0]

    # engine level: suffixes of different lengths (slots laid out group by group: prompt 1 lands in slot 2), in the caller's order
    ragged = [prompts[0].tolist(), prompts[1].tolist()[:cut + 8] + [-205], prompts[2].tolist(), base.tolist()[:cut] + [5, -205]]
    want = eng.generate([fa] * 4, [ts] * 4, ragged, [1, 1, 0, 1], 12)
    got, dv, dr = delta(lambda: eng.generate_questions(fa, ts, ragged, [1, 1, 0, 1], 12))
    assert got == want
    assert (dv, dr) == (4, P_VIDEO + 13 + 9 + 13 + 2)
    sp = SamplingParams(0.8, 10, 0.9, 1234)
    assert eng.generate_questions(fa, ts, ragged, [1, 1, 0, 1], 12, sampling=sp) == eng.generate([fa] * 4, [ts] * 4, ragged, [1, 1, 0, 1], 12, sampling=sp)
    with pytest.raises(ValueError, match="differs from prompt 0"):
        eng.generate_questions(fa, ts, [ragged[0], [3] + ragged[1][1:]], [1, 1], 4)
    with pytest.raises(ValueError, match="nothing to append"):
        eng.generate_questions(fa, ts, [ragged[0], ragged[0][:cut]], [1, 1], 4)


# ---------------------------------------------------------------------------------------------------------------- 8
def test_errors_come_before_any_launch(tiny):
    """Every refused call raises TraceHipError with its message, and the engine still answers a correct generate afterwards."""
    get, E = tiny
    cfg, eng, emb, K, VT = get("bf16")
    ts, ids = E["timestamps"].tolist(), E["input_ids"].tolist()
    frames = synth.synth_frames(cfg, 0).to(torch.bfloat16)
    want = eng.generate([frames], [ts], [ids], [1], 12)
    eng.prefill(0, 20, embeds=emb[:20])
    k0, vt0 = K[:, 0, :, :20].clone(), VT[:, 0, :, :, :20].clone()
    ptr1 = (C.c_void_p * 1)(emb.data_ptr())
    with pytest.raises(TraceHipError, match="past exceeds the rows the slot holds"):
        eng.prefill_append(0, 21, emb[:5])
    eng.prefill(1, 10, embeds=emb[:10])
    with pytest.raises(TraceHipError, match="past exceeds the rows the slot holds"):
        eng.prefill_append(0, 15, [emb[:5], emb[:5]])                                       # slot 0 holds 20 rows, slot 1 only 10
    with pytest.raises(TraceHipError, match="bad L / past"):
        eng.prefill_append(0, -1, emb[:5])
    with pytest.raises(TraceHipError, match="bad L / past"):
        eng.lib.trace_llm_prefill_append(eng.h, 0, 1, 20, ptr1, 0, None, None)
    with pytest.raises(TraceHipError, match=r"past \+ L exceeds max_ctx"):
        eng.prefill_append(0, 20, torch.zeros(237, cfg.hidden_size, device="cuda", dtype=emb.dtype))        # 20 + 237 = 257 > 256
    eng.prefill_append(0, 20, torch.zeros(236, cfg.hidden_size, device="cuda", dtype=emb.dtype))            # exactly max_ctx is fine
    eng.prefill(0, 20, embeds=emb[:20])
    with pytest.raises(TraceHipError, match="bad slot / n"):
        eng.prefill_append(8, 0, emb[:5])
    with pytest.raises(TraceHipError, match="bad slot / n"):
        eng.prefill_append(7, 0, [emb[:5], emb[:5]])                                        # slots 7, 8
    with pytest.raises(TraceHipError, match="bad slot / n"):
        eng.prefill_append(-1, 0, emb[:5])
    with pytest.raises(TraceHipError, match="bad slot / n"):
        eng.lib.trace_llm_prefill_append(eng.h, 0, 9, 0, (C.c_void_p * 9)(*[emb.data_ptr()] * 9), 5, None, None)
    with pytest.raises(TraceHipError, match="embeds may be NULL with n == 1 only"):
        eng.lib.trace_llm_prefill_append(eng.h, 0, 2, 0, None, 5, None, None)
    with pytest.raises(TraceHipError, match="hidden_out with n == 1 only"):
        eng.lib.trace_llm_prefill_append(eng.h, 0, 2, 0, (C.c_void_p * 2)(emb.data_ptr(), emb.data_ptr()), 5, C.c_void_p(emb.data_ptr()), None)
    with pytest.raises(ValueError):
        eng.prefill_append(0, 0, [emb[:5]] * 9)
    with pytest.raises(ValueError):
        eng.prefill_append(0, 0, [emb[:5], emb[:6]])
    # kv_copy
    with pytest.raises(TraceHipError, match="the source slot is among the destinations"):
        eng.kv_copy(0, [1, 0], 10)
    with pytest.raises(TraceHipError, match="rows exceeds the rows the source slot holds"):
        eng.kv_copy(0, [1], 21)
    with pytest.raises(TraceHipError, match="destination slot out of range"):
        eng.kv_copy(0, [1, 8], 10)
    with pytest.raises(TraceHipError, match="source slot out of range"):
        eng.kv_copy(8, [1], 10)
    with pytest.raises(TraceHipError, match="bad rows"):
        eng.kv_copy(0, [1], 0)
    with pytest.raises(TraceHipError, match="bad dst_slots / n"):
        eng.kv_copy(0, [], 10)
    # embed_rows
    with pytest.raises(TraceHipError, match="<video> placeholder among the ids"):
        eng.embed_rows([5, -201, 6])
    with pytest.raises(TraceHipError, match="<video> placeholder among the ids"):
        eng.embed_rows([-200])
    with pytest.raises(TraceHipError, match="token id out of range"):
        eng.embed_rows([5, cfg.vocab_size])
    with pytest.raises(TraceHipError, match="more <time> placeholders than time tokens"):
        eng.embed_rows([5, -203])
    with pytest.raises(TraceHipError, match="more rows than max_ctx"):
        eng.embed_rows([5] * 257)
    same(K[:, 0, :, :20], k0, "slot 0 K after the refused calls")
    same(VT[:, 0, :, :, :20], vt0, "slot 0 V^T after the refused calls")
    rows = eng.embed_rows([7, -203, -204, -205], time_rows=[3], score_rows=[2], want_output=True)
    same(rows[0], eng.embed_rows([7], want_output=True)[0], "embed_rows: a token row next to <time> / <score> / <sync> rows")
    assert rows.shape == (4, cfg.hidden_size) and torch.isfinite(rows.float()).all()
    # n x L above the prefill workspace needs a longer context than the shared engine's: 8192 rows hold four 2000-row suffixes, not five
    big = TraceEngine(cfg, max_batch=8, max_ctx=2048, max_frames=4, max_new_tokens=8)
    try:
        big.load_weights(synth.state_dict(cfg).items())
        pre = (torch.randn(10, cfg.hidden_size, device="cuda") * 0.02).to(emb.dtype)
        big.prefill_multi(0, [pre] * 5)
        long_embs = [(torch.randn(2000, cfg.hidden_size, device="cuda") * 0.02).to(emb.dtype) for _ in range(5)]
        with pytest.raises(TraceHipError, match="prefill workspace"):
            big.prefill_append(0, 10, long_embs)
        big.prefill_append(0, 10, long_embs[:4])
        assert torch.isfinite(run(big, [0, 3])[0, :, cfg.vocab_size + 1:cfg.vocab_size + 1 + cfg.time_vocab_size]).all()
    finally:
        big.close()
    assert eng.generate([frames], [ts], [ids], [1], 12) == want


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_real_width_c2_shape(kind):
    """The C2 prompt shape at the real Mistral-7B widths (two layers): L = 1967 random embedding rows.  A 25-row suffix on 1942 cached rows
    (P neither a multiple of 64 nor of 8; GEMMs at M = 25 against M = 1967) and 1817 rows on 150 in a run of four (M = 7268 against 7868)
    each equal the full prefill, in the logits and in the cache.  Decides whether the GEMM dispatch (128^2 tiles below M = 1024, 256^2
    above) gives row-identical bits at these shapes."""
    dtype = KINDS[kind]["dtype"]
    cfg = dataclasses.replace(tcfg.trace_7b(128), num_hidden_layers=2)
    L = 1967
    eng = TraceEngine(cfg, max_batch=4, max_ctx=2048, max_frames=128, max_new_tokens=8, dtype=dtype)
    try:
        eng.load_weights(synth.iter_weights(cfg, dtype=dtype, device="cuda:0"))
        K, VT = cache_views(eng, 4)
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        embs = [(torch.randn(L, cfg.hidden_size, device="cuda", generator=g) * s).to(dtype) for s in (0.02, 0.05, 0.01, 0.03)]
        # one prompt: full against 1942 + 25
        eng.prefill(0, L, embeds=embs[0])
        want1 = run(eng, [0])
        fin = torch.isfinite(want1)
        assert fin[:, :, cfg.vocab_size + 1:cfg.vocab_size + 1 + cfg.time_vocab_size].all()
        k_full, vt_full = K[:, 0, :, :L].clone(), VT[:, 0, :, :, :L].clone()
        hid_full = eng.prefill(0, L, embeds=embs[0], want_hidden=True)
        P = 1942
        eng.prefill(1, P, embeds=embs[0][:P])
        eng.prefill_append(1, P, embs[0][P:])
        same(run(eng, [1]), want1, f"{kind}: 1942 + 25: logits")
        same(K[:, 1, :, :L], k_full, f"{kind}: 1942 + 25: K")
        same(VT[:, 1, :, :, :L], vt_full, f"{kind}: 1942 + 25: V^T")
        eng.prefill(1, P, embeds=embs[0][:P])
        same(eng.prefill_append(1, P, embs[0][P:], want_hidden=True), hid_full[P:], f"{kind}: 1942 + 25: hidden rows")
        # the same through a copy of the prefix
        eng.prefill(2, P, embeds=embs[0][:P])
        eng.kv_copy(2, [3], P)
        same(K[:, 3, :, :P], k_full[:, :, :P], f"{kind}: kv_copy of 1942 rows: K")
        same(VT[:, 3, :, :, :P], vt_full[:, :, :, :P], f"{kind}: kv_copy of 1942 rows: V^T")
        eng.prefill_append(3, P, embs[0][P:])
        same(run(eng, [3]), want1, f"{kind}: 1942 copied + 25: logits")
        # a run of four: full against 150 + 1817
        eng.prefill_multi(0, embs)
        want4 = run(eng, [0, 1, 2, 3])
        k4, vt4 = K[:, :, :, :L].clone(), VT[:, :, :, :, :L].clone()
        P = 150
        eng.prefill_multi(0, [e[:P] for e in embs])
        eng.prefill_append(0, P, [e[P:] for e in embs])
        same(K[:, :, :, :L], k4, f"{kind}: 4 x (150 + 1817): K")
        same(VT[:, :, :, :, :L], vt4, f"{kind}: 4 x (150 + 1817): V^T")
        same(run(eng, [0, 1, 2, 3]), want4, f"{kind}: 4 x (150 + 1817): logits")
    finally:
        eng.close()
