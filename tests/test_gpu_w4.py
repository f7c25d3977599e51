"""The w4 weight path on the device: the quantiser / packer / dequantiser against trace_amd/w4.py bit for bit, the decode GEMV against probes with exact
answers (tests/w4_probes.py) and against Gaussian operands, and an engine on w4 weights (TraceEngine(llm_w4=True)) against its TWIN — a bf16 engine loaded
with the same weights except that the four decoder projections are W~ = w4.dequant(w4.quant(W)).  Every w4 value is a bf16 value and activations are never
quantised, so the twin multiplies by the same matrix: the prefill must agree bit for bit, the decode steps up to the summation order of the GEMVs.

Two geometries, each with its own twin and its own bound: "tiny" (hidden 4096, intermediate 256, 2 layers) and "real" (intermediate 14336, 2 layers — the
real-width plans: the down projection in several k-chunks with WPT > 1, gate|up on the NT = 2 route with the 16-row gate / up interleave).

Decode bound (taken from the twin itself, before looking at the w4 engine): D = the largest |logit| difference between the twin's own GEMV step and its
fused-norm step (ops.tuned(decode__fuse_norm_rows=0) against decode__fuse_norm_rows=4) over the same forced 12 steps at B = 1 and 3 — two summation orders
of the same products on the same weights; the w4 engine must stay within 2 D of the twin, and pick the twin's ids wherever the twin's top-2 margin exceeds
2 D.  The same 2 D is applied at B = 33, where the twin has no fused step to take a D of its own from (the fused step takes at most 4 rows): a row's
logits do not depend on the other rows of its batch, and the w4 GEMV's k-partition changes with the row-group count (NB = 1, 2, 4) exactly as the bf16
GEMV's does, so the difference per row is of the same kind at every batch size; what grows with B is only the number of rows the maximum is taken over
(429 against 52 values per logit column).  At B = 33 the twin runs its default step there, the wide GEMM step; its difference from the twin's own GEMV
step at that batch size is printed beside the result, for information.
Measured on an MI355X (profiles/w4_parity_measured.txt, section 3, which this module rewrites on every run):
  tiny: D = 0.010156, bound 0.020312; w4 against its twin max |dlogit| 0.011908 (B = 1), 0.012912 (B = 3), 0.019723 (B = 33); the margin condition leaves
        out 0 of 13, 0 of 39 and 1 of 429 steps.
  real: D = 0.014431, bound 0.028862; max |dlogit| 0.018967 (B = 1), 0.022304 (B = 3), 0.023478 (B = 33); left out 1 of 13, 3 of 39 and 42 of 429 steps
        (random weights: small margins).  The twin's wide GEMM step against its GEMV step at B = 33: 0.015722 (tiny), 0.025657 (real).
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import w4_probes as P  # noqa: E402
from trace_amd import config as tcfg, synth, w4  # noqa: E402
from trace_amd.engine import TraceEngine, ops  # noqa: E402

dev = torch.device("cuda")
BF = torch.bfloat16
SHAPES = ((16, 256), (48, 512), (16384, 256), (64, 14336), (4112, 4352))


RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "w4_parity_measured.txt")
MARK = "-- 3. the w4 engine against its twin"
_recorded = []


def record(line):
    """the figures this run measured, printed and kept as section 3 of profiles/w4_parity_measured.txt: everything from the marker line on is rewritten
    from the run's first line on, what stands before it (tools/w4_parity.py's sections) is kept; a tree that cannot be written to only prints"""
    print(line)
    _recorded.append(line)
    try:
        head = open(RECORD).read().split(MARK)[0] if os.path.exists(RECORD) else ""
        with open(RECORD, "w") as f:
            f.write(head + MARK + " (a bf16 engine loaded with W~; written by tests/test_gpu_w4.py, bounds: its docstring) --\n")
            f.write("\n".join(_recorded) + "\n")
    except OSError:
        pass


def _weights(N, K, seed=0):
    g = torch.Generator().manual_seed(seed + N + K)
    W = (torch.randn((N, K), generator=g) * 0.02).to(BF)
    W[0, :32] = 0                                                                               # a zero block
    W[N - 1, K - 32:] = 0
    W[1, 32:64] = torch.tensor([0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0, 0.25] * 4).to(BF) * 2.0 ** -7    # exact ties under amax 6 * 2^-7
    W[2, 0] = 2.0 ** -130                                                                       # a denormal beside nothing else in its block
    W[2, 1:32] = 0
    return W


@pytest.mark.parametrize("N,K", ((16, 256), (48, 512), (4112, 4352), (64, 14336)))
def test_quantiser_packer_and_dequantiser_equal_the_torch_statement(N, K):
    W = _weights(N, K)
    codes, exps = w4.quant(W)
    gc, ge = ops.quant_rows_w4(W.to(dev))
    assert torch.equal(gc.cpu(), codes), f"{int((gc.cpu() != codes).sum())} code bytes differ"
    assert torch.equal(ge.cpu(), exps)
    tc, te = ops.tile_pack_w4(gc, ge)
    rc, re = w4.tile_pack(codes, exps)
    assert torch.equal(tc.cpu(), rc.reshape(-1)) and torch.equal(te.cpu(), re.reshape(-1))
    Wt = ops.dequant_w4(tc, te, N, K)
    assert torch.equal(Wt.cpu().view(torch.int16), w4.dequant(codes, exps).view(torch.int16))   # bits: no negative zeros either


def test_plan_classes_of_the_five_shapes():
    p = {s: ops.skinny_w4_plan(s[0], s[1], 1) for s in SHAPES}
    assert p[(16, 256)]["grid"] == 1 and p[(48, 512)]["ntiles"] == 3 and p[(16384, 256)]["NT"] == 2
    assert p[(64, 14336)]["KS"] > 1 and p[(64, 14336)]["WPT"] > 1 and p[(4112, 4352)]["ntiles"] == 257


@pytest.mark.parametrize("B", (1, 3, 16, 17, 33, 64))
@pytest.mark.parametrize("N,K", SHAPES)
def test_gemv_probes_are_exact(N, K, B):
    plan = ops.skinny_w4_plan(N, K, B)
    for name in P.PROBES:
        codes, exps, X = P.build(name, N, K, B)
        want = P.expected(codes, exps, X)
        dc, de, dx = codes.to(dev), exps.to(dev), X.to(dev)
        tc, te = ops.tile_pack_w4(dc, de)
        keep = (tc.clone(), te.clone(), dx.clone())
        out = torch.full((plan["KS"] + 1, P.SK_ROWS, N), P.SENTINEL, dtype=torch.float32, device=dev)      # the last chunk is a guard
        ops.skinny_w4(dx, tc, te, N, out=out)
        got, clean = P.result(out.cpu(), B)
        assert clean, f"{name}: rows >= B or the guard chunk were written"
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {got.numel()} differ, first {(got != want).nonzero()[:3].tolist()}"
        assert torch.equal(tc, keep[0]) and torch.equal(te, keep[1]) and torch.equal(dx, keep[2]), f"{name}: inputs changed"


@pytest.mark.parametrize("B", (1, 20, 40, 64))
@pytest.mark.parametrize("N,K", ((6144, 4096), (4096, 14336), (28672, 4096), (256, 512)))
def test_gemv_on_gaussian_operands(B, N, K):
    """the bound tests/test_gpu_fp8.py holds the weight-only GEMV to: the same products, fp32 accumulation in another order, W~ enters exactly"""
    torch.manual_seed(B + N + 2)
    x = torch.randn(B, K, device=dev).to(BF)
    w = (torch.randn(N, K, device=dev) * 0.02).to(BF)
    codes, exps = ops.quant_rows_w4(w)
    tc, te = ops.tile_pack_w4(codes, exps)
    Wt = ops.dequant_w4(tc, te, N, K)
    got = ops.skinny_w4(x, tc, te, N).sum(0)[:B]
    ref = x.float() @ Wt.float().t()
    err = (got - ref).abs().max().item()
    assert err < 1e-3 * ref.abs().max().item() + 1e-4, err


# ---- the engine and its twin ----
NSLOTS = 34


def _make_pair(golden_dir, kind):
    """(cfg, w4 engine, twin engine, spliced rows [79, hidden], fixture arrays, frames, state dict, kind)"""
    cfg = tcfg.tiny(num_frames=4)
    if kind == "real":
        cfg = dataclasses.replace(cfg, intermediate_size=14336)
    E = np.load(os.path.join(golden_dir, "tiny_e2e.npz"))
    sd = synth.state_dict(cfg) if kind == "tiny" else dict(synth.iter_weights(cfg, device="cuda"))    # (real width: W~ is then made on the device)
    e4 = TraceEngine(cfg, max_batch=NSLOTS, max_ctx=256, max_frames=4, max_new_tokens=32, llm_w4=True)
    e4.load_weights(sd.items())
    tw = TraceEngine(cfg, max_batch=NSLOTS, max_ctx=256, max_frames=4, max_new_tokens=32)
    tw.load_weights(w4.twin_items(sd.items()))
    frames = synth.synth_frames(cfg, 0).to(BF)
    tw.encode_video(frames, E["timestamps"].tolist())
    L, emb = tw.splice(E["input_ids"].tolist(), want_output=True)
    assert L == 79
    return cfg, e4, tw, emb.clone(), E, frames, sd, kind


@pytest.fixture(scope="module", params=["tiny", "real"])
def geo(request, golden_dir):
    """the w4 engine and its twin at one of the two geometries"""
    p = _make_pair(golden_dir, request.param)
    yield p
    p[1].close()
    p[2].close()


@pytest.fixture(scope="module")
def pair(golden_dir):
    """the tiny geometry alone (the API-level tests)"""
    p = _make_pair(golden_dir, "tiny")
    yield p[:7]
    p[1].close()
    p[2].close()


def test_real_geometry_takes_the_real_width_plans():
    """what the tiny geometry never runs: down in several k-chunks with several waves a tile, gate|up with two 16-row tiles a task"""
    for B in (1, 3, 33):
        r = ops.decode_route_w4(B, 4096, 14336, 6144)
        assert r["ks_d"] > 1 and ops.skinny_w4_plan(4096, 14336, B)["WPT"] > 1 and ops.skinny_w4_plan(28672, 4096, B)["NT"] == 2
        t = ops.decode_route_w4(B, 4096, 256, 6144)
        assert t["ks_d"] == 1 and ops.skinny_w4_plan(512, 4096, B)["NT"] == 1


def test_context_type_and_memory(geo):
    """(d) trace_ctx_device_bytes: the w4 context is smaller than its twin by exactly what the engine allocates differently — both 16-bit copies of the
    projections (row-major and tile) against their w4 copy, one layer of 16-bit scratch and the staging pair of the largest loaded tensor"""
    cfg, e4, tw, emb, E, frames, sd, kind = geo
    assert e4.llm_w4 and not tw.llm_w4 and e4.decode_batch_max == NSLOTS
    assert e4.lib.trace_ctx_llm_weights_type(e4.h) == 3 and tw.lib.trace_ctx_llm_weights_type(tw.h) == 0
    H, I, NL = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    QKV = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * cfg.head_dim
    elems = QKV * H + H * H + 2 * I * H + H * I                      # one layer's four projections
    bytes16 = NL * elems * 2 * 2                                     # the twin's row-major and tile copies
    bytes4 = NL * sum(w4.weight_bytes(n, k) for n, k in ((QKV, H), (H, H), (2 * I, H), (H, I)))
    scratch = elems * 2
    piece = max(QKV * H, H * H, H * I)                               # the largest tensor a load call brings (gate and up come apart)
    staging = piece // 2 + piece // 32
    saved, want = tw.device_bytes() - e4.device_bytes(), bytes16 - bytes4 - scratch - staging
    record(f"{kind}: device bytes twin {tw.device_bytes()}, w4 {e4.device_bytes()}, saved {saved} (projections 16-bit {bytes16}, w4 {bytes4}, scratch {scratch}, "
           f"staging {staging}: expected {want})")
    assert abs(saved - want) <= 64 * 256, (saved, want)             # every allocation is rounded up to 256 bytes
    assert saved >= bytes16 // 2 - bytes4 - scratch                  # the issue's floor: one 16-bit copy minus the 4-bit size minus the scratch


def test_prefill_equals_the_twin_bit_for_bit(geo):
    """(a) hidden rows, last row (through the step-0 logits) of a single prompt, a run of three, and prefill_append cut at two places"""
    cfg, e4, tw, emb, E, frames, sd, kind = geo
    L = emb.shape[0]
    for want_hidden in (True, False):
        h4, ht = e4.prefill(0, L, embeds=emb, want_hidden=want_hidden), tw.prefill(0, L, embeds=emb, want_hidden=want_hidden)
        if want_hidden:
            assert torch.equal(h4, ht), "hidden rows"
        a, b = (e.decode_begin([0], [1], 8, eos=-1, want_logits=True).clone() for e in (e4, tw))
        assert torch.equal(a, b), "step-0 logits"
    single = a
    three = [emb.contiguous(), (emb.float() * 0.5).to(BF).contiguous(), (emb.float() * -0.25).to(BF).contiguous()]
    for e in (e4, tw):
        e.prefill_multi(1, three)
    a, b = (e.decode_begin([1, 2, 3], [1] * 3, 8, eos=-1, want_logits=True).clone() for e in (e4, tw))
    assert torch.equal(a, b) and torch.equal(a[:1], single), "a run of three"
    for cut in (33, 66):
        res = []
        for e in (e4, tw):
            e.prefill(4, cut, embeds=emb[:cut])
            hid = e.prefill_append(4, cut, embeds=emb[cut:], want_hidden=True)
            res.append((hid.clone(), e.decode_begin([4], [1], 8, eos=-1, want_logits=True).clone()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), f"prefill_append at {cut}"
        assert torch.equal(res[0][1], single), f"a row's bits depend on the cut at {cut}"


def _forced(cfg):
    """12 fed ids that cross all three heads starting from the time head: time digits, time-<sync> -> score head, score ids, score-<sync> -> text head,
    text ids, <sync> -> time head, time digits"""
    V, Tv = cfg.vocab_size, cfg.time_vocab_size
    t, s = V + 1, V + 1 + Tv
    return [t + 3, t + 5, t + 2, t, s + 4, s + 2, s, 17, 101, V, t + 7, t + 1]


def _decode(eng, emb, B, forced, use_graph=False):
    """[13, B, NV] logits of decode_begin + 12 forced steps, and the recorded ids"""
    L = emb.shape[0]
    for b in range(B):
        eng.prefill(b, L, embeds=(emb.float() * (1.0 - 0.02 * b)).to(BF))
    n = len(forced) + 1
    lg = [eng.decode_begin(list(range(B)), [1] * B, n, eos=-1, forced=[forced] * B, want_logits=True).clone()]
    for _ in range(n - 1):
        lg.append(eng.decode_steps(1, use_graph=use_graph, want_logits=True).clone())
    ids, _ = eng.decode_read()
    return torch.stack(lg), [list(r) for r in ids]


@pytest.fixture(scope="module")
def twin_bound(geo):
    """2 D of the module's docstring for this geometry: the twin's GEMV step against its own fused-norm step"""
    cfg, e4, tw, emb, E, frames, sd, kind = geo
    forced = _forced(cfg)
    d = 0.0
    for B in (1, 3):
        with ops.tuned(decode__fuse_norm_rows=4):
            assert ops.decode_route(B, 0, cfg.hidden_size, cfg.intermediate_size, 6144)["step"] == 2
            fused, _ = _decode(tw, emb, B, forced)
        with ops.tuned(decode__fuse_norm_rows=0):
            assert ops.decode_route(B, 0, cfg.hidden_size, cfg.intermediate_size, 6144)["step"] == 1
            plain, _ = _decode(tw, emb, B, forced)
        fin = torch.isfinite(plain)
        assert torch.equal(fin, torch.isfinite(fused))
        d = max(d, (plain[fin] - fused[fin]).abs().max().item())
    record(f"{kind}: twin, GEMV step against fused-norm step, 12 forced steps, B = 1 and 3: D = max |dlogit| = {d:.6f}; bound 2 D = {2 * d:.6f}")
    assert d > 0
    return 2 * d


@pytest.mark.parametrize("B", (1, 3, 33))
def test_forced_decode_stays_within_the_twins_own_bound(geo, twin_bound, B):
    """(b) 12 forced steps over all three heads: logits within 2 D of the twin, ids equal wherever the twin's top-2 margin exceeds 2 D"""
    cfg, e4, tw, emb, E, frames, sd, kind = geo
    forced = _forced(cfg)
    with ops.tuned(decode__fuse_norm_rows=0):
        ref, rid = _decode(tw, emb, B, forced)
    got, gid = _decode(e4, emb, B, forced)
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(got)), "head masks differ"
    err = (got[fin] - ref[fin]).abs().max().item()
    srt = torch.sort(torch.where(fin, ref, torch.full_like(ref, -1e30)), dim=-1, descending=True).values
    margin = srt[..., 0] - srt[..., 1]
    gated = margin > twin_bound                                       # [13, B]
    record(f"{kind}: w4 engine against its twin, B = {B}: max |dlogit| = {err:.6f} (bound {twin_bound:.6f}); {int(gated.sum())} of {gated.numel()} steps have a "
           f"margin above it")
    if B == 33:                                                       # for information: the twin's own two summation orders at this batch size
        assert ops.decode_route(B, 0, cfg.hidden_size, cfg.intermediate_size, 6144)["step"] == 3      # (ref above: the twin's default, the wide GEMM step)
        with ops.tuned(decode__wide_min_rows=65):
            assert ops.decode_route(B, 0, cfg.hidden_size, cfg.intermediate_size, 6144)["step"] == 1
            gemv, _ = _decode(tw, emb, B, forced)
        record(f"{kind}: twin, wide GEMM step against GEMV step, B = 33: max |dlogit| = {(gemv[fin] - ref[fin]).abs().max().item():.6f} (not part of the bound)")
    assert gated.float().mean().item() >= 0.9, "the margin condition leaves out more than one step in ten"
    assert err <= twin_bound, (err, twin_bound)
    own = got.argmax(-1)                                              # the model's own choice at every step (forced ids are what is fed)
    assert torch.equal(own[gated], ref.argmax(-1)[gated])
    rec4, rect = torch.tensor(gid).t(), torch.tensor(rid).t()         # the ids the steps recorded, [13, B]: the same rule, read back through decode_read
    assert torch.equal(rec4[gated.cpu()], rect[gated.cpu()])


def test_graph_replay_equals_eager_and_runs_repeat(geo):
    """(c)"""
    cfg, e4, tw, emb, E, frames, sd, kind = geo
    L = emb.shape[0]
    for B in (1, 3):
        res = []
        for g in (False, True, True):
            for b in range(B):
                e4.prefill(b, L, embeds=(emb.float() * (1.0 - 0.25 * b)).to(BF))
            lg0 = e4.decode_begin(list(range(B)), [1] * B, 16, eos=-1, want_logits=True).clone()
            if g:
                e4.decode_steps(5, use_graph=True)
            else:
                for _ in range(5):
                    e4.decode_steps(1, use_graph=False)
            lg6 = e4.decode_steps(1, use_graph=False, want_logits=True).clone()
            res.append((e4.decode_read()[0], lg0, lg6))
        for r in res[1:]:
            assert r[0] == res[0][0] and torch.equal(r[1], res[0][1]) and torch.equal(r[2], res[0][2]), B


def test_batch_of_65_is_refused(pair):
    cfg, e4, tw, emb, E, frames, sd = pair
    from trace_amd import _lib
    big = TraceEngine(cfg, max_batch=66, max_ctx=128, max_frames=4, max_new_tokens=8, llm_w4=True)
    try:
        assert big.decode_batch_max == 64
        big.load_weights(sd.items())
        with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_decode_begin: bad batch \(at most 64 sequences decode together\)"):
            big.decode_begin(list(range(65)), [1] * 65, 4)
    finally:
        big.close()


def test_public_api_on_a_w4_model(pair):
    """generate greedy and sampled, score(continuations=...), and the prefix cache: a second question bit-identical to the uncached call"""
    from trace_amd.model.trace_mistral import TraceMistralForCausalLM
    cfg, e4, tw, emb, E, frames, sd = pair
    m = TraceMistralForCausalLM(cfg, e4)
    V, Tv = cfg.vocab_size, cfg.time_vocab_size
    ids = torch.from_numpy(E["input_ids"]).long()
    q2 = ids.clone()
    cut = ids.tolist().index(-201) + 1
    q2[cut:-1] = (q2[cut:-1] + 17) % (V - 3) + 3
    kw = dict(images_or_videos=[frames], video_timestamps=[E["timestamps"].tolist()])
    gkw = dict(heads=[1], max_new_tokens=10, eos_token_id=-1, **kw)
    conts = [[V + 1 + 3, V + 1 + 4, V + 1], [V + 1 + 2, V + 1, V + 1 + Tv + 3, V + 1 + Tv], [V + 1 + 9]]
    g1, g2 = m.generate(ids, **gkw), m.generate(q2, **gkw)
    assert g1.shape[-1] == 10
    torch.manual_seed(11)
    s1 = m.generate(ids, do_sample=True, temperature=0.8, top_k=5, **gkw)
    torch.manual_seed(11)
    assert torch.equal(s1, m.generate(ids, do_sample=True, temperature=0.8, top_k=5, **gkw))
    sc = m.score(q2, continuations=conts, **kw)
    assert all(np.isfinite(x).all() for x in sc.logprobs)
    m.enable_prefix_cache(True)
    try:
        rows0 = e4.stats["prefill_rows"]
        assert torch.equal(m.generate(ids, **gkw), g1)               # the miss
        rows1 = e4.stats["prefill_rows"]
        assert torch.equal(m.generate(q2, **gkw), g2)                # the hit: only the rows after <video> are prefilled
        rows2 = e4.stats["prefill_rows"]
        assert rows2 - rows1 < rows1 - rows0
        hit = m.score(q2, continuations=conts, **kw)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(hit.logprobs, sc.logprobs))
    finally:
        m.enable_prefix_cache(False)
