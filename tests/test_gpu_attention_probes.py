"""The attention kernels on inputs where every key counts (tests/attn_probes.py), against float64 references computed on the device with the mask
stated explicitly: the decode attention at the engine's own (batch, split) pairs and block / split / slot edges, always over poisoned caches; its
fused prologue and qkv_finish_kernel (sums, RoPE, cache append, the splice of the newest row) through trace_op_qkv_finish /
trace_op_attn_decode_fused; the causal GQA kernel in its prefill, batched and append forms; the three ViT kernels at their routing edges.
tests/test_attn_probes_cpu.py shows that the judge and bounds used here reject a kernel that loses, gains or misweighs a single key."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import attn_probes as P  # noqa: E402
from trace_amd import _lib  # noqa: E402
from trace_amd.engine import ops  # noqa: E402

DEV = torch.device("cuda", 0)
NQ, NKV, HD = 32, 8, 128
SCALE = 1 / math.sqrt(HD)
MARGINS = {}                       # (kernel, probe) -> [E, max |got - ref|, max err / bound]


def judge(kernel, probe, got, r, name):
    ratio, err = (P.attention_error_ratio(got, r) if probe != "uniform" else
                  (float(torch.nan_to_num((got.double() - r.ref).abs() / (P.RTOL * r.ref.abs()), nan=0.0, posinf=float("inf")).max()),
                   float((got.double() - r.ref).abs().max())))
    m = MARGINS.setdefault((kernel, probe), [0.0, 0.0, 0.0])
    m[0], m[1], m[2] = max(m[0], r.E), max(m[1], err), max(m[2], ratio)
    (P.assert_uniform_close if probe == "uniform" else P.assert_attention_close)(got, r, f"{kernel} {probe} {name}")


@pytest.fixture(scope="module", autouse=True)
def margins_record():
    """the measured margins (per kernel and probe: E, max |got - ref|, the largest error / bound) are printed, and appended to the file that the
    environment variable TRACE_ATTN_PROBE_MARGINS names, if it is set: the record profiles/attn_probe_margins.txt is made from"""
    yield
    lines = [f"{k:<18} {p:<10} E {m[0]:.3e}  max|got-ref| {m[1]:.3e}  max err/bound {m[2]:.3f}" for (k, p), m in sorted(MARGINS.items())]
    print("\n".join(lines))
    path = os.environ.get("TRACE_ATTN_PROBE_MARGINS")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
def decode_probe_set(ctxs, max_ctx, nsplit, dtype, seed):
    B = len(ctxs)
    pos = torch.tensor([c - 1 for c in ctxs], dtype=torch.int32, device=DEV)
    nvis = pos.long() + 1
    s = {"uniform": P.probe_uniform(B, NQ, NKV, 1, max_ctx, HD, dtype, seed, DEV),
         "pointer": P.probe_pointer(P.decode_pointer_target_tensor(ctxs, NQ, nsplit, DEV), NQ, NKV, max_ctx, HD, dtype, seed + 1, DEV),
         "ramp_up": P.probe_ramp(nvis, B, NQ, NKV, 1, max_ctx, HD, SCALE, dtype, True, seed + 2, DEV),
         "ramp_down": P.probe_ramp(nvis, B, NQ, NKV, 1, max_ctx, HD, SCALE, dtype, False, seed + 3, DEV)}
    for q, k, v in s.values():
        P.poison_decode(q, k, v, pos)
    return s, pos


def run_attn_decode(q, k, v, pos, nsplit):
    """canonical q [B, H, 1, hd], k / v [B, KVH, max_ctx, hd] -> [B, H, 1, hd]; the caches get one more slot behind the batch, filled with 3e4"""
    B = q.shape[0]
    other = torch.full((1,) + tuple(k.shape[1:]), P.POISON_OTHER_SLOT, dtype=k.dtype, device=DEV)
    kc = torch.cat([k, other])
    vt = torch.cat([v, other]).transpose(2, 3).contiguous()
    o = ops.attn_decode(q[:, :, 0, :].reshape(B, -1).contiguous(), kc, None, pos, nsplit, SCALE, vtcache=vt)
    return o.view(B, NQ, 1, HD)


def decode_launches(B, nsplit, max_ctx):
    """context lists of B rows each that together hold every context of P.decode_contexts (a batch that has room holds all of them at once)"""
    need = P.decode_contexts(nsplit, max_ctx)
    if B >= len(need):
        g = torch.Generator().manual_seed(B * 131 + nsplit)
        fill = torch.randint(1, max_ctx + 1, (B - len(need),), generator=g).tolist()
        return [need + fill]
    n = -(-len(need) // B)
    return [[need[(l * B + b) % len(need)] for b in range(B)] for l in range(n)]


def check_decode(B, max_ctx, splits, dtype=torch.bfloat16, kernel="attn_decode"):
    for nsplit in splits:
        for li, ctxs in enumerate(decode_launches(B, nsplit, max_ctx)):
            probes, pos = decode_probe_set(ctxs, max_ctx, nsplit, dtype, seed=1000 * B + 10 * nsplit + li)
            vis = P.decode_visible(pos, max_ctx)
            for pn, (q, k, v) in probes.items():
                r = P.reference(q, k, v, vis, SCALE, False)
                got = run_attn_decode(q, k, v, pos, nsplit)
                judge(kernel, pn, got, r, f"B {B} nsplit {nsplit} max_ctx {max_ctx} ctxs {ctxs[:16]}")


@pytest.mark.parametrize("B", [1, 3, 8, 32, 128])
def test_decode_probes(B):
    """every batch at the engine's own split count and at 1 / 5 / 16 / 32 splits; contexts 1, 31, 32, 33, 64, 65, 127, 128, 129, 32 nsplit,
    32 nsplit + 1, one whose last split holds a single key, 2047 and 2048 = max_ctx; all four probes over poisoned caches"""
    check_decode(B, 2048, sorted({P.decode_nsplit(B), 1, 5, 16, 32}))


@pytest.mark.parametrize("B", [1, 8])
def test_decode_probes_ctx_4096(B):
    check_decode(B, 4096, sorted({P.decode_nsplit(B), 16}))


@pytest.mark.parametrize("B", [8, 128])
def test_decode_probes_three_wave_build(B):
    with ops.tuned(attn__decode__waves=1):
        check_decode(B, 2048, sorted({P.decode_nsplit(B), 16}), kernel="attn_decode(3w)")


def test_decode_probes_fp16_library():
    try:
        ops.use("f16")
        check_decode(3, 2048, [P.decode_nsplit(3)], dtype=torch.float16, kernel="attn_decode(f16)")
    finally:
        ops.use("bf16")


def test_decode_back_to_back_launches_share_the_tickets():
    """launches with different split counts queued on one stream without a synchronisation in between (every merge re-zeroes its ticket for the
    next launch) give the bits of the same launches run apart"""
    ctxs = P.decode_contexts(16, 2048)[:8]
    probes, pos = decode_probe_set(ctxs, 2048, 16, torch.bfloat16, seed=77)
    q, k, v = probes["pointer"]
    splits = [16, 5, 32, 2, 16, 1, 13]
    apart = []
    for ns in splits:
        torch.cuda.synchronize()
        apart.append(run_attn_decode(q, k, v, pos, ns).clone())
        torch.cuda.synchronize()
    kc = torch.cat([k, torch.full_like(k[:1], P.POISON_OTHER_SLOT)])
    vt = torch.cat([v, torch.full_like(v[:1], P.POISON_OTHER_SLOT)]).transpose(2, 3).contiguous()
    q2 = q[:, :, 0, :].reshape(len(ctxs), -1).contiguous()
    torch.cuda.synchronize()
    queued = [ops.attn_decode(q2, kc, None, pos, ns, SCALE, vtcache=vt) for ns in splits]
    torch.cuda.synchronize()
    for ns, a, b in zip(splits, apart, queued):
        assert torch.equal(a.reshape(-1), b.reshape(-1)), ns


# ---- the fused prologue and qkv_finish ------------------------------------------------------------------------------------------------------
def rope_tables(max_ctx):
    inv = 10000.0 ** (-torch.arange(64, dtype=torch.float64) / 64)
    ang = torch.arange(max_ctx, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().to(DEV), ang.sin().float().to(DEV)


def prologue_reference(part, pos, cos_t, sin_t, dtype):
    """the documented prologue: the partial rows summed in chunk order in fp32, rounded to the element type; rotate-half RoPE of the q and k heads
    in float64 from the tables, rounded -> (q [B, NQ, 128], k [B, NKV, 128], v [B, NKV, 128])"""
    B = pos.shape[0]
    x = part[0, :B].clone()
    for c in range(1, part.shape[0]):
        x = x + part[c, :B]
    x = x.to(dtype).view(B, NQ + 2 * NKV, HD)
    h = x[:, :NQ + NKV].double()
    c, s = cos_t[pos.long()].double()[:, None, :], sin_t[pos.long()].double()[:, None, :]
    x1, x2 = h[..., :64], h[..., 64:]
    roped = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(dtype)
    return roped[:, :NQ], roped[:, NQ:], x[:, NQ + NKV:]


def fused_case(poss, ks, nsplit, max_ctx, dtype, seed):
    B = len(poss)
    S = 2 * B + 1
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *shape: torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)
    pos = torch.tensor(poss, dtype=torch.int32, device=DEV)
    slots = torch.tensor([S - 1 - 2 * b for b in range(B)], dtype=torch.int32, device=DEV)           # reversed, with gaps
    cos_t, sin_t = rope_tables(max_ctx)
    # raw rows: q of the first head of a group = 3 x the new k (it points at the newest key); the other q heads are 3 x Gaussian and get their key below
    k_raw, v_raw = rn(B, NKV, HD), rn(B, NKV, HD)
    q_raw = 3.0 * rn(B, NQ, HD)
    q_raw[:, ::4] = 3.0 * k_raw
    want = torch.cat([q_raw, k_raw, v_raw], 1).reshape(B, -1)
    part = torch.zeros((ks, ops.sk_rows(), want.shape[1]), dtype=torch.float32, device=DEV)
    for c in range(ks - 1):
        part[c, :B] = 0.5 * rn(*want.shape)
    part[ks - 1, :B] = want - part[:ks - 1, :B].sum(0)
    q_ref, k_ref, v_ref = prologue_reference(part, pos, cos_t, sin_t, dtype)
    # caches: Gaussian below pos, poison from pos on (the append overwrites pos itself), 3e4 in every slot no row uses
    kc = torch.full((S, NKV, max_ctx, HD), P.POISON_OTHER_SLOT, dtype=dtype, device=DEV)
    vc = torch.full((S, NKV, max_ctx, HD), P.POISON_OTHER_SLOT, dtype=dtype, device=DEV)
    k = rn(B, NKV, max_ctx, HD).to(dtype)
    v = rn(B, NKV, max_ctx, HD).to(dtype)
    for b, p in enumerate(poss):                     # heads 1..3 of every group point at pos - 1, 0 and pos // 2 (where those are distinct old keys)
        taken = set()
        for hq, t in ((1, p - 1), (2, 0), (3, p // 2)):
            if 0 <= t < p and t not in taken:
                taken.add(t)
                k[b, :, t] = (q_ref[b, hq::4].float() / 3.0).to(dtype)
    P.poison_decode(q_ref[:, :, None, :], k, v, pos - 1)
    sl = slots.long()
    kc[sl], vc[sl] = k, v
    vt = vc.transpose(2, 3).contiguous()
    # the reference attention: the cache with the REFERENCE's new row in place
    kr, vr = k.clone(), v.clone()
    bi = torch.arange(B, device=DEV)
    kr[bi, :, pos.long()] = k_ref
    vr[bi, :, pos.long()] = v_ref
    r = P.reference(q_ref[:, :, None, :].contiguous(), kr, vr, P.decode_visible(pos, max_ctx), SCALE, False)
    return dict(part=part, pos=pos, slots=slots, cos=cos_t, sin=sin_t, kc=kc, vt=vt, q_ref=q_ref, k_ref=k_ref, v_ref=v_ref, ref=r, B=B, S=S)


def check_fused(poss, ks, nsplit, max_ctx=2048, dtype=torch.bfloat16, seed=0, kernel="attn_decode_fused"):
    c = fused_case(poss, ks, nsplit, max_ctx, dtype, seed)
    B, pos, sl, bi = c["B"], c["pos"].long(), c["slots"].long(), torch.arange(c["B"], device=DEV)
    name = f"B {B} ks {ks} nsplit {nsplit} pos {poss[:16]}"
    kA, vA = c["kc"].clone(), c["vt"].clone()
    out_f = ops.attn_decode_fused(c["part"], kA, vA, c["slots"], c["pos"], c["cos"], c["sin"], NQ, nsplit, SCALE)
    kB, vB = c["kc"].clone(), c["vt"].clone()
    q_rows = ops.qkv_finish(c["part"], kB, vB, c["slots"], c["pos"], c["cos"], c["sin"], NQ)
    # the prologue: within one unit in the last place of the float64 reference, bit-equal between the two kernels
    k_new, v_new = kB[sl, :, pos], vB[sl, :, :, pos]                                               # [B, NKV, 128] each
    for what, got, ref in (("q rows", q_rows.view(B, NQ, HD), c["q_ref"]), ("K row", k_new, c["k_ref"]), ("V^T column", v_new, c["v_ref"])):
        d = P.ulp_distance(got, ref)
        assert int(d.max()) <= 1, f"{what} {name}: {int((d > 1).sum())} elements more than one ulp off the reference (max {int(d.max())})"
    assert torch.equal(kA, kB) and torch.equal(vA, vB), f"{name}: the fused prologue and qkv_finish appended different bits"
    # nothing but the B appended rows / columns was written
    k0, v0 = c["kc"].clone(), c["vt"].clone()
    k0[sl, :, pos], v0[sl, :, :, pos] = k_new, v_new
    assert torch.equal(k0, kB) and torch.equal(v0, vB), f"{name}: the append wrote outside its row / column"
    # the attention itself, and the fused launch against finish + unfused on the same cache (gathered into slot order for the identity-slot op)
    judge(kernel, "pointer", out_f.view(B, NQ, 1, HD), c["ref"], name)
    out_u = ops.attn_decode(q_rows, kB[sl].contiguous(), None, c["pos"], nsplit, SCALE, vtcache=vB[sl].contiguous())
    assert torch.equal(out_f, out_u), f"{name}: fused output differs from qkv_finish + attn_decode"


BASES = (0, 32, 64, 96, 480, 2016)              # the newest position in the first block, in a block of each wave, in the last of 16 splits, at the end of the slot
KS = (1, 3, 4, 5, 14)


def test_fused_prologue_batch_1():
    """pos % 32 = every value (the splice's 32 register / half-word paths), ks 1 / 3 / 4 / 5 / 14, the engine's 16 splits"""
    ns = P.decode_nsplit(1)
    for r in range(32):
        check_fused([BASES[r % 6] + r], KS[r % 5], ns, seed=r)
    for i, p in enumerate((0, 480, 2047, 2016, 1023)):           # alone in the cache; alone in the last split; the last position of the slot
        check_fused([p], KS[i], ns, seed=100 + i)


def test_fused_prologue_batch_4():
    ns = P.decode_nsplit(4)
    for l in range(8):
        check_fused([BASES[(l + b) % 6] + 4 * l + b for b in range(4)], KS[l % 5], ns, seed=200 + l)
    check_fused([2047, 32 * (ns - 1), 0, 31], 14, ns, seed=300)    # 32 (nsplit - 1): the newest key alone in the last split


def test_fused_prologue_batch_128():
    ns = P.decode_nsplit(128)
    poss = [BASES[(b // 32 + b) % 6] + b % 32 for b in range(128)]
    poss[127] = 2047
    check_fused(poss, 5, ns, seed=400)


def test_fused_prologue_fp16_library():
    try:
        ops.use("f16")
        check_fused([2016 + 31, 480, 33, 7], 3, P.decode_nsplit(4), dtype=torch.float16, seed=500, kernel="attn_decode_fused(f16)")
    finally:
        ops.use("bf16")


def test_decode_entry_points_refuse_what_their_arrays_cannot_hold():
    """a batch above trace_op_sk_rows(), a slot outside the caches or given twice, a position outside the slot: TRACE_ERR_ARG, nothing launched"""
    rows = ops.sk_rows()
    B, max_ctx = rows + 1, 32
    kc = torch.zeros((B, NKV, max_ctx, HD), dtype=torch.bfloat16, device=DEV)
    pos = torch.zeros((B,), dtype=torch.int32, device=DEV)
    q = torch.zeros((B, NQ * HD), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.TraceHipError, match="trace_op_attn_decode"):
        ops.attn_decode(q, kc, None, pos, 1, SCALE, vtcache=kc.transpose(2, 3).contiguous())
    cos_t, sin_t = rope_tables(max_ctx)
    part = torch.ones((1, rows, (NQ + 2 * NKV) * HD), dtype=torch.float32, device=DEV)
    vt = kc.transpose(2, 3).contiguous()
    slots = torch.arange(B, dtype=torch.int32, device=DEV)
    for bad_slots, bad_pos in ((slots, pos), (torch.tensor([0, 4], dtype=torch.int32, device=DEV), pos[:2]),
                               (torch.tensor([1, 1], dtype=torch.int32, device=DEV), pos[:2]),
                               (slots[:2], torch.tensor([0, max_ctx], dtype=torch.int32, device=DEV)),
                               (torch.tensor([0, -1], dtype=torch.int32, device=DEV), pos[:2])):
        k4, v4 = kc[:4], vt[:4]
        kk, vv = (kc, vt) if bad_slots.numel() > 2 else (k4, v4)
        with pytest.raises(_lib.TraceHipError, match="trace_op_qkv_finish"):
            ops.qkv_finish(part, kk, vv, bad_slots, bad_pos, cos_t, sin_t, NQ)
        with pytest.raises(_lib.TraceHipError, match="trace_op_attn_decode_fused"):
            ops.attn_decode_fused(part, kk, vv, bad_slots, bad_pos, cos_t, sin_t, NQ, 1, SCALE)
    torch.cuda.synchronize()
    assert not kc.any() and not vt.any()


# ---- causal GQA (head_dim 128) ------------------------------------------------------------------------------------------------------------
def run_attention(q, k, v, causal, scale):
    """canonical layout -> ops.attention's token-major one and back"""
    o = ops.attention(q.permute(0, 2, 1, 3).contiguous(), k.permute(0, 2, 1, 3).contiguous(), v.permute(0, 2, 1, 3).contiguous(), causal, scale)
    return o.permute(0, 2, 1, 3)


def check_causal(B, nq, nkv, KVH, dtype=torch.bfloat16, kernel="attn_causal"):
    H = 4 * KVH
    vis = P.causal_visible(B, nq, nkv, DEV)
    nvis = torch.full((B,), nkv, device=DEV)
    seed = 7 * nq + nkv + KVH
    probes = {"uniform": P.probe_uniform(B, H, KVH, nq, nkv, HD, dtype, seed, DEV),
              "pointer": P.probe_pointer(P.causal_pointer_targets(B, H, nq, nkv, DEV), H, KVH, nkv, HD, dtype, seed + 1, DEV),
              "ramp_up": P.probe_ramp(nvis, B, H, KVH, nq, nkv, HD, SCALE, dtype, True, seed + 2, DEV),
              "ramp_down": P.probe_ramp(nvis, B, H, KVH, nq, nkv, HD, SCALE, dtype, False, seed + 3, DEV)}
    for pn, (q, k, v) in probes.items():
        r = P.reference(q, k, v, vis, SCALE, True)
        judge(kernel, pn, run_attention(q, k, v, True, SCALE), r, f"B {B} nq {nq} nkv {nkv} kv heads {KVH}")


CAUSAL_L = (1, 31, 32, 33, 64, 65, 127, 128, 129, 333, 1086, 1967)


@pytest.mark.parametrize("KVH", [1, 2, 8])
def test_causal_probes_prefill(KVH):
    for L in CAUSAL_L:
        check_causal(1, L, L, KVH)


@pytest.mark.parametrize("KVH", [1, 2, 8])
@pytest.mark.parametrize("B", [3, 8])
def test_causal_probes_batched(B, KVH):
    for L in CAUSAL_L:
        check_causal(B, L, L, KVH)


@pytest.mark.parametrize("KVH", [1, 2, 8])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_causal_probes_append(B, KVH):
    """fewer query rows than keys: what a prefill continuation launches, and (nq = 1) the prefill's last layer"""
    for nq, nkv in ((1, 200), (1, 1967), (7, 64), (40, 333), (33, 1999), (128, 2048)):
        check_causal(B, nq, nkv, KVH, kernel="attn_causal(append)")


def test_causal_probes_fp16_library():
    try:
        ops.use("f16")
        check_causal(1, 333, 333, 2, dtype=torch.float16, kernel="attn_causal(f16)")
        check_causal(1, 40, 333, 2, dtype=torch.float16, kernel="attn_causal(f16)")
    finally:
        ops.use("bf16")


# ---- ViT (head_dim 64) ----------------------------------------------------------------------------------------------------------------------
def vit_kernel(n, variant):
    """the routing of launch_attn_vit for self-attention over n tokens, restated: row-major V (attn_vit_wants_perm) needs >= 128 keys and at most
    TAILV = 8 keys past the last whole 64-key tile; the 192-row kernel (attn_vit_big_ok; variants 191 / 192) on top of that >= 192 rows of which 192
    leaves at most BIG_MAXLEFT = 4 over and at most BIG_MAXKV = 1024 keys; everything else goes to the generic kernel"""
    perm = n >= 128 and n % 64 <= 8
    if variant != 190 and perm and n >= 192 and n % 192 <= 4 and n <= 1024:
        return "attn_vit_192row"
    return "attn_vit_4x32row" if perm else "attn_vit_generic"


# n -> the kernel it reaches under variant 192 (written out, so that a change of the routing or of its restatement above is noticed)
VIT_SHAPES = {17: "generic", 64: "generic", 100: "generic", 127: "generic", 128: "4x32row", 129: "4x32row", 136: "4x32row", 137: "generic",
              192: "192row", 193: "192row", 196: "192row", 197: "4x32row", 384: "192row", 385: "192row", 388: "192row", 389: "4x32row",
              576: "192row", 577: "192row", 584: "4x32row", 585: "generic", 776: "4x32row", 960: "192row", 964: "192row", 1024: "4x32row",
              1025: "4x32row", 1152: "4x32row", 1153: "4x32row"}
VIT_BATCH_HEADS = ((1, 1), (2, 3), (1, 5), (3, 3), (1, 4))       # (frame, head) pairs: 1, 6, 5, 9 leave the last quad partly empty


@pytest.mark.parametrize("n", list(VIT_SHAPES))
def test_vit_probes(n):
    assert vit_kernel(n, 192) == vit_kernel(n, 191) == "attn_vit_" + VIT_SHAPES[n]
    B, H = VIT_BATCH_HEADS[list(VIT_SHAPES).index(n) % len(VIT_BATCH_HEADS)]
    if n == 577:
        B, H = 3, 16
    scale = 0.125
    vis = P.full_visible(B, n, n, DEV)
    nvis = torch.full((B,), n, device=DEV)
    dt = torch.bfloat16
    probes = {"uniform": P.probe_uniform(B, H, H, n, n, 64, dt, n, DEV),
              "pointer": P.probe_pointer(P.vit_pointer_targets(B, H, n, n, DEV), H, H, n, 64, dt, n + 1, DEV),
              "ramp_up": P.probe_ramp(nvis, B, H, H, n, n, 64, scale, dt, True, n + 2, DEV),
              "ramp_down": P.probe_ramp(nvis, B, H, H, n, n, 64, scale, dt, False, n + 3, DEV)}
    for pn, (q, k, v) in probes.items():
        r = P.reference(q, k, v, vis, scale, True)
        outs = {}
        for var in (190, 191, 192):
            with ops.tuned(attn__vit__big=var - 190):
                outs[var] = run_attention(q, k, v, False, scale)
        for var in (190, 191, 192):
            judge(vit_kernel(n, var), pn, outs[var], r, f"variant {var} n {n} B {B} heads {H}")
        assert torch.equal(outs[191], outs[192]), f"{pn} n {n}: the ring depth changed the arithmetic"
        if vit_kernel(n, 192) == vit_kernel(n, 190):
            assert torch.equal(outs[190], outs[192]), f"{pn} n {n}: variants 190 and 192 were expected to reach the same kernel"
