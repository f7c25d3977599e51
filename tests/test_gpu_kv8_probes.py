"""The kernels of the e4m3 KV cache (trace_amd/csrc/kv8.hip) over loose arrays: the decode attention on the probes of tests/attn_probes.py quantised
with kv8.pack_cache_ref and judged against tests/kv8_probes.py's reference (the judge and bounds are the 16-bit tests', unchanged;
tests/test_kv8_cpu.py shows that they reject a mishandled scale, key or layout); kv8_pack / kv8_unpack against the torch statement of the format, bit
for bit; qkv_finish_kv8 against the 16-bit qkv_finish through that statement."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a HIP device", allow_module_level=True)

import attn_probes as P  # noqa: E402
import kv8_probes as K8  # noqa: E402
import test_gpu_attention_probes as T16  # noqa: E402  (fused_case, prologue_reference, rope_tables: the 16-bit tests' own cases)
from trace_amd import _lib, kv8  # noqa: E402
from trace_amd.engine import ops  # noqa: E402

DEV = torch.device("cuda", 0)
NQ, NKV, HD = 32, 8, 128
SCALE = 1 / math.sqrt(HD)


def judge(probe, got, r, name):
    ratio, err = P.attention_error_ratio(got, r)
    print(f"attn_decode_kv8 {probe:<9} {name}: E {r.E:.3e} max|got-ref| {err:.3e} max err/bound {ratio:.3f}")
    (P.assert_uniform_close if probe == "uniform" else P.assert_attention_close)(got, r, f"attn_decode_kv8 {probe} {name}")


# ---- decode attention ----------------------------------------------------------------------------------------------------------------------
def kv8_probe_set(ctxs, max_ctx, nsplit, dtype, seed):
    """the four probes of the 16-bit decode test, poisoned past pos and packed; one more slot of poison behind the batch"""
    probes, pos = T16.decode_probe_set(ctxs, max_ctx, nsplit, dtype, seed)          # (already poisoned there: poisoning twice changes nothing)
    out = {}
    for pn, (q, k, v) in probes.items():
        out[pn] = (q,) + K8.quantise_probe(q, k, v, pos)
    return out, pos


def run_attn_decode_kv8(q, k8, v8, ks, vs, pos, nsplit):
    B = q.shape[0]
    a = K8.with_poison_slot(k8, v8, ks, vs)
    o = ops.attn_decode_kv8(q[:, :, 0, :].reshape(B, -1).contiguous(), a[0], a[1], a[2], a[3], pos, nsplit, SCALE)
    return o.view(B, NQ, 1, HD)


def check_decode(B, max_ctx, splits, dtype=torch.bfloat16):
    for nsplit in splits:
        for li, ctxs in enumerate(T16.decode_launches(B, nsplit, max_ctx)):
            probes, pos = kv8_probe_set(ctxs, max_ctx, nsplit, dtype, seed=1000 * B + 10 * nsplit + li)
            vis = P.decode_visible(pos, max_ctx)
            for pn, (q, k8, v8, ks, vs) in probes.items():
                r = K8.reference_kv8(q, k8, ks, v8, vs, vis, SCALE)
                got = run_attn_decode_kv8(q, k8, v8, ks, vs, pos, nsplit)
                judge(pn, got, r, f"B {B} nsplit {nsplit} max_ctx {max_ctx} ctxs {ctxs[:16]}")


@pytest.mark.parametrize("B", [1, 3, 8, 128])
def test_decode_probes(B):
    """every batch at the engine's own split count and at 1 and 16 splits; contexts 1, 31, 32, 33, 64, 65, 127, 128, 129, 32 nsplit, 32 nsplit + 1, one
    whose last split holds a single key, 2047 and 2048 = max_ctx; all four probes over poisoned arrays"""
    check_decode(B, 2048, sorted({P.decode_nsplit(B), 1, 16}))


def test_decode_probes_ctx_4096():
    check_decode(1, 4096, [P.decode_nsplit(1)])


def test_decode_probes_fp16_library():
    try:
        ops.use("f16")
        check_decode(3, 2048, [P.decode_nsplit(3)], dtype=torch.float16)
    finally:
        ops.use("bf16")


def test_decode_back_to_back_launches_share_the_tickets():
    """launches with different split counts, one after the other on one stream with nothing resetting the tickets in between (every merge re-zeroes
    its ticket for the next launch; the op itself reads the positions back before each launch, so the host does wait between them), give the bits of
    the same launches run apart"""
    ctxs = P.decode_contexts(16, 2048)[:8]
    probes, pos = kv8_probe_set(ctxs, 2048, 16, torch.bfloat16, seed=77)
    q, k8, v8, ks, vs = probes["pointer"]
    splits = [16, 5, 32, 2, 16, 1, 13]
    apart = []
    for ns in splits:
        torch.cuda.synchronize()
        apart.append(run_attn_decode_kv8(q, k8, v8, ks, vs, pos, ns).clone())
        torch.cuda.synchronize()
    a = K8.with_poison_slot(k8, v8, ks, vs)
    q2 = q[:, :, 0, :].reshape(len(ctxs), -1).contiguous()
    torch.cuda.synchronize()
    queued = [ops.attn_decode_kv8(q2, a[0], a[1], a[2], a[3], pos, ns, SCALE) for ns in splits]
    torch.cuda.synchronize()
    for ns, x, y in zip(splits, apart, queued):
        assert torch.equal(x.reshape(-1), y.reshape(-1)), ns


# ---- kv8_pack / kv8_unpack -------------------------------------------------------------------------------------------------------------------
def sentinel_arrays(S, nkv, max_ctx):
    """arrays no kernel output can be mistaken for: bytes 0x11, scales 7"""
    return (torch.full((S, nkv, max_ctx, HD), 0x11, dtype=torch.uint8, device=DEV), torch.full((S, nkv, max_ctx // 32, HD, 32), 0x11, dtype=torch.uint8, device=DEV),
            torch.full((S, nkv, max_ctx), 7.0, dtype=torch.float32, device=DEV), torch.full((S, nkv, max_ctx), 7.0, dtype=torch.float32, device=DEV))


def assert_codes_equal(got, ref, what):
    """bytes equal the torch statement's; the allowance of tests/test_gpu_fp8.py's row quantiser test, applied the same way: a product on a rounding
    boundary may land one code away, on fewer than 1e-3 of the elements"""
    diff = got != ref
    n = int(diff.sum())
    if n:
        print(f"{what}: {n} of {diff.numel()} codes differ from the torch statement")
    assert diff.float().mean().item() < 1e-3, what
    assert ((got.int() - ref.int()).abs()[diff] <= 1).all(), what


def check_pack(R, pos0, dtype, nkv=2, max_ctx=2048):
    B, S = 2, 5
    g = torch.Generator(device=DEV).manual_seed(R * 4099 + pos0)
    k = (torch.randn((B, nkv, R, HD), generator=g, device=DEV) * (torch.rand((B, nkv, R, 1), generator=g, device=DEV) * 3 + 0.01)).to(dtype)
    v = (torch.randn((B, nkv, R, HD), generator=g, device=DEV) * (torch.rand((B, nkv, R, 1), generator=g, device=DEV) * 3 + 0.01)).to(dtype)
    k[0, 0, R // 2] = 0                                              # an all-zero row: scale 1, bytes 0
    v[1, nkv - 1, 0] = 0
    slots = torch.tensor([3, 1], dtype=torch.int32, device=DEV)      # reversed, with gaps
    arr = sentinel_arrays(S, nkv, max_ctx)
    ops.kv8_pack(k, v, *arr, slots, pos0)
    torch.cuda.synchronize()
    kb, ksr = kv8.quantize_rows_ref(k.cpu())
    vb, vsr = kv8.quantize_rows_ref(v.cpu())
    exp = [a.cpu() for a in sentinel_arrays(S, nkv, max_ctx)]
    got = [a.cpu() for a in arr]
    sl = slots.cpu().long()
    name = f"R {R} pos0 {pos0} {dtype}"
    # the rows themselves
    assert torch.equal(got[2][sl, :, pos0:pos0 + R], ksr) and torch.equal(got[3][sl, :, pos0:pos0 + R], vsr), f"{name}: scales"
    assert_codes_equal(got[0][sl, :, pos0:pos0 + R], kb, f"{name}: K8")
    got_v = kv8.unblock_v(got[1])
    assert_codes_equal(got_v[sl, :, pos0:pos0 + R], vb, f"{name}: V8")
    assert float(got[2][3, 0, pos0 + R // 2]) == 1.0 and not got[0][3, 0, pos0 + R // 2].any()
    assert float(got[3][1, nkv - 1, pos0]) == 1.0 and not got_v[1, nkv - 1, pos0].any()
    # nothing outside the rows: put the device's own rows into untouched arrays
    exp[0][sl, :, pos0:pos0 + R] = got[0][sl, :, pos0:pos0 + R]
    ev = kv8.unblock_v(exp[1])
    ev[sl, :, pos0:pos0 + R] = got_v[sl, :, pos0:pos0 + R]
    exp[1] = kv8.block_v(ev)
    exp[2][sl, :, pos0:pos0 + R], exp[3][sl, :, pos0:pos0 + R] = ksr, vsr
    for a, e, what in zip(got, exp, ("K8", "V8", "ks", "vs")):
        assert torch.equal(a, e), f"{name}: {what} written outside the rows"
    # unpack: rows [0, pos0 + R) of the two slots, bit-equal to the torch statement rounded to the element type; nothing from there on
    n = pos0 + R                                                     # (rows below pos0 hold the sentinel, a finite value like any other)
    k_out = torch.full((B, nkv, max_ctx, HD), 5.0, dtype=dtype, device=DEV)
    vt_out = torch.full((B, nkv, HD, max_ctx), 5.0, dtype=dtype, device=DEV)
    ops.kv8_unpack(*arr, slots, n, k_out, vt_out)
    torch.cuda.synchronize()
    now = [a.cpu() for a in arr]
    kd, vd = kv8.unpack_cache_ref(now[0][sl], now[1][sl], now[2][sl], now[3][sl], dtype)
    k_o, v_o = k_out.cpu(), vt_out.cpu().transpose(2, 3)
    assert torch.equal(k_o[:, :, :n].view(torch.int16), kd[:, :, :n].view(torch.int16)), f"{name}: unpacked K"
    assert torch.equal(v_o[:, :, :n].contiguous().view(torch.int16), vd[:, :, :n].contiguous().view(torch.int16)), f"{name}: unpacked V^T"
    assert bool((k_o[:, :, n:] == 5.0).all()) and bool((v_o[:, :, n:] == 5.0).all()), f"{name}: unpack wrote past its rows"


@pytest.mark.parametrize("pos0", [0, 5, 32, 2015])
def test_kv8_pack_and_unpack_bit_exact(pos0):
    for R in (1, 31, 32, 33, 333):
        if pos0 + R <= 2048:
            check_pack(R, pos0, torch.bfloat16)
        else:
            arr = sentinel_arrays(3, 2, 2048)
            rows = torch.ones((1, 2, R, HD), dtype=torch.bfloat16, device=DEV)
            with pytest.raises(_lib.TraceHipError, match="trace_op_kv8_pack"):
                ops.kv8_pack(rows, rows, *arr, torch.zeros((1,), dtype=torch.int32, device=DEV), pos0)
            torch.cuda.synchronize()
            assert bool((arr[0] == 0x11).all()) and bool((arr[2] == 7.0).all())


def test_kv8_pack_and_unpack_fp16_library():
    try:
        ops.use("f16")
        check_pack(33, 5, torch.float16)
    finally:
        ops.use("bf16")


# ---- qkv_finish_kv8 ----------------------------------------------------------------------------------------------------------------------------
def check_finish(poss, ks_chunks, nsplit, max_ctx=2048, dtype=torch.bfloat16, seed=0):
    """a case of the 16-bit fused-prologue test (reversed slots with gaps, poison from pos on and in every unused slot): the kv8 append against the
    16-bit append of the same input, through the torch statement of the row rule"""
    c = T16.fused_case(poss, ks_chunks, nsplit, max_ctx, dtype, seed)
    B, pos, sl = c["B"], c["pos"].long(), c["slots"].long()
    name = f"B {B} ks {ks_chunks} nsplit {nsplit} pos {poss[:16]}"
    # the 16-bit append
    kB, vB = c["kc"].clone(), c["vt"].clone()
    q16 = ops.qkv_finish(c["part"], kB, vB, c["slots"], c["pos"], c["cos"], c["sin"], NQ)
    k_new, v_new = kB[sl, :, pos], vB[sl, :, :, pos]                                               # [B, NKV, 128] each
    # the kv8 arrays: the same cache, packed (3e4 in the unused slots quantises to bytes 0x7E)
    arr0 = kv8.pack_cache_ref(c["kc"], c["vt"].transpose(2, 3))
    arr = [a.clone() for a in arr0]
    q8 = ops.qkv_finish_kv8(c["part"], *arr, c["slots"], c["pos"], c["cos"], c["sin"], NQ)
    torch.cuda.synchronize()
    d = P.ulp_distance(q8.view(B, NQ, HD), c["q_ref"])
    assert int(d.max()) <= 1, f"q rows {name}: {int((d > 1).sum())} elements more than one ulp off the reference (max {int(d.max())})"
    assert torch.equal(q8, q16), f"{name}: q rows differ from the 16-bit qkv_finish"
    kb, ksr = kv8.quantize_rows_ref(k_new.cpu())
    vb, vsr = kv8.quantize_rows_ref(v_new.cpu())
    g_k8, g_v8, g_ks, g_vs = [a.cpu() for a in arr]
    slc, posc = sl.cpu(), pos.cpu()
    g_v = kv8.unblock_v(g_v8)
    assert torch.equal(g_ks[slc, :, posc], ksr) and torch.equal(g_vs[slc, :, posc], vsr), f"{name}: appended scales"
    assert torch.equal(g_k8[slc, :, posc], kb), f"{name}: appended K8 row: {int((g_k8[slc, :, posc] != kb).sum())} bytes differ"
    assert torch.equal(g_v[slc, :, posc], vb), f"{name}: appended V8 column: {int((g_v[slc, :, posc] != vb).sum())} bytes differ"
    # nothing but the B rows / columns / scales was written
    e_k8, e_v8, e_ks, e_vs = [a.cpu() for a in arr0]
    e_v = kv8.unblock_v(e_v8)
    e_k8[slc, :, posc], e_v[slc, :, posc], e_ks[slc, :, posc], e_vs[slc, :, posc] = kb, vb, ksr, vsr
    assert torch.equal(e_k8, g_k8) and torch.equal(kv8.block_v(e_v), g_v8) and torch.equal(e_ks, g_ks) and torch.equal(e_vs, g_vs), \
        f"{name}: the append wrote outside its row / column / scales"
    # the attention over the result (gathered into slot order for the identity-slot op): the pointer probe
    a = [x[sl].contiguous() for x in arr]
    r = K8.reference_kv8(q8.view(B, NQ, 1, HD), a[0], a[2], a[1], a[3], P.decode_visible(c["pos"], max_ctx), SCALE)
    out = ops.attn_decode_kv8(q8, *a, c["pos"], nsplit, SCALE)
    judge("pointer", out.view(B, NQ, 1, HD), r, name)
    return out


def test_qkv_finish_kv8_batch_1():
    """pos % 32 = every value (the byte column of the V8 block), ks 1 / 3 / 4 / 5 / 14, the engine's 16 splits"""
    ns = P.decode_nsplit(1)
    for r in range(32):
        check_finish([T16.BASES[r % 6] + r], T16.KS[r % 5], ns, seed=r)
    for i, p in enumerate((0, 480, 2047)):
        check_finish([p], T16.KS[i], ns, seed=100 + i)


def test_qkv_finish_kv8_batch_4():
    ns = P.decode_nsplit(4)
    for l in range(4):
        check_finish([T16.BASES[(l + b) % 6] + 4 * l + b for b in range(4)], T16.KS[l % 5], ns, seed=200 + l)
    check_finish([2047, 32 * (ns - 1), 0, 31], 14, ns, seed=300)


def test_qkv_finish_kv8_batch_128():
    ns = P.decode_nsplit(128)
    poss = [T16.BASES[(b // 32 + b) % 6] + b % 32 for b in range(128)]
    poss[127] = 2047
    check_finish(poss, 5, ns, seed=400)


def test_qkv_finish_kv8_fp16_library():
    try:
        ops.use("f16")
        check_finish([2016 + 31, 480, 33, 7], 3, P.decode_nsplit(4), dtype=torch.float16, seed=500)
    finally:
        ops.use("bf16")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_kv8_entry_points_refuse_what_their_arrays_cannot_hold():
    """a batch above trace_op_sk_rows(), a slot outside the arrays or given twice, a position outside the slot, a context that is no multiple of 32:
    TRACE_ERR_ARG, nothing launched"""
    rows = ops.sk_rows()
    B, max_ctx = rows + 1, 32
    arr = sentinel_arrays(B, NKV, max_ctx)
    pos = torch.zeros((B,), dtype=torch.int32, device=DEV)
    q = torch.zeros((B, NQ * HD), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_lib.TraceHipError, match="trace_op_attn_decode_kv8"):
        ops.attn_decode_kv8(q, *arr, pos, 1, SCALE)
    with pytest.raises(_lib.TraceHipError, match="trace_op_attn_decode_kv8"):                      # a position outside the slot
        ops.attn_decode_kv8(q[:2], *[a[:2] for a in arr], torch.tensor([0, max_ctx], dtype=torch.int32, device=DEV), 1, SCALE)
    odd = (torch.zeros((2, NKV, 48, HD), dtype=torch.uint8, device=DEV), torch.zeros((2, NKV, 1, HD, 32), dtype=torch.uint8, device=DEV),
           torch.zeros((2, NKV, 48), device=DEV), torch.zeros((2, NKV, 48), device=DEV))
    with pytest.raises(_lib.TraceHipError, match="trace_op_attn_decode_kv8"):                      # max_ctx % 32
        ops.attn_decode_kv8(q[:2], *odd, pos[:2], 1, SCALE)
    cos_t, sin_t = T16.rope_tables(max_ctx)
    part = torch.ones((1, rows, (NQ + 2 * NKV) * HD), dtype=torch.float32, device=DEV)
    slots = torch.arange(B, dtype=torch.int32, device=DEV)
    rows16 = torch.ones((B, NKV, 1, HD), dtype=torch.bfloat16, device=DEV)
    for bad_slots, bad_pos in ((slots, pos), (torch.tensor([0, 4], dtype=torch.int32, device=DEV), pos[:2]),
                               (torch.tensor([1, 1], dtype=torch.int32, device=DEV), pos[:2]),
                               (slots[:2], torch.tensor([0, max_ctx], dtype=torch.int32, device=DEV)),
                               (torch.tensor([0, -1], dtype=torch.int32, device=DEV), pos[:2])):
        a = arr if bad_slots.numel() > 2 else [x[:4] for x in arr]
        with pytest.raises(_lib.TraceHipError, match="trace_op_qkv_finish_kv8"):
            ops.qkv_finish_kv8(part, *a, bad_slots, bad_pos, cos_t, sin_t, NQ)
        if int(bad_pos.max()) < max_ctx:                             # (pack and unpack take no positions)
            n = bad_slots.numel()
            with pytest.raises(_lib.TraceHipError, match="trace_op_kv8_pack"):
                ops.kv8_pack(rows16[:n], rows16[:n], *a, bad_slots, 0)
            with pytest.raises(_lib.TraceHipError, match="trace_op_kv8_unpack"):
                ops.kv8_unpack(*a, bad_slots, 1)
    with pytest.raises(_lib.TraceHipError, match="trace_op_kv8_unpack"):                           # more rows than the slot has
        ops.kv8_unpack(*[x[:4] for x in arr], slots[:2], max_ctx + 1)
    torch.cuda.synchronize()
    assert bool((arr[0] == 0x11).all()) and bool((arr[1] == 0x11).all()) and bool((arr[2] == 7.0).all()) and bool((arr[3] == 7.0).all())
