"""The e4m3 KV cache format and its probes on the CPU (trace_amd/kv8.py, tests/kv8_probes.py; no GPU): the row rule's error bound and edge rows, the
blocked V8 index map written out, the exact widening of every finite e4m3 byte to bf16 and fp16, and — in the style of tests/test_attn_probes_cpu.py —
the evidence that the judge with reference_kv8 rejects kernels that mishandle a scale, a key or the V8 layout.  Both libraries build and export the
kv8 entry points."""
import functools
import math

import pytest
import torch

import attn_probes as P
import kv8_probes as K8
from trace_amd import kv8


# ---- the row rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_quantize_rows_round_trip_bound(dtype):
    """|x - deq| <= 2^-4 |x| + amax 2^-9 / 448: half a step of a 3-bit mantissa on a normal value, half a subnormal step (2^-9 of the byte range's unit)
    below the smallest normal"""
    g = torch.Generator().manual_seed(0)
    x = (torch.randn((64, 7, 128), generator=g) * torch.rand((64, 7, 1), generator=g) * 5).to(dtype)
    x[3] *= 1e-3
    x[5, 2, ::2] *= 1e-4                                             # values far below the row's amax: e4m3's subnormal range
    b, s = kv8.quantize_rows_ref(x)
    assert b.dtype == torch.uint8 and s.dtype == torch.float32 and b.shape == x.shape and s.shape == x.shape[:-1]
    xf = x.float()
    amax = xf.abs().amax(-1, keepdim=True)
    err = (xf - kv8.dequantize_ref(b, s)).abs()
    assert bool((err <= 2.0 ** -4 * xf.abs() + amax * 2.0 ** -9 / 448 * (1 + 2.0 ** -20)).all())
    assert torch.equal(s, (amax[..., 0] / 448.0))
    assert not ((b & 0x7F) == 0x7F).any()                            # never NaN
    assert int((b & 0x7F).max()) == 0x7E                             # the row's amax lands on 448


def test_all_zero_and_single_nonzero_rows():
    x = torch.zeros((3, 128), dtype=torch.bfloat16)
    x[1, 17] = -0.37
    x[2, 127] = 3e4
    b, s = kv8.quantize_rows_ref(x)
    assert not b[0].any() and float(s[0]) == 1.0
    assert int(b[1, 17]) == 0xFE and int(b[1].int().sum()) == 0xFE and float(s[1]) == float(x[1, 17].float().abs() / 448.0)
    assert int(b[2, 127]) == 0x7E and int(b[2].int().sum()) == 0x7E
    d = kv8.dequantize_ref(b, s, torch.bfloat16)
    assert torch.equal(d, x)                                         # 448 s is amax again to within fp32 round-off, far inside a bf16 ulp


def test_pack_unpack_is_the_identity_on_bytes_and_the_index_map():
    g = torch.Generator().manual_seed(1)
    B, KVH, ctx = 2, 3, 96
    k = torch.randn((B, KVH, ctx, 128), generator=g).bfloat16()
    v = torch.randn((B, KVH, ctx, 128), generator=g).bfloat16()
    k8, v8, ks, vs = kv8.pack_cache_ref(k, v)
    assert k8.shape == (B, KVH, ctx, 128) and v8.shape == (B, KVH, ctx // 32, 128, 32) and ks.shape == vs.shape == (B, KVH, ctx)
    vb, sv = kv8.quantize_rows_ref(v)
    assert torch.equal(kv8.unblock_v(v8), vb) and torch.equal(kv8.block_v(kv8.unblock_v(v8)), v8) and torch.equal(vs, sv)
    kd, vd = kv8.unpack_cache_ref(k8, v8, ks, vs, torch.bfloat16)
    k8b, v8b, ksb, vsb = kv8.pack_cache_ref(kd, vd)                  # dequantise, quantise again: the same bytes
    assert torch.equal(k8b, k8) and torch.equal(v8b, v8)
    # the blocked map, written out: value d of position p is byte p // 32 * 4096 + d * 32 + p % 32 of the (slot, kv head)'s V8
    flat = v8.reshape(B, KVH, -1)
    for p, blk, col in ((0, 0, 0), (31, 0, 31), (32, 1, 0), (33, 1, 1), (ctx - 1, 2, 31)):
        assert kv8.v8_index(p, 5) == (blk, 5, col)
        for d in (0, 5, 127):
            assert torch.equal(flat[:, :, blk * 4096 + d * 32 + col], vb[:, :, p, d])
            assert torch.equal(v8[:, :, blk, d, col], vb[:, :, p, d])


def test_every_finite_e4m3_byte_widens_exactly_to_bf16_and_fp16():
    b = torch.arange(256, dtype=torch.uint8)
    finite = (b & 0x7F) != 0x7F
    assert int(finite.sum()) == 254
    f = kv8.e4m3_to_float(b)[finite]
    assert bool(torch.isfinite(f).all()) and float(f.abs().max()) == 448.0
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(f.to(dt).float(), f), dt


def test_cache_bytes_per_position():
    assert kv8.cache_bytes_per_position(1, True) == 264 and kv8.cache_bytes_per_position(1, False) == 512
    assert kv8.cache_bytes_per_position(8, True) == 8 * 264


# ---- the judge with reference_kv8 rejects wrong kernels -----------------------------------------------------------------------------------
FAULTS = ["ignore_ks", "ignore_vs", "ks_of_next", "vs_of_next", "drop_newest", "count_one_poisoned", "v8_unblocked"]


def emulate_kv8(q, k8, ks, v8, vs, visible, scale, nsplit, fault=None):
    """a torch stand-in for the kv8 decode attention: 32-position tiles, the context split into chunks of whole tiles, online softmax with the two
    scales where the format puts them, partials merged with exp(m_s - M) — and a fault switch"""
    B, H, nq, hd = q.shape
    KVH, nkv = k8.shape[1], k8.shape[2]
    G = H // KVH
    dtype = q.dtype
    rnd = lambda x: x.to(dtype).float()
    vis = visible.clone()
    n = visible.sum(-1)                                               # [B, nq]
    j = torch.arange(nkv)[None, None, :]
    if fault == "drop_newest":
        vis &= ~((j == (n - 1)[..., None]) & (n > 1)[..., None])
    if fault == "count_one_poisoned":
        vis |= (j == n[..., None]) & (n < nkv)[..., None]
        assert not torch.equal(vis, visible)
    kq = kv8.e4m3_to_float(k8)
    if fault == "v8_unblocked":                                       # the V8 bytes of a (slot, kv head) read as V^T [128][ctx]
        vq = kv8.e4m3_to_float(v8.reshape(B, KVH, hd, nkv).transpose(2, 3).contiguous())
    else:
        vq = kv8.e4m3_to_float(kv8.unblock_v(v8))
    ksf, vsf = ks.float(), vs.float()
    if fault == "ignore_ks":
        ksf = torch.ones_like(ksf)
    if fault == "ignore_vs":
        vsf = torch.ones_like(vsf)
    if fault == "ks_of_next":
        ksf = torch.cat([ksf[..., 1:], ksf[..., -1:]], -1)
    if fault == "vs_of_next":
        vsf = torch.cat([vsf[..., 1:], vsf[..., -1:]], -1)
    kvmap = torch.arange(H) // G
    s = (torch.einsum("bhqd,bhjd->bhqj", q.float(), kq[:, kvmap]) * scale) * ksf[:, kvmap][:, :, None, :]
    vh, vsh = vq[:, kvmap], vsf[:, kvmap][:, :, None, :]
    chunk = ((-(-n // nsplit)) + 31) // 32 * 32
    split_id = j // chunk[..., None]
    ms, ls, accs = [], [], []
    for sp in range(nsplit):
        m = torch.full((B, H, nq, 1), -1e30)
        l = torch.zeros((B, H, nq, 1))
        acc = torch.zeros((B, H, nq, hd))
        for t0 in range(0, nkv, 32):
            mk = (vis[..., t0:t0 + 32] & (split_id[..., t0:t0 + 32] == sp))[:, None]
            if not mk.any():
                continue
            st = torch.where(mk, s[..., t0:t0 + 32], torch.full((), -1e30))
            mn = torch.maximum(m, st.amax(-1, keepdim=True))
            a = torch.exp(m - mn)
            p = torch.where(mk, torch.exp(st - mn), torch.zeros(()))
            l = l * a + p.sum(-1, keepdim=True)
            acc = acc * a + torch.einsum("bhqj,bhjd->bhqd", rnd(p * vsh[..., t0:t0 + 32]), vh[:, :, t0:t0 + 32])
            m = mn
        ms.append(m); ls.append(l); accs.append(acc)
    M = torch.stack(ms).amax(0)
    num = torch.zeros((B, H, nq, hd))
    den = torch.zeros((B, H, nq, 1))
    for sp in range(nsplit):
        f = torch.exp(ms[sp] - M)
        num += f * accs[sp]
        den += f * ls[sp]
    return (num / den).to(dtype)


def kv8_decode_set(ctxs, max_ctx, nsplit, H=32, KVH=8, hd=128, dtype=torch.bfloat16):
    """the four decode probes as tests/test_gpu_kv8_probes.py builds them: poisoned past pos, then packed"""
    B = len(ctxs)
    scale = 1 / math.sqrt(hd)
    pos = torch.tensor([c - 1 for c in ctxs])
    nvis = pos + 1
    vis = P.decode_visible(pos, max_ctx)
    raw = {"uniform": P.probe_uniform(B, H, KVH, 1, max_ctx, hd, dtype, seed=1),
           "pointer": P.probe_pointer(P.decode_pointer_target_tensor(ctxs, H, nsplit), H, KVH, max_ctx, hd, dtype, seed=2),
           "ramp_up": P.probe_ramp(nvis, B, H, KVH, 1, max_ctx, hd, scale, dtype, True, seed=3),
           "ramp_down": P.probe_ramp(nvis, B, H, KVH, 1, max_ctx, hd, scale, dtype, False, seed=4)}
    out = {pn: (q,) + K8.quantise_probe(q, k, v, pos) for pn, (q, k, v) in raw.items()}
    return out, vis, scale


CASES = {
    "decode-small": (lambda: kv8_decode_set([33, 70], 128, 2), 2),
    "decode-real": (lambda: kv8_decode_set([2047, 1999, 200], 2048, 16), 16),
    "decode-small-f16": (lambda: kv8_decode_set([31, 65], 128, 2, dtype=torch.float16), 2),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    build, nsplit = CASES[name]
    probes, vis, scale = build()
    refs = {pn: K8.reference_kv8(q, k8, ks, v8, vs, vis, scale) for pn, (q, k8, v8, ks, vs) in probes.items()}
    return probes, refs, vis, scale, nsplit


def _verdicts(name, fault):
    probes, refs, vis, scale, nsplit = _case(name)
    out = {}
    for pn, (q, k8, v8, ks, vs) in probes.items():
        got = emulate_kv8(q, k8, ks, v8, vs, vis, scale, nsplit, fault)
        out[pn] = (P.uniform_close if pn == "uniform" else P.attention_close)(got, refs[pn], f"{name} {pn}")
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_fault_free_kv8_emulation_is_accepted(name):
    for pn, (ok, msg) in _verdicts(name, None).items():
        assert ok, msg


@pytest.mark.parametrize("name,fault", [(n, f) for n in CASES for f in FAULTS])
def test_every_kv8_fault_is_rejected_by_a_probe(name, fault):
    v = _verdicts(name, fault)
    rejected = [pn for pn, (ok, _) in v.items() if not ok]
    print(f"{name} / {fault}: rejected by {rejected}")
    assert rejected, f"{fault} passes every probe of {name}"


def test_poison_is_finite_and_large():
    probes, _, vis, _, _ = _case("decode-small")
    q, k8, v8, ks, vs = probes["pointer"]
    past = ~vis[:, 0]                                                 # [B, ctx]
    vb = kv8.unblock_v(v8)
    assert bool((vb[:, 0][past] == K8.POISON_BYTE).all())
    assert torch.allclose(kv8.dequantize_ref(vb, vs)[:, 0][past], torch.tensor(P.POISON_V).bfloat16().float())
    assert not ((k8 & 0x7F) == 0x7F).any() and bool(torch.isfinite(ks).all()) and bool(torch.isfinite(vs).all())
    pk, pv, pks, pvs = K8.poison_slot(8, 128)
    assert float(kv8.dequantize_ref(pk, pks).min()) == pytest.approx(P.POISON_OTHER_SLOT, rel=1e-6)


# ---- the libraries ------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("trace_op_attn_decode_kv8", "trace_op_qkv_finish_kv8", "trace_op_kv8_pack", "trace_op_kv8_unpack", "trace_ctx_create_opts",
               "trace_ctx_kv_cache_type", "trace_debug_kv8_buffers")


def test_both_libraries_build_and_export_the_kv8_entry_points():
    from trace_amd import build, _lib
    build.build()
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        for name in NEW_SYMBOLS:
            assert name in _lib.SIGNATURES and hasattr(lib, name), (element, name)
    from trace_amd.engine import ops
    for name in ("attn_decode_kv8", "qkv_finish_kv8", "kv8_pack", "kv8_unpack"):
        assert callable(getattr(ops, name))


def test_create_opts_refuses_a_bad_combination_before_any_device_call():
    """trace_ctx_create_opts checks its options first: fp8 weights with an fp8 cache, a flag outside {0, 1} and a short struct are TRACE_ERR_ARG on a
    machine with no device at all (a valid call would go on to hipSetDevice)"""
    import ctypes as C
    from trace_amd import build, _lib, config as tcfg
    build.build()
    cfg = tcfg.tiny()
    for element in ("bf16", "f16"):
        lib = _lib.load(element)
        c = _lib.TraceConfigC()
        c.llm_weights_fp8 = 1
        h = C.c_void_p()
        o = _lib.TraceCtxOptsC(C.sizeof(_lib.TraceCtxOptsC), 1)
        with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: kv_cache_fp8 with llm_weights_fp8"):
            lib.trace_ctx_create_opts(C.byref(c), 0, C.byref(o), C.byref(h))
        c.llm_weights_fp8 = 0
        with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: kv_cache_fp8 must be 0 or 1"):
            lib.trace_ctx_create_opts(C.byref(c), 0, C.byref(_lib.TraceCtxOptsC(C.sizeof(_lib.TraceCtxOptsC), 2)), C.byref(h))
        with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: trace_ctx_opts::size"):
            lib.trace_ctx_create_opts(C.byref(c), 0, C.byref(_lib.TraceCtxOptsC(4, 1)), C.byref(h))
        with pytest.raises(_lib.TraceHipError, match=r"error -1 in trace_ctx_create_opts: null argument"):
            lib.trace_ctx_create_opts(None, 0, C.byref(o), C.byref(h))
        assert not h.value
    assert C.sizeof(_lib.TraceCtxOptsC) == 8


def test_engine_rejects_unknown_kv_cache_before_any_device_work():
    from trace_amd import config as tcfg
    from trace_amd.engine import TraceEngine
    for bad in ("int8", "fp16", True, 1):
        with pytest.raises(ValueError, match="kv_cache must be None or 'fp8'"):
            TraceEngine(tcfg.tiny(), kv_cache=bad)
    with pytest.raises(ValueError, match="kv_cache='fp8' with llm_fp8"):
        TraceEngine(tcfg.tiny(), kv_cache="fp8", llm_fp8="weight_only")
