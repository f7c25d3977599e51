"""The attention probes must reject wrong kernels (tests/attn_probes.py; no GPU).

A torch "kernel" stands in for the HIP ones: online softmax over key tiles, the keys of a row split into chunks of whole tiles the way the decode
attention splits a context, partials merged with exp(m_s - M), P rounded to the element type before PV, fp32 sums, the output rounded — and a fault
switch.  For every probe set tests/test_gpu_attention_probes.py uses and every fault below, at one small and one real shape per kernel family: the
fault-free emulation is accepted and each fault is rejected by at least one probe of the set, under the very judge and bounds the GPU tests use.
This is the evidence that those bounds are not too loose; loosening them later shows up here."""
import functools
import math

import pytest
import torch

import attn_probes as P

FAULTS = ["last_key", "first_key", "tail_key", "one_past", "narrow", "block32", "merge_no_rescale", "l_no_rescale", "swap_v", "wrong_kv_head",
          "wrong_slot"]


def _mask_fault(visible, fault):
    """faults that only change which keys count.  Every mask here is a prefix of the keys per row."""
    vis = visible.clone()
    nkv = vis.shape[-1]
    j = torch.arange(nkv)[None, None, :]
    n = vis.sum(-1, keepdim=True)                                     # [B, nq, 1]
    last = n - 1
    if fault == "last_key":                                           # the newest key of the sequence
        vis &= ~((j == last.amax(1, keepdim=True)) & (n > 1))
    elif fault == "first_key":
        vis &= ~((j == 0) & (n > 1))
    elif fault == "tail_key":                                         # the first key after the last whole 64-key tile
        vis &= ~((j == 64 * (n // 64)) & (n % 64 != 0) & (n > 64))
    elif fault == "one_past":                                         # decode pos + 1, causal i + 1
        vis |= j == last + 1
    elif fault == "narrow":                                           # every row loses its own newest key
        vis &= ~((j == last) & (n > 1))
    elif fault == "block32":                                          # the middle 32-position block of what a row sees
        blk = (n // 32) // 2
        vis &= ~((j >= 32 * blk) & (j < 32 * blk + 32) & (n >= 64))
    else:
        return vis, False
    assert not torch.equal(vis, visible), f"{fault} changes nothing at this shape"
    return vis, True


def emulate(q, k, v, visible, scale, nsplit, tile, fold, fault=None):
    B, H, nq, hd = q.shape
    KVH, nkv = k.shape[1], k.shape[2]
    G = H // KVH
    dtype = q.dtype
    rnd = lambda x: x.to(dtype).float()
    vis, _ = _mask_fault(visible, fault)
    kvmap = torch.arange(H) // G
    if fault == "wrong_kv_head":
        assert KVH > 1
        kvmap = (kvmap + 1) % KVH
    kf, vf = k.float(), v.float()
    if fault == "wrong_slot":
        assert B > 1
        kf, vf = kf.roll(-1, 0), vf.roll(-1, 0)
    if fault == "swap_v":                                             # the first two rows of the 32-position block that holds the key before the newest
        vf = vf.clone()
        for b in range(B):
            ctx = int(visible[b].sum(-1).max())
            assert ctx >= 2
            j0 = 32 * ((ctx - 2) // 32)
            vf[b, :, [j0, j0 + 1]] = vf[b, :, [j0 + 1, j0]]
    kh, vh = kf[:, kvmap], vf[:, kvmap]                               # [B, H, nkv, hd]
    if fold:
        s = torch.einsum("bhqd,bhjd->bhqj", rnd(q.float() * (scale * 1.4426950408889634)), kh)
        ex = torch.exp2
    else:
        s = torch.einsum("bhqd,bhjd->bhqj", q.float(), kh) * scale
        ex = torch.exp
    n = visible.sum(-1)                                               # [B, nq]: the split geometry follows the true context
    chunk = ((-(-n // nsplit)) + tile - 1) // tile * tile
    split_id = torch.arange(nkv)[None, None, :] // chunk[..., None]   # [B, nq, nkv]
    ms, ls, accs = [], [], []
    for sp in range(nsplit):
        m = torch.full((B, H, nq, 1), -1e30)
        l = torch.zeros((B, H, nq, 1))
        acc = torch.zeros((B, H, nq, hd))
        for t0 in range(0, nkv, tile):
            mk = (vis[..., t0:t0 + tile] & (split_id[..., t0:t0 + tile] == sp))[:, None]          # [B, 1, nq, tile]
            if not mk.any():
                continue
            st = torch.where(mk, s[..., t0:t0 + tile], torch.full((), -1e30))
            mn = torch.maximum(m, st.amax(-1, keepdim=True))
            a = ex(m - mn)
            p = torch.where(mk, ex(st - mn), torch.zeros(()))
            l = (l if fault == "l_no_rescale" else l * a) + p.sum(-1, keepdim=True)
            acc = acc * a + torch.einsum("bhqj,bhjd->bhqd", rnd(p), vh[:, :, t0:t0 + tile])
            m = mn
        ms.append(m); ls.append(l); accs.append(acc)
    M = torch.stack(ms).amax(0)
    num = torch.zeros((B, H, nq, hd))
    den = torch.zeros((B, H, nq, 1))
    for sp in range(nsplit):
        f = ex(ms[sp] - M)
        if fault == "merge_no_rescale" and sp == 0:
            f = torch.ones_like(f)
        num += f * accs[sp]
        den += f * ls[sp]
    return (num / den).to(dtype)


# ---- the probe sets, as the GPU tests build them ----------------------------------------------------------------------------------------
def decode_set(ctxs, max_ctx, nsplit, H=32, KVH=8, hd=128, dtype=torch.bfloat16):
    B = len(ctxs)
    scale = 1 / math.sqrt(hd)
    pos = torch.tensor([c - 1 for c in ctxs])
    nvis = pos + 1
    vis = P.decode_visible(pos, max_ctx)
    out = {}
    out["uniform"] = P.probe_uniform(B, H, KVH, 1, max_ctx, hd, dtype, seed=1)
    out["pointer"] = P.probe_pointer(P.decode_pointer_target_tensor(ctxs, H, nsplit), H, KVH, max_ctx, hd, dtype, seed=2)
    out["ramp_up"] = P.probe_ramp(nvis, B, H, KVH, 1, max_ctx, hd, scale, dtype, True, seed=3)
    out["ramp_down"] = P.probe_ramp(nvis, B, H, KVH, 1, max_ctx, hd, scale, dtype, False, seed=4)
    for q, k, v in out.values():
        P.poison_decode(q, k, v, pos)
    return out, vis, scale, False


def causal_set(B, nq, nkv, KVH, hd=128, dtype=torch.bfloat16):
    H = 4 * KVH
    scale = 1 / math.sqrt(hd)
    vis = P.causal_visible(B, nq, nkv)
    nvis = torch.full((B,), nkv)
    out = {"uniform": P.probe_uniform(B, H, KVH, nq, nkv, hd, dtype, seed=1),
           "pointer": P.probe_pointer(P.causal_pointer_targets(B, H, nq, nkv), H, KVH, nkv, hd, dtype, seed=2),
           "ramp_up": P.probe_ramp(nvis, B, H, KVH, nq, nkv, hd, scale, dtype, True, seed=3),
           "ramp_down": P.probe_ramp(nvis, B, H, KVH, nq, nkv, hd, scale, dtype, False, seed=4)}
    return out, vis, scale, True


def vit_set(B, n, H, hd=64, dtype=torch.bfloat16):
    scale = 1 / math.sqrt(hd)
    vis = P.full_visible(B, n, n)
    nvis = torch.full((B,), n)
    out = {"uniform": P.probe_uniform(B, H, H, n, n, hd, dtype, seed=1),
           "pointer": P.probe_pointer(P.vit_pointer_targets(B, H, n, seed=5), H, H, n, hd, dtype, seed=2),
           "ramp_up": P.probe_ramp(nvis, B, H, H, n, n, hd, scale, dtype, True, seed=3),
           "ramp_down": P.probe_ramp(nvis, B, H, H, n, n, hd, scale, dtype, False, seed=4)}
    return out, vis, scale, True


# name -> (builder, emulation's split count, key tile, faults that do not exist for the family)
CASES = {
    "decode-small": (lambda: decode_set([33, 70], 128, 2), 2, 32, ()),
    "decode-real": (lambda: decode_set([2047, 2048, 200], 2048, 16), 16, 32, ()),
    "decode-real-f16": (lambda: decode_set([2048, 481], 2048, 16, dtype=torch.float16), 16, 32, ()),
    "causal-small": (lambda: causal_set(2, 150, 150, 2), 2, 64, ()),
    "causal-append-real": (lambda: causal_set(2, 40, 333, 2), 4, 64, ()),
    "vit-small": (lambda: vit_set(2, 150, 2), 2, 64, ("one_past", "narrow")),          # no key past the end of a full attention, no diagonal
    "vit-real": (lambda: vit_set(2, 577, 4), 4, 64, ("one_past", "narrow")),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    build, nsplit, tile, na = CASES[name]
    probes, vis, scale, fold = build()
    refs = {pn: P.reference(q, k, v, vis, scale, fold) for pn, (q, k, v) in probes.items()}
    return probes, refs, vis, scale, fold, nsplit, tile


def _verdicts(name, fault):
    probes, refs, vis, scale, fold, nsplit, tile = _case(name)
    out = {}
    for pn, (q, k, v) in probes.items():
        got = emulate(q, k, v, vis, scale, nsplit, tile, fold, fault)
        out[pn] = (P.uniform_close if pn == "uniform" else P.attention_close)(got, refs[pn], f"{name} {pn}")
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_fault_free_emulation_is_accepted(name):
    for pn, (ok, msg) in _verdicts(name, None).items():
        assert ok, msg


@pytest.mark.parametrize("name,fault", [(n, f) for n in CASES for f in FAULTS if f not in CASES[n][3]])
def test_every_fault_is_rejected_by_a_probe(name, fault):
    v = _verdicts(name, fault)
    rejected = [pn for pn, (ok, _) in v.items() if not ok]
    print(f"{name} / {fault}: rejected by {rejected}")
    assert rejected, f"{fault} passes every probe of {name}"


def test_gaussian_check_of_the_kernel_tests_misses_a_lost_key():
    """What the probes are for: on Gaussian data at ctx 2047 the tolerance of tests/test_gpu_kernels.py (2e-2 + 2e-2 |ref|) accepts a decode
    attention that ignores the newest key on every element (a key weighs ~1 / 2047 there, ten times less than the tolerance); the probe set does
    not (the test above)."""
    g = torch.Generator().manual_seed(0)
    H, KVH, hd, ctx = 32, 8, 128, 2047
    q = torch.randn((1, H, 1, hd), generator=g).bfloat16()
    k, v = torch.randn((1, KVH, 2048, hd), generator=g).bfloat16(), torch.randn((1, KVH, 2048, hd), generator=g).bfloat16()
    vis = P.decode_visible(torch.tensor([ctx - 1]), 2048)
    r = P.reference(q, k, v, vis, 1 / math.sqrt(hd), False)
    got = emulate(q, k, v, vis, 1 / math.sqrt(hd), 16, 32, False, "last_key").double()
    flagged = (got - r.ref).abs() > 2e-2 + 2e-2 * r.ref.abs()
    print(f"Gaussian check, newest key ignored at ctx {ctx}: {int(flagged.sum())} of {flagged.numel()} elements flagged")
    assert int(flagged.sum()) == 0


def test_decode_geometry_helpers():
    assert [P.decode_nsplit(b) for b in (1, 2, 3, 8, 32, 128)] == [16, 16, 13, 5, 1, 1]
    assert P.decode_chunk(481, 16) == 32 and P.decode_chunk(513, 16) == 64 and P.decode_chunk(2048, 16) == 128
    for ns in (1, 5, 13, 16, 32):
        for ctx in P.decode_contexts(ns, 2048):
            t = P.decode_pointer_targets(ctx, ns)
            assert all(0 <= x < ctx for x in t) and ctx - 1 in t and 0 in t
    ctx = 32 * 15 + 1                                   # 16 splits: the last one holds exactly one key
    assert ctx in P.decode_contexts(16, 2048) and ctx - P.decode_chunk(ctx, 16) * ((ctx - 1) // P.decode_chunk(ctx, 16)) == 1


def test_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 3.0]).bfloat16()
    b = torch.tensor([1.0078125, -1.0078125, -0.0, 3.0]).bfloat16()
    assert P.ulp_distance(a, b).tolist() == [1, 1, 0, 0]
