"""Attention probes over an e4m3 KV cache (trace_amd/kv8.py states the format): the probes, judges and bounds are those of tests/attn_probes.py,
unchanged; what is new is the reference — the float64 attention of the 16-bit q over the DEQUANTISED cache (float64(scale) x e4m3(byte)), so the
quantisation itself is no part of the error judged — and a float32 restatement of exactly the arithmetic the kv8 decode attention documents:

    score_j = (acc_j * scale) * ks[j]          acc = fp32 sum of q . e4m3(K8[j])
    p_j     = exp(score_j - m);  l += p_j      (l sums the UNSCALED p)
    P_j     = round16(p_j * vs[j])
    o       = round16((sum_j P_j . e4m3(V8[j])) / l)

Runs on the CPU as well as on a device; nothing here imports the HIP library."""
import torch

import attn_probes as P
from trace_amd import kv8

POISON_BYTE = 0x7E                # +448, the largest finite e4m3fn value


def reference_kv8(q, k8, ks, v8, vs, visible, scale):
    """q [B, H, nq, 128] 16-bit; k8 [B, KVH, ctx, 128] uint8, v8 [B, KVH, ctx/32, 128, 32] uint8, ks / vs [B, KVH, ctx] fp32; visible bool
    [B, nq, ctx] -> attn_probes.Ref: ref / A float64 over the dequantised cache, E = the largest error of the float32 restatement above."""
    B, H, nq, hd = q.shape
    KVH, nkv = k8.shape[1], k8.shape[2]
    G = H // KVH
    dtype = q.dtype
    ref = torch.empty((B, H, nq, hd), dtype=torch.float64, device=q.device)
    A = torch.empty_like(ref)
    kd_all = torch.empty((B, KVH, nkv, hd), dtype=torch.float32, device=q.device)       # only Ref.weights (failure messages) reads it
    E = 0.0
    step = max(1, min(B, (1 << 26) // max(1, H * nq * nkv)))
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        nb = sl.stop - sl.start
        vis = visible[sl][:, None, None]                                                                 # [b, 1, 1, nq, nkv]
        kq, vq = kv8.e4m3_to_float(k8[sl]), kv8.e4m3_to_float(kv8.unblock_v(v8[sl]))                      # fp32, exact
        k64 = kq.double() * ks[sl].double()[..., None]
        v64 = vq.double() * vs[sl].double()[..., None]
        kd_all[sl] = k64.float()
        q64 = q[sl].double().view(nb, KVH, G, nq, hd)
        s = torch.einsum("bkgqd,bkjd->bkgqj", q64, k64) * scale
        w = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
        r = torch.einsum("bkgqj,bkjd->bkgqd", w, v64)
        ref[sl] = r.view(nb, H, nq, hd)
        A[sl] = torch.einsum("bkgqj,bkjd->bkgqd", w, v64.abs()).view(nb, H, nq, hd)
        del s, w, k64, v64
        # the float32 restatement
        qf = q[sl].float().view(nb, KVH, G, nq, hd)
        s32 = (torch.einsum("bkgqd,bkjd->bkgqj", qf, kq) * scale) * ks[sl].float()[:, :, None, None, :]
        s32 = s32.masked_fill(~vis, float("-inf"))
        m = s32.amax(-1, keepdim=True)
        p = torch.exp(s32 - m)
        l = p.sum(-1, keepdim=True)
        pv = torch.where(vis, p * vs[sl].float()[:, :, None, None, :], torch.zeros((), device=q.device)).to(dtype).float()
        o = (torch.einsum("bkgqj,bkjd->bkgqd", pv, vq) / l).to(dtype).float()
        E = max(E, float((o.double() - r).abs().max()))
    return P.Ref(ref, A, E, q, kd_all, visible, scale)


def quantise_probe(q, k, v, pos):
    """poisons the canonical 16-bit probe (q, k, v) past pos in place, the way the 16-bit tests do, and packs it: a poisoned position then holds the
    quantised 4 q as its K row and bytes 0x7E with the scale that dequantises them to attn_probes.POISON_V as its V row -> (k8, v8, ks, vs)"""
    P.poison_decode(q, k, v, pos)
    return kv8.pack_cache_ref(k, v)


def poison_slot(KVH, nkv, device="cpu"):
    """one more slot behind the batch: every byte 0x7E, every scale 3e4 / 448 (each value dequantises to attn_probes.POISON_OTHER_SLOT)"""
    k8 = torch.full((1, KVH, nkv, kv8.HD), POISON_BYTE, dtype=torch.uint8, device=device)
    v8 = torch.full((1, KVH, nkv // kv8.BLOCK, kv8.HD, kv8.BLOCK), POISON_BYTE, dtype=torch.uint8, device=device)
    s = torch.full((1, KVH, nkv), P.POISON_OTHER_SLOT / kv8.FP8_MAX, dtype=torch.float32, device=device)
    return k8, v8, s, s.clone()


def with_poison_slot(k8, v8, ks, vs):
    pk, pv, pks, pvs = poison_slot(k8.shape[1], k8.shape[2], k8.device)
    return torch.cat([k8, pk]), torch.cat([v8, pv]), torch.cat([ks, pks]), torch.cat([vs, pvs])
