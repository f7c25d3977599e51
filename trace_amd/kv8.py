"""The e4m3 KV cache format ("kv8") restated in torch; runs on the CPU, imports nothing of the HIP library.  include/trace_hip.h states the format:

    amax   = max |x_d|                          over the 128 values of one position of one kv head, read as fp32
    s      = amax / 448 if amax > 0 else 1      (fp32 division)  -> scale
    inv    = 448 / amax if amax > 0 else 1      (fp32 division)
    byte_d = e4m3fn(clamp(x_d * inv, -448, 448))   round to nearest even (OCP e4m3fn)
    dequantised value = s * e4m3(byte)

Arrays of one layer (B = slots, KVH = kv heads, ctx % 32 == 0):
    K8     uint8 [B, KVH, ctx, 128]
    V8     uint8 [B, KVH, ctx // 32, 128, 32]   position-blocked V^T: value d of position p is V8[b, h, p // 32, d, p % 32]
    ks, vs fp32  [B, KVH, ctx]
"""
from __future__ import annotations

import torch

FP8_MAX = 448.0
HD = 128
BLOCK = 32


def quantize_rows_ref(x):
    """x [..., n] (any float type; the amax runs over the last dimension) -> (uint8 e4m3fn bytes [..., n], fp32 scales [...])"""
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    # both are TRUE fp32 divisions of two tensors: torch evaluates `python_float / tensor` as reciprocal(tensor) * float, which is off by one unit in the
    # last place on a quarter of all values — enough to move a product across a rounding boundary (x / amax * 448 is often exactly half-way: both are 16-bit)
    top = torch.full_like(amax, FP8_MAX)
    scale = torch.where(amax > 0, amax / top, torch.ones_like(amax))
    inv = torch.where(amax > 0, top / amax, torch.ones_like(amax))
    q = (xf * inv[..., None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def e4m3_to_float(b):
    """uint8 e4m3fn bytes -> fp32 (exact)"""
    return b.contiguous().view(torch.float8_e4m3fn).float()


def dequantize_ref(b, scale, dtype=None):
    """bytes [..., n], scales [...] -> fp32 s * e4m3(byte) (one fp32 rounding), rounded to `dtype` if one is given"""
    x = e4m3_to_float(b) * scale.float()[..., None]
    return x if dtype is None else x.to(dtype)


def v8_index(p, d):
    """(block, row, column) of value d of position p in V8[b, h]"""
    return p // BLOCK, d, p % BLOCK


def block_v(v_bytes):
    """canonical bytes [B, KVH, ctx, 128] -> V8 [B, KVH, ctx // 32, 128, 32]"""
    B, KVH, ctx, hd = v_bytes.shape
    assert ctx % BLOCK == 0
    return v_bytes.view(B, KVH, ctx // BLOCK, BLOCK, hd).transpose(3, 4).contiguous()


def unblock_v(v8):
    """V8 [B, KVH, ctx // 32, 128, 32] -> canonical bytes [B, KVH, ctx, 128]"""
    B, KVH, nb, hd, blk = v8.shape
    return v8.transpose(3, 4).reshape(B, KVH, nb * blk, hd).contiguous()


def pack_cache_ref(k, v):
    """canonical k (roped) / v [B, KVH, ctx, 128] in the element type -> (K8, V8, ks, vs)"""
    k8, ks = quantize_rows_ref(k)
    vb, vs = quantize_rows_ref(v)
    return k8.contiguous(), block_v(vb), ks.contiguous(), vs.contiguous()


def unpack_cache_ref(k8, v8, ks, vs, dtype=None):
    """the four arrays -> canonical (k, v) [B, KVH, ctx, 128]: fp32 s * e4m3, rounded to `dtype` if one is given"""
    return dequantize_ref(k8, ks, dtype), dequantize_ref(unblock_v(v8), vs, dtype)


def cache_bytes_per_position(kv_heads: int, fp8: bool) -> int:
    """bytes one position of one layer takes: 2 x 128 16-bit values per kv head, or 2 x 128 bytes + two fp32 scales"""
    return kv_heads * (2 * HD + 8 if fp8 else 4 * HD)
