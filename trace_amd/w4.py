"""The 4-bit decoder weight format ("w4") restated in torch; runs on the CPU, imports nothing of the HIP library.  include/trace_hip.h states the format:

    block    32 consecutive k of one output row of W [N, K] (bf16)
    element  OCP e2m1: magnitudes {0, 0.5, 1, 1.5, 2, 3, 4, 6} = codes 0..7, bit 3 = sign
    scale    2^e, one e8m0 byte per block: byte = e + 127
    e        the smallest integer with amax / 2^e <= 6, kept >= -120; an all-zero block: every code 0 and byte 0 (e = -127)
    code     round to nearest, ties to the even code, of |v| / 2^e; the sign bit only beside a non-zero magnitude
    W~[n, k] = e2m1(code) * 2^e, exactly a bf16 value

Logical arrays:
    codes uint8 [N, K / 2]    k = 2 j in the low nibble of byte j, k = 2 j + 1 in the high nibble
    exps  uint8 [N, K / 32]
Decode tile layout (N % 16 == 0, K % 256 == 0; U = K / 256):
    tcodes uint8 [N / 16, U, 64, 32]   lane = g * 16 + r holds row tile * 16 + r, k = unit * 256 + g * 64 .. + 64, in logical byte order
    texps  uint8 [N / 16, U, 64, 2]    the exponent bytes of the lane's two blocks
Everything here is integer arithmetic on the bf16 bits or exact float arithmetic, so a device kernel can be held to it bit for bit; the functions
run on whatever device their tensors are on.
"""
from __future__ import annotations

import torch

BLOCK = 32
UNIT = 256
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E_MIN = -120


def _bits(W):
    """bf16 tensor -> int32 bit patterns"""
    return W.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def _pow2(e):
    """2^e as float64 for an integer tensor e (|e| < 1023), built from the bits: exact on every device"""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def exp_bytes(W):
    """W bf16 [N, K] -> int32 exponent bytes [N, K / 32] (0 for an all-zero block)"""
    N, K = W.shape
    mag = (_bits(W) & 0x7FFF).view(N, K // BLOCK, BLOCK).amax(dim=-1)      # positive floats order as their bits
    e = (mag >> 7) - 127 - 2 + ((mag & 0x7F) > 0x40).to(torch.int32)
    e = torch.clamp(e, min=E_MIN) + 127
    return torch.where(mag == 0, torch.zeros_like(e), e)


def quant(W):
    """W bf16 [N, K] (K % 32 == 0) -> (codes uint8 [N, K / 2], exps uint8 [N, K / 32]) in the logical order"""
    assert W.dtype == torch.bfloat16 and W.dim() == 2 and W.shape[1] % BLOCK == 0
    N, K = W.shape
    eb = exp_bytes(W)                                                       # [N, K/32]
    bits = _bits(W)
    # |v| / 2^e in float64: exact (a power-of-two quotient of a bf16 value, no underflow at this width)
    a = W.float().abs().double().view(N, K // BLOCK, BLOCK) * _pow2(127 - eb)[..., None]
    m = torch.zeros_like(a, dtype=torch.int32)
    # thresholds in ascending order: 0.25] 0.75) 1.25] 1.75) 2.5] 3.5) 5]
    m += (a > 0.25).to(torch.int32) + (a >= 0.75).to(torch.int32) + (a > 1.25).to(torch.int32) + (a >= 1.75).to(torch.int32)
    m += (a > 2.5).to(torch.int32) + (a >= 3.5).to(torch.int32) + (a > 5.0).to(torch.int32)
    m = torch.where(eb[..., None] == 0, torch.zeros_like(m), m).view(N, K)
    sign = (bits >> 12) & 8
    c = torch.where(m > 0, m | sign, m)
    codes = (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)
    return codes.contiguous(), eb.to(torch.uint8).contiguous()


def unpack_codes(codes):
    """codes uint8 [N, K / 2] -> int32 [N, K] of 4-bit codes in k order"""
    c = codes.to(torch.int32)
    return torch.stack((c & 15, c >> 4), dim=-1).view(codes.shape[0], -1)


def pack_codes(c):
    """int [N, K] of 4-bit codes -> uint8 [N, K / 2]"""
    c = c.to(torch.int32)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8).contiguous()


def dequant(codes, exps, dtype=torch.bfloat16):
    """(codes, exps) -> W~ [N, K] in `dtype` (exact in bfloat16, float32 and float64)"""
    c = unpack_codes(codes)
    N, K = c.shape
    lut = torch.tensor(E2M1, dtype=torch.float64, device=codes.device)
    v = lut[(c & 7).long()]
    v = torch.where((c & 8) != 0, -v, v)
    eb = exps.to(torch.int32)
    scale = _pow2(eb - 127)
    scale = torch.where(eb == 0, torch.zeros_like(scale), scale)
    out = (v.view(N, K // BLOCK, BLOCK) * scale[..., None]).view(N, K)
    out = torch.where(out == 0, torch.zeros_like(out), out)                 # byte 0 / code 0: a plain zero
    return out.to(dtype)


def roundtrip(W):
    """W bf16 -> W~ bf16 = dequant(quant(W))"""
    return dequant(*quant(W))


def tile_index(n, k, K):
    """(tile, unit, lane, byte, nibble) of weight (n, k) in tcodes, and (tile, unit, lane, half) of its exponent byte in texps"""
    tile, r, u, g, j = n // 16, n % 16, k // UNIT, (k % UNIT) // 64, k % 64
    lane = g * 16 + r
    return (tile, u, lane, j // 2, j % 2), (tile, u, lane, j // BLOCK)


def tile_pack(codes, exps):
    """logical (codes [N, K / 2], exps [N, K / 32]) -> (tcodes [N / 16, U, 64, 32], texps [N / 16, U, 64, 2])"""
    N, K = codes.shape[0], codes.shape[1] * 2
    assert N % 16 == 0 and K % UNIT == 0
    U = K // UNIT
    tc = codes.view(N // 16, 16, U, 4, 32).permute(0, 2, 3, 1, 4).reshape(N // 16, U, 64, 32).contiguous()      # [tile, r, u, g, 32] -> [tile, u, g, r, 32]
    te = exps.view(N // 16, 16, U, 4, 2).permute(0, 2, 3, 1, 4).reshape(N // 16, U, 64, 2).contiguous()
    return tc, te


def tile_unpack(tc, te):
    """the inverse of tile_pack"""
    T, U = tc.shape[0], tc.shape[1]
    codes = tc.view(T, U, 4, 16, 32).permute(0, 3, 1, 2, 4).reshape(T * 16, U * 128).contiguous()
    exps = te.view(T, U, 4, 16, 2).permute(0, 3, 1, 2, 4).reshape(T * 16, U * 8).contiguous()
    return codes, exps


def weight_bytes(N: int, K: int) -> int:
    """bytes of one projection in this format: half a byte a weight and one byte per block (4.25 bits a weight)"""
    return N * K // 2 + N * K // BLOCK


PROJECTIONS = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
               "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")


def is_projection(name: str) -> bool:
    """True for the state-dict names a w4 engine quantises (the four projections of every decoder layer; q / k / v and gate / up arrive apart and
    are quantised row-wise, so apart or together gives the same codes)"""
    return name.startswith("model.layers.") and name.endswith(PROJECTIONS)


def twin_items(items):
    """(name, tensor) pairs with every decoder projection replaced by W~: what a bf16 engine is loaded with to be the exact reference of a w4 one"""
    for name, t in items:
        yield (name, roundtrip(t.detach().to(torch.bfloat16)) if is_projection(name) else t)      # (on the tensor's own device)
