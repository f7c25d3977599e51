"""Probe builders for the w4 decode GEMV (tests/test_w4_cpu.py, tests/test_gpu_w4.py).  No GPU, no HIP library.

A probe is (codes, exps, X) given directly in the logical order of trace_amd/w4.py — not through the quantiser, so a block may carry any exponent byte
whatever its codes — with an answer every summation order reproduces bit for bit: codes x power-of-two scales spanning 2^3 x integer activations in
[-8, 8] are multiples of 0.5 below 2^10, so a sum over K <= 4096 needs at most 23 bits; probes with a longer K keep the activations in {-1, 0, 1}.
`expected()` is the float64 product cast to fp32; `order_free()` is the probes' own condition (fp32 accumulation forward and backward gives the same).

emulate() restates the kernel's walk over the tile layout in torch (units, lanes, dwords, bytes, nibbles, the lane's two exponent bytes, k-chunks,
the rows it stores) and can be told to make one named mistake; each mistake is caught by a named probe.
"""
from __future__ import annotations

import torch

from trace_amd import w4

SK_ROWS = 256
SENTINEL = -12345.5
FAULTS = ("nibbles_swapped", "byte_sel_off_by_one", "neighbour_block_scale", "next_row_scale", "last_unit_dropped", "chunk_boundary_lost", "rows_past_B_stored")
PROBES = ("pointer", "count_holes", "mixed_scales")
# which probe is named to reject which fault
REJECTS = {"nibbles_swapped": "pointer", "byte_sel_off_by_one": "pointer", "neighbour_block_scale": "mixed_scales", "next_row_scale": "mixed_scales",
           "last_unit_dropped": "count_holes", "chunk_boundary_lost": "count_holes", "rows_past_B_stored": "count_holes"}
EXP0 = 126          # exponent bytes 126 .. 129: scales 0.5 .. 4, a span of 2^3


def _x(B, K, small):
    b = torch.arange(B, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    if small:
        return (((b * 5 + k * 3) % 7) % 3 - 1).to(torch.bfloat16)          # {-1, 0, 1}
    return (((b * 7 + k * 3) % 17) - 8).to(torch.bfloat16)                 # integers in [-8, 8]; neighbours in k always differ


def _exps(N, K):
    n = torch.arange(N, dtype=torch.int64)[:, None]
    kb = torch.arange(K // 32, dtype=torch.int64)[None, :]
    return (EXP0 + (n * 3 + kb) % 4).to(torch.uint8)                        # differs between neighbouring blocks and neighbouring rows


def pointer(N, K, B):
    """one nonzero code per row, at a k that walks over every position of a 64-k lane run, every lane group and every unit as n grows: the answer is
    X[b, k_n] * W~[n, k_n], so reading any other nibble, byte, lane or unit than the stated one shows"""
    n = torch.arange(N, dtype=torch.int64)
    kn = (n * 37 + (n // 16) * 11 + (n // 64) * 256) % K
    c = torch.zeros((N, K), dtype=torch.int32)
    c[n, kn] = (1 + n % 7 + 8 * ((n // 7) % 2)).to(torch.int32)            # magnitudes 1..7, both signs
    return w4.pack_codes(c), _exps(N, K), _x(B, K, K > 4096)


def count_holes(N, K, B):
    """every code 1.0 under scale 1 except holes; activations of ones (K <= 4096: small integers that vary with the row): the answer counts the
    k that took part, so a unit or a chunk edge lost or taken twice shows"""
    n = torch.arange(N, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    c = torch.where((k * 7 + n) % 13 == 0, 0, 2).to(torch.int32)
    exps = torch.full((N, K // 32), 127, dtype=torch.uint8)
    X = torch.ones((B, K), dtype=torch.bfloat16)
    if K <= 4096:
        X = X * (1 + torch.arange(B) % 8).to(torch.bfloat16)[:, None]
    return w4.pack_codes(c), exps, X


def mixed_scales(N, K, B, seed=0):
    """seeded random codes under exponent bytes that differ from block to block and row to row"""
    g = torch.Generator().manual_seed(seed + N * 31 + K)
    c = torch.randint(0, 16, (N, K), generator=g, dtype=torch.int32)
    c = torch.where(c == 8, torch.zeros_like(c), c)                          # no negative zeros
    return w4.pack_codes(c), _exps(N, K), _x(B, K, K > 4096)


def build(name, N, K, B):
    return {"pointer": pointer, "count_holes": count_holes, "mixed_scales": mixed_scales}[name](N, K, B)


def expected(codes, exps, X):
    """float64 X . W~^T cast to fp32 [B, N]"""
    return (X.double() @ w4.dequant(codes, exps, torch.float64).t()).float()


def order_free(codes, exps, X):
    """True iff sequential fp32 accumulation over k, forward and backward, both give the float64 answer exactly"""
    W = w4.dequant(codes, exps, torch.float32)
    Xf = X.float()
    want = expected(codes, exps, X)
    K = W.shape[1]
    for order in (range(K), range(K - 1, -1, -1)):
        acc = torch.zeros((X.shape[0], W.shape[0]), dtype=torch.float32)
        for k in order:
            acc = acc + Xf[:, k, None] * W[None, :, k]
        if not torch.equal(acc, want):
            return False
    return True


def emulate(tc, te, X, N, K, B, plan, fault=None):
    """The kernel's walk in torch: tile copies (w4.tile_pack) + X [B, K] -> partial rows [KS + 1, SK_ROWS, N] fp32, pre-filled with SENTINEL (the last
    chunk is a guard nothing may write).  plan: {"KS", "chunk_units", "NB"} of trace_op_skinny_w4_plan."""
    assert fault is None or fault in FAULTS
    T, U = N // 16, K // 256
    c = tc.view(T, U, 64, 8, 4).to(torch.int32)                              # [tile, unit, lane, dword, byte]
    if fault == "byte_sel_off_by_one":
        c = c.roll(-1, dims=-1)
    lo, hi = c & 15, c >> 4
    if fault == "nibbles_swapped":
        lo, hi = hi, lo
    code = torch.stack((lo, hi), dim=-1).view(T, U, 64, 8, 8)                # [.., dword = fragment q, element]
    e = te.view(T, U, 4, 16, 2).to(torch.int32)                              # [tile, unit, g, r, half]
    if fault == "neighbour_block_scale":
        e = e.flip(-1)
    if fault == "next_row_scale":
        e = e.roll(-1, dims=3)
    e = e.reshape(T, U, 64, 2)
    lut = torch.tensor(w4.E2M1, dtype=torch.float64)
    v = lut[(code & 7).long()]
    v = torch.where((code & 8) != 0, -v, v)
    scale = torch.pow(torch.tensor(2.0, dtype=torch.float64), (torch.clamp(e, min=1) - 127).double())     # byte 0 reads as 2^-126 beside zero codes
    v = v * scale.repeat_interleave(4, dim=-1)[..., None]                    # dwords 0-3: first byte, 4-7: second
    # lane (r, g), fragment q, element i is k = unit * 256 + g * 64 + q * 8 + i of row tile * 16 + r
    Wt = v.view(T, U, 4, 16, 8, 8).permute(0, 3, 1, 2, 4, 5).reshape(N, U, 256)
    Xu = X.double().view(B, U, 256)
    KS, chunk = plan["KS"], plan["chunk_units"]
    out = torch.full((KS + 1, SK_ROWS, N), SENTINEL, dtype=torch.float32)
    rows = 16 * plan["NB"] if fault == "rows_past_B_stored" else B
    for ks in range(KS):
        u0, u1 = ks * chunk, min(U, (ks + 1) * chunk)
        if fault == "chunk_boundary_lost" and ks > 0:
            u0 += 1
        if fault == "last_unit_dropped" and u1 == U:
            u1 -= 1
        part = torch.einsum("buk,nuk->bn", Xu[:, u0:u1], Wt[:, u0:u1]).float() if u1 > u0 else torch.zeros((B, N))
        out[ks, :B] = part
        if rows > B:
            out[ks, B:rows] = part[B - 1]                                    # rows >= B park row B - 1's activations
    return out


def result(out, B):
    """(product [B, N], True iff rows >= B of every chunk and the guard chunk still hold SENTINEL)"""
    clean = bool((out[:-1, B:] == SENTINEL).all()) and bool((out[-1] == SENTINEL).all())
    return out[:-1, :B].sum(0), clean
