"""Prefill cache-write probes: the three row movers that WRITE the 16-bit KV cache and the embedding rows of every request — rope_kv_kernel and
gather_rows_kernel (csrc/llm.hip), transpose_v_kernel<64|128> (csrc/attn.hip) — each alone, on inputs where one wrong offset, sign or stride changes
bits, in buffers pre-filled with a sentinel so that a probe says where a store may land and nowhere else.

  references   RoPE: float64 from the 16-bit inputs and the fp32 table values as given, o1 = x1 c - x2 s, o2 = x2 c + x1 s, the partner of d is
               d + hd/2, ONE rounding to the element type.  Row r of the launch has sq = seq_len > 0 ? r / seq_len : 0,
               pos = pos_arr ? pos_arr[r] : pos0 + r - sq seq_len, slot = slot_arr ? slot_arr[r] : slot0 + sq; q heads are rewritten in place, k head h
               goes to kcache[slot slot_stride + h kv_head_stride + pos hd], v head h to the same offset of the optional row-major vcache.
               Transpose and gather: pure placement, bit for bit (16-bit patterns, compared as int16).
  judge        exact probes: bit equal.  Gaussian RoPE: |got - ref| <= half a 16-bit ulp of ref + E, E = 2^-23 (|x1 c| + |x2 s|) — two fp32 products
               and one fp32 add, each within 2^-24 relative, contracted into an FMA or not.  The bound is additive, which is encode_probes.bound's
               treatment of a value within E of a rounding tie: either neighbour is inside it.  Nothing in it comes from a kernel's output.
               Every word outside the judged windows must still hold what it held (sentinel, or the untouched k | v columns of qkv).
  emulations   torch restatements of the kernels' structure (16-byte items of a grid-stride loop over 4096 x 256 threads; 64-position tiles written in
               8-position chunks, the chunk that straddles p0 element by element), each taking fault=<name>: tests/test_prefill_glue_probes_cpu.py shows
               every fault rejected by a named probe, and which of them a prefill-against-prefill comparison cannot see.

Runs on the CPU and on a device; nothing here imports the HIP library."""
from types import SimpleNamespace

import torch

import encode_probes as EP
from gemm_probes import SENTINEL, round16, subnormal_step

GRID_THREADS = 4096 * 256            # both llm.hip launchers cap the grid at 4096 workgroups of 256 threads; further items take the grid-stride loop
PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)        # perm = 1: position j of every 16 holds key PERM16[j]


def round_up(x, m):
    return (x + m - 1) // m * m


def sentinel_buf(n, dtype, device="cpu"):
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=device).view(dtype)


def bits(t):
    return t.view(torch.int16)


def codes(n, salt, device="cpu"):
    """n 16-bit patterns, consecutive ones always different, none equal to the sentinel or to zero (so a zero fill and an untouched word both show)"""
    c = (torch.arange(n, dtype=torch.int64, device=device) * 40503 + 12345 + 7919 * salt) & 0xFFFF
    c = torch.where((c == SENTINEL) | (c == 0), torch.ones_like(c), c)
    return torch.where(c >= 32768, c - 65536, c).to(torch.int16)


# ================================================================================================================ RoPE
ROPE_EXACT = ("identity", "quarter-turn", "per-position", "half", "heads")
# name -> geometry and launch form.  ctx: positions a kv head holds (kv_head_stride = ctx hd, slot_stride = nkv kv_head_stride + gap)
ROPE_CASES = {
    "single-R7":     dict(nq=4, nkv=1, R=7, seq_len=7, slot0=1, pos0=0, nslots=3, ctx=16),
    "single-R1":     dict(nq=4, nkv=1, R=1, seq_len=1, slot0=0, pos0=0, nslots=1, ctx=8),
    "past-R64":      dict(nq=4, nkv=1, R=64, seq_len=64, slot0=2, pos0=37, nslots=3, ctx=128),
    "multi-3xL7":    dict(nq=32, nkv=8, R=21, seq_len=7, slot0=1, pos0=5, nslots=5, ctx=16),
    "arrays":        dict(nq=4, nkv=1, R=7, seq_len=0, slot0=0, pos0=0, nslots=9, ctx=32, slot_arr=(5, 0, 8, 2, 7, 1, 4), pos_arr=(3, 31, 0, 17, 9, 30, 1)),
    "vcache":        dict(nq=4, nkv=1, R=7, seq_len=7, slot0=1, pos0=3, nslots=2, ctx=16, with_v=True),
    "vcache-32/8":   dict(nq=32, nkv=8, R=1, seq_len=1, slot0=1, pos0=9, nslots=2, ctx=16, with_v=True),
    "ld-padded":     dict(nq=32, nkv=8, R=7, seq_len=7, slot0=0, pos0=2, nslots=2, ctx=16, ld_pad=72),
    "ld-padded-4/1": dict(nq=4, nkv=1, R=64, seq_len=32, slot0=0, pos0=1, nslots=2, ctx=64, ld_pad=8),
    # 2760 rows x 48 heads x 8 items = 1,059,840 > 4096 x 256: rows from 2730 on are reached by the grid-stride loop only
    "grid-stride":   dict(nq=32, nkv=8, R=2760, seq_len=920, slot0=1, pos0=3, nslots=4, ctx=928),
}
ROPE_SMALL = tuple(k for k in ROPE_CASES if k != "grid-stride")
ROPE_FAULTS = ("interleaved_pairs", "sin_sign", "second_half_from_rotated_first", "q_not_rotated", "k_not_rotated", "pos_ignores_past",
               "pos_not_reset_per_sequence", "pos_off_by_one", "slot_not_advanced", "k_head_from_q_index", "table_stride_hd", "rows_past_grid_dropped",
               "padding_columns_written", "products_rounded_to_16")
_PAIRS = ((1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0), (0.5, 0.5), (0.5, -0.5), (-0.5, 0.5), (-0.5, -0.5))


def exact_tables(name, rows, half, device="cpu"):
    """(cos, sin) fp32 [rows, half] with entries from {0, +-1, +-1/2}, chosen per (position, j)"""
    p = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    j = torch.arange(half, dtype=torch.int64, device=device)[None, :]
    one, zero = torch.ones((rows, half), device=device), torch.zeros((rows, half), device=device)
    if name == "identity":
        return one, zero
    if name in ("quarter-turn", "heads"):                       # c = 0, s = +-1: the sign and the partner
        sgn = 1.0 - 2.0 * (((p * 5 + j * 3 + (p * j) // 7) % 2).float())
        return zero, sgn
    if name == "half":
        return 0.5 * one, 0.5 * one
    if name == "per-position":                                  # the base-8 digits of the position pick one of eight (c, s) pairs: a wrong pos changes bits
        digit = (p >> (3 * (j % 4))) & 7
        k = (digit + j) % 8
        pc = torch.tensor([q[0] for q in _PAIRS], device=device)
        ps = torch.tensor([q[1] for q in _PAIRS], device=device)
        return pc[k].contiguous(), ps[k].contiguous()
    raise KeyError(name)


def hashed_rows(R, nh, hd, device="cpu"):
    """integers in -63 .. 63 hashed from (row, head, d): neighbours along every index, and d against its partners d + hd/2 and d ^ 1, differ; every
    product with {0, +-1, +-1/2} and every sum of two is exact in bf16 and fp16"""
    r = torch.arange(R, dtype=torch.int64, device=device)[:, None, None]
    h = torch.arange(nh, dtype=torch.int64, device=device)[None, :, None]
    d = torch.arange(hd, dtype=torch.int64, device=device)[None, None, :]
    return ((r * 31 + h * 17 + d * 3 + (d // (hd // 2)) * 40) % 127 - 63).double()


def rope_probe(name, case, dtype, device="cpu", hd=128):
    """One launch: inputs, tables and sentinel-filled destinations.  name: one of ROPE_EXACT, or "gaussian" (real tables of 4096 rows are the caller's:
    gaussian_rope_probe)."""
    g = dict(ROPE_CASES[case]) if isinstance(case, str) else dict(case)
    nq, nkv, R = g["nq"], g["nkv"], g["R"]
    nh, half = nq + 2 * nkv, hd // 2
    width = nh * hd
    ld = width + g.get("ld_pad", 0)
    ctx, nslots = g["ctx"], g["nslots"]
    khs = ctx * hd
    ss = nkv * khs + g.get("slot_gap", 0)
    if name == "heads":                                         # the value names the head: q, k and v blocks and every kv head distinguishable
        h = torch.arange(nh, dtype=torch.float64, device=device)[None, :, None]
        first = (torch.arange(hd, device=device) < half)[None, None, :]
        x = torch.where(first, h + 1, 2 * (h + 1)).expand(R, nh, hd) + 0 * hashed_rows(R, nh, hd, device)
    else:
        x = hashed_rows(R, nh, hd, device)
    table_rows = g.get("table_rows", ctx)
    cos_t, sin_t = exact_tables(name, table_rows, half, device)
    return _rope_lay(name, case if isinstance(case, str) else "custom", x, cos_t, sin_t, g, dtype, device, hd, ld, ss, khs, nslots, exact=True)


def _rope_lay(name, case, x, cos_t, sin_t, g, dtype, device, hd, ld, ss, khs, nslots, exact):
    nq, nkv, R = g["nq"], g["nkv"], g["R"]
    nh = nq + 2 * nkv
    qkv = sentinel_buf(R * ld, dtype, device)
    qkv.view(R, ld)[:, :nh * hd] = round16(x.reshape(R, nh * hd), dtype, exact=exact)
    kcache = sentinel_buf(nslots * ss, dtype, device)
    vcache = sentinel_buf(nslots * ss, dtype, device) if g.get("with_v") else None
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=device)
    return SimpleNamespace(name=name, case=case, dtype=dtype, exact=exact, R=R, nq=nq, nkv=nkv, hd=hd, ld=ld, seq_len=g["seq_len"], slot0=g["slot0"],
                           pos0=g["pos0"], slot_arr=i32(g.get("slot_arr")), pos_arr=i32(g.get("pos_arr")), slot_stride=ss, kv_head_stride=khs, nslots=nslots,
                           qkv=qkv, kcache=kcache, vcache=vcache, cos_t=cos_t.contiguous(), sin_t=sin_t.contiguous())


def gaussian_rope_probe(case, dtype, tables, device="cpu", seed=0, hd=128):
    """Gaussian rows (sigma 2) through the real tables (encode_probes.rope_tables(4096, hd, rope_theta): the engine's)"""
    g = dict(case)
    nq, nkv, R = g["nq"], g["nkv"], g["R"]
    nh = nq + 2 * nkv
    x = (2.0 * torch.randn((R, nh, hd), generator=torch.Generator().manual_seed(seed), dtype=torch.float32)).double().to(device)
    khs = g["ctx"] * hd
    return _rope_lay("gaussian", g.get("label", "custom"), x, tables[0].to(device), tables[1].to(device), g, dtype, device, hd, nh * hd + g.get("ld_pad", 0),
                     nkv * khs, khs, g["nslots"], exact=False)


# positions 0 and 1, the last row of a 4096-row table, an append at an odd past of three sequences, array form at scattered positions
GAUSSIAN_CASES = (
    dict(label="pos0", nq=4, nkv=1, R=7, seq_len=7, slot0=0, pos0=0, nslots=1, ctx=16),
    dict(label="table-end", nq=4, nkv=1, R=64, seq_len=64, slot0=0, pos0=4096 - 64, nslots=1, ctx=4096),
    dict(label="odd-past-3seq", nq=32, nkv=8, R=21, seq_len=7, slot0=1, pos0=1001, nslots=4, ctx=1024),
    dict(label="arrays", nq=4, nkv=1, R=5, seq_len=0, slot0=0, pos0=0, nslots=5, ctx=4096, slot_arr=(4, 2, 0, 1, 3), pos_arr=(4095, 0, 1, 2047, 333)),
)


def rope_rows(pr, fault=None):
    """(slot, pos) int64 [R]: the documented rule of a row's cache slot and position"""
    dev = pr.qkv.device
    r = torch.arange(pr.R, dtype=torch.int64, device=dev)
    sq = r // pr.seq_len if pr.seq_len > 0 else torch.zeros_like(r)
    if fault == "pos_not_reset_per_sequence":
        pos = pr.pos0 + r
    elif fault == "pos_ignores_past":
        pos = r - sq * pr.seq_len
    else:
        pos = pr.pos0 + r - sq * pr.seq_len
    slot = pr.slot0 + (torch.zeros_like(sq) if fault == "slot_not_advanced" else sq)
    if pr.pos_arr is not None:
        pos = pr.pos_arr.to(torch.int64)
    if pr.slot_arr is not None:
        slot = pr.slot_arr.to(torch.int64)
    return slot, pos


def _rope_inputs(pr):
    nh = pr.nq + 2 * pr.nkv
    return pr.qkv.view(pr.R, pr.ld)[:, :nh * pr.hd].reshape(pr.R, nh, pr.hd)


def _cache_index(pr, slot, pos):
    """flat cache offsets [R, nkv, hd] of the rows (slot[r], kv head, pos[r])"""
    dev = pr.qkv.device
    h = torch.arange(pr.nkv, dtype=torch.int64, device=dev)[None, :, None]
    d = torch.arange(pr.hd, dtype=torch.int64, device=dev)[None, None, :]
    return slot[:, None, None] * pr.slot_stride + h * pr.kv_head_stride + pos[:, None, None] * pr.hd + d


def rope_reference(pr):
    """float64: the rotated q and k heads, their E, and the buffers a correct launch leaves (judged windows hold the reference rounded once)"""
    x = _rope_inputs(pr).double()
    half = pr.hd // 2
    slot, pos = rope_rows(pr)
    c, s = pr.cos_t.double()[pos][:, None, :], pr.sin_t.double()[pos][:, None, :]
    rot = x[:, :pr.nq + pr.nkv]
    x1, x2 = rot[..., :half], rot[..., half:]
    o = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    E = 2.0 ** -23 * torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    o16 = round16(o, pr.dtype, exact=pr.exact)
    qkv = pr.qkv.clone()
    qkv.view(pr.R, pr.ld)[:, :pr.nq * pr.hd] = o16[:, :pr.nq].reshape(pr.R, -1)
    idx = _cache_index(pr, slot, pos)
    kcache = pr.kcache.clone()
    kcache[idx.reshape(-1)] = o16[:, pr.nq:].reshape(-1)
    vcache = None
    if pr.vcache is not None:
        vcache = pr.vcache.clone()
        vcache[idx.reshape(-1)] = _rope_inputs(pr)[:, pr.nq + pr.nkv:].reshape(-1)
    bound = torch.clamp(EP.half_ulp(o, pr.dtype) + E, min=subnormal_step(pr.dtype))
    return SimpleNamespace(o=o, bound=bound, idx=idx, qkv=qkv, kcache=kcache, vcache=vcache)


def rope_judge(pr, got, ref=None):
    """got = (qkv, kcache, vcache) after the launch -> (error / bound over the rotated q and k elements, everything else intact).  Exact probes: the ratio
    is 0 where the bits are the reference's and inf elsewhere."""
    ref = ref or rope_reference(pr)
    qkv, kcache, vcache = got
    R, nq, hd = pr.R, pr.nq, pr.hd
    gq = qkv.view(R, pr.ld)[:, :nq * hd].reshape(R, nq, hd)
    gk = kcache[ref.idx.reshape(-1)].reshape(R, pr.nkv, hd)
    g = torch.cat([gq, gk], 1)
    if pr.exact:
        want = torch.cat([ref.qkv.view(R, pr.ld)[:, :nq * hd].reshape(R, nq, hd), ref.kcache[ref.idx.reshape(-1)].reshape(R, pr.nkv, hd)], 1)
        ratio = 0.0 if bool((bits(g) == bits(want)).all()) else float("inf")
    else:
        q = (g.double() - ref.o).abs() / ref.bound
        ratio = float(torch.nan_to_num(q, nan=float("inf"), posinf=float("inf")).max())
    # outside the judged windows: bit equal to the reference buffers (which hold the inputs' own words there)
    oq, ok = bits(qkv).clone(), bits(kcache).clone()
    eq, ek = bits(ref.qkv).clone(), bits(ref.kcache).clone()
    oq.view(R, pr.ld)[:, :nq * hd] = 0
    eq.view(R, pr.ld)[:, :nq * hd] = 0
    ok[ref.idx.reshape(-1)] = 0
    ek[ref.idx.reshape(-1)] = 0
    intact = bool((oq == eq).all()) and bool((ok == ek).all())
    if pr.vcache is not None:
        intact = intact and vcache is not None and bool((bits(vcache) == bits(ref.vcache)).all())
    return ratio, intact


def emulate_rope(pr, fault=None, fma=False, swap_order=False):
    """rope_kv_kernel in torch: fp32 products and sum per 16-byte item of the grid-stride loop.  fma: the second product contracted into the sum;
    swap_order: the sum taken as (-x2 s) + x1 c.  Returns (qkv, kcache, vcache)."""
    assert fault is None or fault in ROPE_FAULTS, fault
    dev = pr.qkv.device
    R, nq, nkv, hd = pr.R, pr.nq, pr.nkv, pr.hd
    nh, half = nq + 2 * nkv, hd // 2
    x = _rope_inputs(pr).float()
    slot, pos = rope_rows(pr, fault)
    tpos = pos + 1 if fault == "pos_off_by_one" else pos
    j = torch.arange(half, dtype=torch.int64, device=dev)[None, :]
    flat_c, flat_s = pr.cos_t.reshape(-1), pr.sin_t.reshape(-1)
    ti = (tpos[:, None] * (hd if fault == "table_stride_hd" else half) + j) % flat_c.numel()
    c, s = flat_c[ti][:, None, :], flat_s[ti][:, None, :]
    if fault == "sin_sign":
        s = -s
    rot = x[:, :nq + nkv]
    if fault == "interleaved_pairs":
        x1, x2 = rot[..., 0::2], rot[..., 1::2]
    else:
        x1, x2 = rot[..., :half], rot[..., half:]

    def combine(a, ca, b, sb):                                  # a ca + b sb in fp32
        if fault == "products_rounded_to_16":
            return (a * ca).to(pr.dtype).float() + (b * sb).to(pr.dtype).float()
        if fma:
            return torch.addcmul((a * ca).double(), b.double(), sb.double()).float()          # one rounding of the second product and the sum
        return (b * sb) + (a * ca) if swap_order else (a * ca) + (b * sb)
    o1 = combine(x1, c, x2, -s)
    o2 = combine(x2, c, (o1 if fault == "second_half_from_rotated_first" else x1), s)
    if fault == "interleaved_pairs":
        o = torch.stack([o1, o2], -1).reshape(R, nq + nkv, hd)
    else:
        o = torch.cat([o1, o2], -1)
    o16 = o.to(pr.dtype)
    src = _rope_inputs(pr)
    if fault == "q_not_rotated":
        o16[:, :nq] = src[:, :nq]
    if fault == "k_not_rotated":
        o16[:, nq:] = src[:, nq:nq + nkv]
    if fault == "k_head_from_q_index":                           # kv head j stored from the head at index j (a q head) instead of nq + j
        o16[:, nq:] = o16[:, :nkv].clone()
    # which (row, head) the grid reaches: item i = (r nh + head) (hd / 16) + lane; rows_past_grid_dropped stops at the grid's own threads
    done = torch.ones((R, nh), dtype=torch.bool, device=dev)
    if fault == "rows_past_grid_dropped":
        first = (torch.arange(R, dtype=torch.int64, device=dev)[:, None] * nh + torch.arange(nh, dtype=torch.int64, device=dev)[None, :]) * (half // 8)
        done = first < GRID_THREADS
    qkv, kcache = pr.qkv.clone(), pr.kcache.clone()
    qv = qkv.view(R, pr.ld)
    newq = torch.where(done[:, :nq, None], o16[:, :nq], src[:, :nq])
    qv[:, :nq * hd] = newq.reshape(R, -1)
    if fault == "padding_columns_written" and pr.ld > nh * hd:
        qv[:, nh * hd:] = 0
    idx = _cache_index(pr, slot, pos) % kcache.numel()          # (a fault's wrong row may leave the cache: wrapped, it still lands on a wrong word)
    keep = done[:, nq:nq + nkv, None].expand(R, nkv, hd).reshape(-1)
    kcache[idx.reshape(-1)[keep]] = o16[:, nq:].reshape(-1)[keep]
    vcache = None
    if pr.vcache is not None:
        vcache = pr.vcache.clone()
        keepv = done[:, nq + nkv:, None].expand(R, nkv, hd).reshape(-1)
        vcache[idx.reshape(-1)[keepv]] = src[:, nq + nkv:].reshape(-1)[keepv]
    return qkv, kcache, vcache


# ================================================================================================================ transpose
TRANSPOSE_P0 = (0, 1, 7, 8, 9, 63, 64, 65, 100)
TRANSPOSE_N = (1, 2, 7, 8, 55, 64, 65, 130)
TRANSPOSE_FAULTS = ("p0_chunk_clobbered", "no_zero_fill", "zero_fill_past_block", "rows_past_n_read", "perm_ignored", "perm_when_zero", "p0_mod_64_ignored",
                    "batch_head_strides_swapped")


def transpose_cases(hd):
    """(label, kwargs of transpose_probe): every p0 x n without perm, perm = 1 at p0 = 0, p0 + n == dst_rs, dense and engine-like strides"""
    out = []
    for p0 in TRANSPOSE_P0:
        for n in TRANSPOSE_N:
            out.append((f"p0={p0}-n={n}", dict(hd=hd, p0=p0, n=n)))
    for n in (1, 7, 16, 55, 64, 128, 130):
        out.append((f"perm-n={n}", dict(hd=hd, p0=0, n=n, perm=1)))
    out.append(("perm-n=128-tight", dict(hd=hd, p0=0, n=128, perm=1, tight=True)))
    for p0, n in ((0, 64), (63, 65), (64, 64), (100, 28), (9, 55), (65, 130)):
        out.append((f"tight-p0={p0}-n={n}", dict(hd=hd, p0=p0, n=n, tight=True)))            # p0 + n == dst_rs, or its last block
    out.append(("dense-p0=9-n=55", dict(hd=hd, p0=9, n=55, dense=True)))
    return out


def transpose_probe(hd, p0, n, dtype, perm=0, tight=False, dense=False, heads=2, batch=2, device="cpu"):
    """Two heads x two batches.  Source: heads interleaved in a row as the prefill's qkv rows are (src_hs = hd), rows and batches padded; destination:
    [batch][head][hd][dst_rs] with gaps between heads and batches.  tight: dst_rs = round_up(p0 + n, 64) (no block past the last one written)."""
    tail = 0 if dense else 8
    src_rs = heads * hd + tail
    src_hs = hd
    src_bs = (n + (0 if dense else 3)) * src_rs
    src_rows = batch * (n + (0 if dense else 3)) + 64                     # 64 further rows: what a read past n finds is not a fault of the emulation
    src = codes(src_rows * src_rs, 1, device).view(dtype)
    dst_rs = round_up(p0 + n, 64) + (0 if tight else 64)
    dst_hs = hd * dst_rs + (0 if dense else 16)
    dst_bs = heads * dst_hs + (0 if dense else 24)
    dst = sentinel_buf(batch * dst_bs + 8, dtype, device)
    return SimpleNamespace(hd=hd, p0=p0, n=n, perm=perm, heads=heads, batch=batch, dtype=dtype, src=src, src_bs=src_bs, src_hs=src_hs, src_rs=src_rs, dst=dst,
                           dst_bs=dst_bs, dst_hs=dst_hs, dst_rs=dst_rs)


def _src_rows(pr, b, h, rows):
    """int16 [len(rows), hd]: source rows `rows` of (b, h)"""
    d = torch.arange(pr.hd, dtype=torch.int64, device=pr.src.device)[None, :]
    return bits(pr.src)[b * pr.src_bs + h * pr.src_hs + rows[:, None] * pr.src_rs + d]


def transpose_reference(pr):
    """the destination a correct launch leaves: dst[b, h, d, p0 + r] = src[b, h, r, d]; zeros in [p0 + n, round_up(p0 + n, 64)); all else as it was.
    perm = 1: position q holds key 16 (q / 16) + PERM16[q % 16] (zero where that key is past n)."""
    dev = pr.src.device
    out = bits(pr.dst).clone()
    end = round_up(pr.p0 + pr.n, 64)
    q = torch.arange(pr.p0, end, dtype=torch.int64, device=dev)
    key = q - pr.p0
    if pr.perm:
        key = (q // 16) * 16 + torch.tensor(PERM16, dtype=torch.int64, device=dev)[q % 16]
    live = key < pr.n
    d = torch.arange(pr.hd, dtype=torch.int64, device=dev)[None, :]
    for b in range(pr.batch):
        for h in range(pr.heads):
            v = _src_rows(pr, b, h, torch.where(live, key, torch.zeros_like(key)))
            v = torch.where(live[:, None], v, torch.zeros_like(v))
            out[b * pr.dst_bs + h * pr.dst_hs + d * pr.dst_rs + q[:, None]] = v
    return out


def emulate_transpose(pr, fault=None):
    """transpose_v_kernel in torch: one 64-position tile per block, 8-position chunks, the chunk that straddles p0 written element by element.
    Returns the destination's int16 words."""
    assert fault is None or fault in TRANSPOSE_FAULTS, fault
    dev = pr.src.device
    out = bits(pr.dst).clone()
    p0, n, hd = pr.p0, pr.n, pr.hd
    perm = pr.perm
    if fault == "perm_ignored":
        perm = 0
    if fault == "perm_when_zero" and not pr.perm:
        perm = 1
    nblk = (p0 + n + 63) // 64 - p0 // 64
    nsrc = bits(pr.src).numel()
    d = torch.arange(hd, dtype=torch.int64, device=dev)
    P = torch.tensor(PERM16, dtype=torch.int64, device=dev)
    for b in range(pr.batch):
        for h in range(pr.heads):
            base = b * pr.dst_hs + h * pr.dst_bs if fault == "batch_head_strides_swapped" else b * pr.dst_bs + h * pr.dst_hs
            for blk in range(nblk + (1 if fault == "zero_fill_past_block" else 0)):
                t0 = (blk if fault == "p0_mod_64_ignored" else p0 // 64 + blk) * 64
                if t0 + 64 > pr.dst_rs:
                    continue
                row = torch.arange(64, dtype=torch.int64, device=dev)
                sr = t0 + row - (p0 % 64 if fault == "p0_mod_64_ignored" else p0)
                live = (sr >= 0) & ((sr < n) | (fault == "rows_past_n_read"))
                off = b * pr.src_bs + h * pr.src_hs + torch.where(live, sr, torch.zeros_like(sr))[:, None] * pr.src_rs + d[None, :]
                tile = torch.where(live[:, None], bits(pr.src)[off % nsrc], torch.zeros((64, hd), dtype=torch.int16, device=dev))
                if perm:
                    tile = tile[(row // 16) * 16 + P[row % 16]]
                lo = p0 % 64 if fault == "p0_mod_64_ignored" else p0
                for tc in range(8):
                    cp = t0 + tc * 8
                    if cp >= lo or fault == "p0_chunk_clobbered":
                        first = cp
                    elif cp + 8 > lo:
                        first = lo
                    else:
                        continue
                    if fault == "p0_chunk_clobbered" and cp + 8 <= lo:
                        continue
                    last = cp + 8
                    if fault == "no_zero_fill":
                        last = min(last, max(lo + n, first))
                    if last <= first:
                        continue
                    q = torch.arange(first, last, dtype=torch.int64, device=dev)
                    out[base + d[None, :] * pr.dst_rs + q[:, None]] = tile[q - t0]
    return out


def transpose_judge(pr, got):
    """got: the destination after the launch (any 16-bit view) -> bit equal to the reference everywhere"""
    return bool((bits(got).reshape(-1) == transpose_reference(pr)).all())


def transpose_region_report(pr, got):
    """which part of the contract a wrong destination breaks: 'rows', 'zero-fill', 'before-p0', 'past-block', 'padding'"""
    dev = pr.src.device
    ref, g = transpose_reference(pr), bits(got).reshape(-1)
    bad = g != ref
    end = round_up(pr.p0 + pr.n, 64)
    region = torch.full_like(ref, 4, dtype=torch.int64)                    # padding
    d = torch.arange(pr.hd, dtype=torch.int64, device=dev)[None, :]
    q = torch.arange(pr.dst_rs, dtype=torch.int64, device=dev)
    kind = torch.where(q < pr.p0, 2, torch.where(q < pr.p0 + pr.n, 0, torch.where(q < end, 1, 3)))
    for b in range(pr.batch):
        for h in range(pr.heads):
            region[b * pr.dst_bs + h * pr.dst_hs + d * pr.dst_rs + q[:, None]] = kind[:, None].expand(-1, pr.hd)
    names = ("rows", "zero-fill", "before-p0", "past-block", "padding")
    return sorted({names[int(k)] for k in region[bad].unique()})


# ================================================================================================================ gather
GATHER_ROWS = (5, 3, 7, 2, 1, 4)          # six tables of different row counts
GATHER_FAULTS = ("kind_ignored", "last_chunk_dropped", "gather_rows_past_grid_dropped")
GATHER_CASES = (("H8-L1", 8, 1), ("H8-L64", 8, 64), ("H256-L1", 256, 1), ("H256-L77", 256, 77), ("H4096-L1", 4096, 1), ("H4096-L44", 4096, 44),
                ("H4096-grid-stride", 4096, 2051))            # 2051 x 512 chunks = 1,050,112 > 4096 x 256


def gather_probe(H, L, dtype, device="cpu"):
    """Six tables of distinct contents; kind / row cover every table, the first and last row of each, repeated rows; the output has 3 sentinel rows past L"""
    tabs = [codes(r * H, 10 + k, device).view(dtype) for k, r in enumerate(GATHER_ROWS)]
    kind, row = [], []
    for k, r in enumerate(GATHER_ROWS):                        # first, last, last again, first again of every table
        kind += [k, k, k, k]
        row += [0, r - 1, r - 1, 0]
    i = 0
    while len(kind) < L:                                        # then a fixed walk over all (table, row) pairs
        k = (i * 5 + 2) % 6
        kind.append(k)
        row.append((i * 3 + i // 6) % GATHER_ROWS[k])
        i += 1
    if L < len(kind):                                           # short lists: the LAST row of the LAST tables stays in
        kind, row = kind[-L:], row[-L:]
    out = sentinel_buf((L + 3) * H, dtype, device)
    return SimpleNamespace(H=H, L=L, dtype=dtype, tabs=tabs, kind=torch.tensor(kind, dtype=torch.int32, device=device),
                           row=torch.tensor(row, dtype=torch.int32, device=device), out=out)


def gather_reference(pr):
    out = bits(pr.out).clone()
    for k, t in enumerate(pr.tabs):
        m = pr.kind == k
        if bool(m.any()):
            out.view(-1, pr.H)[:pr.L][m] = bits(t).view(-1, pr.H)[pr.row[m].to(torch.int64)]
    return out


def emulate_gather(pr, fault=None):
    """gather_rows_kernel in torch: item i = row (H / 8) + 16-byte chunk of a grid-stride loop"""
    assert fault is None or fault in GATHER_FAULTS, fault
    dev = pr.out.device
    out = bits(pr.out).clone()
    cpr = pr.H // 8
    rows = torch.arange(pr.L, dtype=torch.int64, device=dev)
    nchunk = torch.full((pr.L,), cpr, dtype=torch.int64, device=dev)                  # leading chunks of each row that get stored
    if fault == "last_chunk_dropped":
        nchunk = nchunk - 1
    if fault == "gather_rows_past_grid_dropped":
        nchunk = torch.clamp(GRID_THREADS - rows * cpr, min=0, max=cpr)
    col = torch.arange(pr.H, dtype=torch.int64, device=dev)[None, :]
    for k, t in enumerate(pr.tabs):
        m = torch.ones_like(pr.kind, dtype=torch.bool) if fault == "kind_ignored" else pr.kind == k
        if fault == "kind_ignored" and k != 0:
            continue
        if not bool(m.any()):
            continue
        tv = bits(t).view(-1, pr.H)
        v = tv[pr.row[m].to(torch.int64) % tv.shape[0]]
        w = out.view(-1, pr.H)[:pr.L][m]
        out.view(-1, pr.H)[:pr.L][m] = torch.where(col < (nchunk[m] * 8)[:, None], v, w)
    return out


def gather_judge(pr, got):
    return bool((bits(got).reshape(-1) == gather_reference(pr)).all())


# ================================================================================================================ a prefill's two cache writes
def emulate_prefill_writes(L, past, dtype, rope_fault=None, transpose_fault=None, nq=4, nkv=1, hd=128, ctx=128):
    """The K rows and V^T columns of ONE sequence of L rows, written (a) by one launch pair over all L rows and (b) by a launch pair over rows [0, past)
    followed by one over rows [past, L) at pos0 = p0 = past — what tests/test_gpu_prefix_reuse.py compares with each other.  The same fault goes into
    every launch.  Returns ((K, V^T) of (a), (K, V^T) of (b)) as int16 [nkv, ctx, hd] / [nkv, hd, ctx] restricted to positions < L."""
    case = dict(nq=nq, nkv=nkv, R=L, seq_len=L, slot0=0, pos0=0, nslots=1, ctx=ctx, table_rows=ctx)
    full = rope_probe("per-position", case, dtype, hd=hd)
    nh = nq + 2 * nkv

    def launches(cuts):
        kc = full.kcache.clone()
        vt = sentinel_buf(nkv * hd * ctx, dtype)
        for lo, hi in cuts:
            pr = SimpleNamespace(**vars(full))
            pr.R, pr.seq_len, pr.pos0 = hi - lo, hi - lo, lo
            pr.qkv = full.qkv.view(L, full.ld)[lo:hi].reshape(-1).clone()
            pr.kcache = kc
            _, kc, _ = emulate_rope(pr, rope_fault)
            v = pr.qkv.view(hi - lo, full.ld)[:, (nq + nkv) * hd:nh * hd].contiguous()
            tp = SimpleNamespace(hd=hd, p0=lo, n=hi - lo, perm=0, heads=nkv, batch=1, dtype=dtype, src=torch.cat([v.reshape(-1), sentinel_buf(64 * nkv * hd, dtype)]),
                                 src_bs=0, src_hs=hd, src_rs=nkv * hd, dst=vt, dst_bs=0, dst_hs=hd * ctx, dst_rs=ctx)
            vt = emulate_transpose(tp, transpose_fault).view(dtype)
        return bits(kc).view(nkv, ctx, hd)[:, :L].clone(), bits(vt).view(nkv, hd, ctx)[:, :, :L].clone()
    return launches([(0, L)]), launches([(0, past), (past, L)])
