"""Decode-step row kernels against float64: add_rmsnorm_kernel (with its e4m3 tail), swiglu_combine_kernel, quant_rows_fp8_kernel, and the two
fused prologues of skinny_lds_kernel (SkinnyPro: PRO == 1 sums + residual + RMSNorm, PRO == 2 SwiGLU), read back through a selection matrix.

  references   float64 with the rounding points the kernels document:
                 x      = el(el(sum_ks part) + R)                              (the GEMV epilogue's rounding, then the add)
                 y      = el(x rsqrt(mean(x^2) + eps) w)   from the DEVICE's x (encode_probes.norm_reference, rms=True)
                 y8, sy   from the DEVICE's y: sy = amax / 448 (1 for a zero row), code_i = rne_e4m3(y_i 448 / amax)
                 swiglu = el(silu(G) U), G and U the chunk sums
  one judge    x      bit equal on every probe whose chunk sums are exact in fp32 (all but `gaussian`); gaussian: half a 16-bit ulp of x + half a
                      16-bit ulp of the sum + E, E = KS 2^-24 sum_ks |part| per element
               y      encode_probes.bound: half a 16-bit ulp + 2^-15 |x rstd w|
               swiglu gemm_probes.act_bound, + one smallest normal of the element type where the gate is below -87 (fp32 exp(-g) overflows at
                      -88.7; bf16 still holds silu(-89) = -2.0e-37, 17 smallest normals, so the kernels must not flush it: decode.hip silu_mul)
               codes  one of the two e4m3 neighbours of the float64 value, and the nearest one unless that value is within 2^-22 (relative) of a
                      tie — the reciprocal's and the product's fp32 roundings.  Where the scaling is an exact power of two (code-table, tiny-row,
                      zero-row) no slack: the round-to-nearest-even code.  Subnormal codes follow the same rule.
               sy     within one fp32 ulp of the float64 quotient
  probes       small integers times powers of two, so every chunk sum is exact in fp32 whatever the order; the part buffers carry NaN in two chunks
               past KS and in the rows B .. SK_ROWS - 1 of every chunk
  emulations   fp32 torch restatements of the four kernels, each taking fault=<name>; tests/test_decode_row_probes_cpu.py shows which probe
               rejects which fault, and which faults the Gaussian tolerances of tests/test_gpu_kernels.py accept.

Runs on the CPU and on a device; nothing here imports the HIP library."""
from types import SimpleNamespace

import torch

import encode_probes as EP
import gemm_probes as GP
from gemm_probes import MIN_NORMAL, P_BITS, SENTINEL, round16

SK_ROWS = 256                        # trace_op_sk_rows(): the row stride of every partial-row buffer (the GPU tests assert it)
EXTRA_CHUNKS = 2                     # NaN chunks behind the KS the kernel is told to read
TIE_SLACK = 2.0 ** -22
TINY_GUARD = 2.0 ** -100             # rows with 0 < amax below this are scaled by 2^64 before the reciprocal (fp8.hip, decode.hip)
INF = float("inf")


def _idx(B, N, device):
    return (torch.arange(B, device=device, dtype=torch.int64)[:, None], torch.arange(N, device=device, dtype=torch.int64)[None, :])


# ---- e4m3fn in float64 --------------------------------------------------------------------------------------------------------------------------
def e4m3_values(device="cpu"):
    """the 127 finite magnitudes of codes 0 .. 126: subnormals m 2^-9, normals (1 + m / 8) 2^(e - 7), 448 the largest (code 127 is NaN)"""
    c = torch.arange(127, device=device, dtype=torch.int64)
    e, m = c >> 3, (c & 7).double()
    return torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * torch.exp2((e - 7).double()))


def e4m3_decode(codes):
    c = codes.to(torch.int64)
    mag = e4m3_values(codes.device)[(c & 0x7F).clamp(max=126)]
    mag = torch.where((c & 0x7F) == 127, torch.full_like(mag, float("nan")), mag)
    return torch.where((c & 0x80) != 0, -mag, mag)


def e4m3_round(v64, mode="rne"):
    """float64 -> e4m3fn codes (uint8): 3 mantissa bits, subnormal step 2^-9, saturation at 448, NaN -> 0x7F.  mode: rne | truncate | ties_away |
    subnormals_flushed (rne, results below 2^-6 become 0) | unclamped (rne, magnitudes above 448 become the NaN code)"""
    a = v64.abs()
    over = a > 448.0
    a = a.clamp(max=448.0)
    _, ex = torch.frexp(a)                                   # a = m 2^ex, m in [0.5, 1)
    step = torch.exp2(((ex - 1).clamp(min=-6) - 3).double())
    q = a / step
    q = torch.floor(q) if mode == "truncate" else torch.floor(q + 0.5) if mode == "ties_away" else torch.round(q)
    val = q * step
    if mode == "subnormals_flushed":
        val = torch.where(val < 2.0 ** -6, torch.zeros_like(val), val)
    code = torch.searchsorted(e4m3_values(v64.device), val.contiguous()).clamp(max=126)
    if mode == "unclamped":
        code = torch.where(over, torch.full_like(code, 127), code)
    code = torch.where(torch.isnan(v64), torch.full_like(code, 127), code)
    return (code + 128 * torch.signbit(v64).to(torch.int64)).to(torch.uint8)


def code_ratio_map(codes, v64, exact):
    """per element: 0 where the code is the nearest-even one; where it is the other neighbour, |v - tie| / (2^-22 |v|) (inf if `exact`); inf for
    anything else.  A zero may carry either sign."""
    got = codes.to(torch.int64)
    near = e4m3_round(v64).to(torch.int64)
    zero = v64 == 0
    ok = (got == near) | (zero & ((got & 0x7F) == 0))
    r = torch.where(ok, torch.zeros_like(v64), torch.full_like(v64, INF))
    if exact:
        return r
    tbl = e4m3_values(v64.device)
    a = v64.abs().clamp(max=448.0)
    hi = torch.searchsorted(tbl, a.contiguous()).clamp(max=126)
    lo = torch.where(tbl[hi] == a, hi, (hi - 1).clamp(min=0))
    nb = (((got & 0x7F) == lo) | ((got & 0x7F) == hi)) & ((got & 0x80) == 128 * torch.signbit(v64).to(torch.int64))
    tie = ((a - (tbl[lo] + tbl[hi]) / 2).abs() / (TIE_SLACK * a.clamp(min=1e-300)))
    return torch.where(ok, r, torch.where(nb, torch.nan_to_num(tie, nan=INF), r))


def quant_reference(y16):
    """(float64 values to be coded, float64 scales) of quant_rows_fp8's rule on the 16-bit rows y16"""
    y = y16.double()
    amax = y.abs().amax(-1)
    pos = amax > 0
    return y * torch.where(pos, 448.0 / amax.clamp(min=1e-300), torch.ones_like(amax))[:, None], torch.where(pos, amax / 448.0, torch.ones_like(amax))


def scale_ratio(sy, q64):
    """|sy - q| in fp32 ulps of q (subnormal quotients: the fixed step 2^-149)"""
    _, ex = torch.frexp(q64)
    ulp = torch.exp2(((ex - 1).clamp(min=-126) - 23).double())
    return float(torch.nan_to_num((sy.double() - q64).abs() / ulp, nan=INF).max())


def judge_quant(codes, sy, y16, exact=False):
    """{'codes', 'sy'}: error / bound of the e4m3 bytes and scales the device made of the 16-bit rows y16"""
    v, q = quant_reference(y16)
    return {"codes": float(code_ratio_map(codes, v, exact).max()), "sy": scale_ratio(sy, q)}


def near_tie_mask(y16):
    """elements whose float64 value y 448 / amax lies within 2^-22 (relative) of a tie between two e4m3 neighbours: the only ones on which two
    correctly rounding quantisers may differ"""
    v, _ = quant_reference(y16)
    tbl = e4m3_values(v.device)
    a = v.abs().clamp(max=448.0)
    hi = torch.searchsorted(tbl, a.contiguous()).clamp(max=126)
    lo = torch.where(tbl[hi] == a, hi, (hi - 1).clamp(min=0))
    return (lo != hi) & ((a - (tbl[lo] + tbl[hi]) / 2).abs() <= TIE_SLACK * a)


# ---- partial-row buffers ---------------------------------------------------------------------------------------------------------------------------
def lay_part(vals, extra=EXTRA_CHUNKS):
    """vals float64 [KS, B, N] (exact fp32 numbers) -> fp32 [KS + extra, SK_ROWS, N]: NaN in the chunks past KS and in the rows past B"""
    KS, B, N = vals.shape
    v32 = vals.float()
    assert bool((v32.double() == vals).all()), "partial rows are not exact fp32 numbers"
    part = torch.full((KS + extra, SK_ROWS, N), float("nan"), dtype=torch.float32, device=vals.device)
    part[:KS, :B] = v32
    return part


def split_over_chunks(x, KS, shift=0):
    """x float64 [B, N] -> [KS, B, N]: column n lives in chunk (n + shift) % KS alone"""
    n = torch.arange(x.shape[-1], device=x.device)
    k = torch.arange(KS, device=x.device)[:, None, None]
    return torch.where(((n + shift) % KS)[None, None, :] == k, x[None], torch.zeros((), dtype=x.dtype, device=x.device))


# ---- add_rmsnorm: probes ----------------------------------------------------------------------------------------------------------------------------
NORM_ROW_PROBES = ("onehot", "balanced", "eps", "ramp")
ADD_PROBES = ("chunk-pointer", "ties", "ties-up", "double-rounding") + tuple(f"{n}/R" for n in NORM_ROW_PROBES) + tuple(f"{n}/split" for n in NORM_ROW_PROBES) + \
    ("massive", "zero-row", "tiny-row", "gaussian")


def zero_row_of(B):
    return min(1, B - 1)


def add_probe(name, B, N, KS, dtype, device="cpu"):
    """-> vals float64 [KS, B, N] (lay_part makes the buffer), R / w in the element type, eps, exact (chunk sums exact in fp32 in any order)"""
    b, n = _idx(B, N, device)
    p = P_BITS[dtype]
    w = EP.ramp_weights(N, dtype, device)[0]
    eps, exact = 1e-5, True
    z = torch.zeros((B, N), dtype=torch.float64, device=device)
    k = torch.arange(KS, device=device, dtype=torch.int64)[:, None, None]
    if name == "chunk-pointer":                  # the value names (b, n); a column lives in chunk n % KS alone
        vals = split_over_chunks((1 + (n * 37 + b * 101) % 199).double(), KS)
        R = ((n + 2 * b) % 7 - 3).double()
    elif name == "ties":                         # sum = 2^p + odd: half-way between 16-bit neighbours of both parities; el(sum) + R (odd) half-way again
        rest = 2 * ((n * 5 + b * 3) % 2 ** (p - 1)) + 1
        sign = (1 - 2 * ((n // 3 + b) % 2)).double()
        share = (rest // KS)[None] + (k < (rest % KS)[None]).to(torch.int64)
        share[0] += 2 ** p
        vals = share.double() * sign[None]
        R = sign * torch.tensor([1.0, -1.0, 3.0, -3.0], dtype=torch.float64, device=device)[(n // 2 + b) % 4]
    elif name == "ties-up":                      # sums on the 16-bit grid (multiples of 4), R = -1 towards zero: el(sum) + R is a tie that rounds back UP in
        m4 = 2 ** p + 4 * (1 + (n * 5 + b * 3) % (2 ** (p - 2) - 1))     # magnitude on every element — a sum of squares of the unrounded x is low by 2 / |x|
        sign = (1 - 2 * ((n // 3 + b) % 2)).double()
        share = (m4 // (4 * KS))[None] * 4 + 4 * (k < ((m4 // 4) % KS)[None]).to(torch.int64)
        vals = share.double() * sign[None]
        R = -sign * torch.ones((B, N), dtype=torch.float64, device=device)
    elif name == "double-rounding":              # el(el(s) + R) != el(s + R) on every element
        i = (n * 3 + b) % (2 ** (p - 2) - 1)
        typ = (n + b) % 2
        M = 2 ** p + 4 * i + 2 * typ             # typ 0: s = M + 1 + 1/8, R = +1;  typ 1: s = M + 1 - 1/8, R = -1
        sign = (1 - 2 * ((n // 2 + b) % 2)).double()
        whole = (M + 1)[None].expand(KS, B, N).clone()
        if KS > 1:
            whole[1:] = 3
            whole[0] = M + 1 - 3 * (KS - 1)
        vals = whole.double()
        vals[KS - 1] += (1 - 2 * typ).double() / 8
        vals = vals * sign[None]
        R = sign * (1 - 2 * typ).double()
    elif name.split("/")[0] in NORM_ROW_PROBES:  # encode_probes.norm_rows as the residual alone, and split over the chunks
        kind, form = name.split("/")
        x = EP.norm_rows(kind, B, N, dtype, device).double()
        if kind == "eps":
            eps = 1e-6
        vals, R = (z[None].expand(KS, B, N).clone(), x) if form == "R" else (split_over_chunks(x, KS, 1), z)
    elif name == "massive":                      # 4 columns at 2^10 times the rest (the outlier dimensions of a residual stream)
        x = EP.norm_rows("ramp", B, N, dtype, device).double()
        hot = torch.zeros(N, dtype=torch.bool, device=device)
        hot[torch.tensor([1 % N, N // 3, (N // 2 + 1) % N, (N - 2) % N], device=device)] = True
        big = (x.abs() + 1) * 2.0 ** 10 * torch.where(x < 0, -1.0, 1.0)
        vals = split_over_chunks(torch.where(hot[None], big, z), KS, 2)
        R = torch.where(hot[None], z, x)
    elif name == "zero-row":                     # one all-zero row among ramp rows whose largest magnitude is negative
        x = EP.norm_rows("ramp", B, N, dtype, device).double()
        x[:, 0] = -16.0
        x[zero_row_of(B)] = 0.0
        vals, R = split_over_chunks(x, KS), torch.where(x == 0, z, ((n + b) % 3 - 1).double())
        R[zero_row_of(B)] = 0.0
    elif name == "tiny-row":                     # y = x rsqrt(eps) 2^-4 with x in {0, +-2^-126}: amax(y) = 2^-121.7, below 448 / FLT_MAX (bf16 only)
        assert dtype == torch.bfloat16
        x = ((n + b) % 3 - 1).double() * 2.0 ** -126
        x[:, 0] = 2.0 ** -126
        vals, R = z[None].expand(KS, B, N).clone(), x
        w = torch.full((N,), 2.0 ** -4, dtype=dtype, device=device)
    elif name == "gaussian":
        g = torch.Generator().manual_seed(B * 131 + N * 7 + KS)
        vals = (torch.randn((KS, B, N), generator=g) * 0.3).double().to(device)
        R = torch.randn((B, N), generator=g).to(dtype).double().to(device)
        w = (1 + 0.1 * torch.randn(N, generator=g)).to(dtype).to(device)
        exact = False
    else:
        raise ValueError(name)
    Rt = R.to(dtype)
    assert bool((Rt.double() == R).all()), f"{name}: the residual is not exact in the element type"
    return SimpleNamespace(name=name, vals=vals, R=Rt, w=w, eps=eps, exact=exact, B=B, N=N, KS=KS, dtype=dtype)


def x_reference(pr):
    """(reference, bound).  Exact probes: x in the element type, bound None — bit equality is asked.  gaussian: the UNROUNDED float64 sum + R, and
    half a 16-bit ulp of x + half a 16-bit ulp of the sum (the two roundings) + E (the fp32 chunk sum)."""
    s = pr.vals.sum(0)
    r = round16(s, pr.dtype, pr.exact)
    x = round16(r.double() + pr.R.double(), pr.dtype, pr.exact)
    if pr.exact:
        return x, None
    E = pr.KS * 2.0 ** -24 * pr.vals.abs().sum(0)
    return s + pr.R.double(), EP.half_ulp(x.double(), pr.dtype) + EP.half_ulp(r.double(), pr.dtype) + E


def x_ratio(x, pr):
    ref, bound = x_reference(pr)
    if bound is None:
        return 0.0 if bool((x.float() == ref.float()).all()) else INF
    return float(torch.nan_to_num((x.double() - ref.double()).abs() / bound, nan=INF).max())


def y_ratio(y, x, pr):
    """y against the float64 RMSNorm of the device's own x"""
    return EP.error_ratio(y, EP.norm_reference(x, pr.w, None, pr.eps, pr.dtype, rms=True))


def judge_add(pr, x, y, y8=None, sy=None):
    out = {"x": x_ratio(x, pr), "y": y_ratio(y, x, pr)}
    if y8 is not None:
        out.update(judge_quant(y8, sy, y))
    return out


def ulps16_apart(a, b):
    """largest distance of two 16-bit tensors in units of the last place (sign-magnitude order; inf for a NaN)"""
    if bool(torch.isnan(a.float()).any()) or bool(torch.isnan(b.float()).any()):
        return INF
    ia, ib = a.view(torch.int16).to(torch.int64), b.view(torch.int16).to(torch.int64)
    ia, ib = torch.where(ia < 0, -(ia & 0x7FFF), ia), torch.where(ib < 0, -(ib & 0x7FFF), ib)
    return float((ia - ib).abs().max())


# ---- add_rmsnorm: the covering set of shapes ---------------------------------------------------------------------------------------------------------
ADD_N, ADD_B, ADD_KS = (4, 252, 1024, 4092, 4096), (1, 3, 64, 65, 256), (1, 7, 8, 9, 16, 17)


def add_cases():
    """every value of each axis with the extremes of the other two (48 of the 150 combinations), each with the probes it runs: chunk-pointer
    everywhere, the others in rotation, gaussian where KS == 17"""
    cases = []
    ext = lambda ax: (ax[0], ax[-1])
    for N in ADD_N:
        for B in ADD_B:
            for KS in ADD_KS:
                if sum((N in ext(ADD_N), B in ext(ADD_B), KS in ext(ADD_KS))) >= 2:
                    cases.append((N, B, KS))
    rot = [p for p in ADD_PROBES if p not in ("chunk-pointer", "gaussian", "tiny-row")]
    out = []
    for i, (N, B, KS) in enumerate(cases):
        probes = ["chunk-pointer", rot[(2 * i) % len(rot)], rot[(2 * i + 1) % len(rot)]]
        if KS == 17:
            probes.append("gaussian")
        if i % 6 == 0:
            probes.append("tiny-row")
        out.append((N, B, KS, tuple(probes)))
    return out


# ---- add_rmsnorm: emulation ----------------------------------------------------------------------------------------------------------------------------
ADD_FAULTS = ("chunk_tail_dropped", "chunk_stride_is_B", "inner_rounding_skipped", "stats_from_unrounded_x", "mean_over_4096", "eps_dropped",
              "idle_threads_counted", "ldr_ignored", "ldx_ignored", "ldy_ignored", "amax_from_unrounded_y", "zero_row_scale_0")
QUANT_FAULTS = ("truncate", "ties_away", "subnormals_flushed", "amax_without_abs", "scale_of_unclamped", "reciprocal_unguarded")


def _quant_f32(v, am, fault=None):
    """the shared tail of quant_rows_fp8_kernel and add_rmsnorm_kernel in fp32: v [rows, K] fp32 (16-bit values), am [rows] -> (codes, scales).
    Rows with 0 < amax < 2^-100 are scaled by 2^64 first, so that 448 / amax stays finite (fault reciprocal_unguarded: they are not)."""
    pos = am > 0
    pre = torch.where(pos & (am < TINY_GUARD) & (fault != "reciprocal_unguarded"), torch.full_like(am, 2.0 ** 64), torch.ones_like(am))
    inv = torch.where(pos, 448.0 / (am * pre), torch.ones_like(am))
    f = v * pre[:, None] * inv[:, None]
    if fault != "scale_of_unclamped":           # fminf(fmaxf(f, -448), 448): a NaN leaves the pair as -448
        f = torch.where(torch.isnan(f), torch.full_like(f, -448.0), f.clamp(-448.0, 448.0))
    mode = fault if fault in ("truncate", "ties_away", "subnormals_flushed") else "unclamped" if fault == "scale_of_unclamped" else "rne"
    return e4m3_round(f.double(), mode), torch.where(pos, am / 448.0, torch.full_like(am, 0.0 if fault == "zero_row_scale_0" else 1.0))


def emulate_quant(x16, fault=None):
    """quant_rows_fp8_kernel.  scale_of_unclamped: the clamp to +-448 is missing, a product that the reciprocal's last bit (or an overflow) takes
    past 448 becomes the NaN code.  amax_without_abs: the row maximum of x instead of |x|."""
    v = x16.float()
    am = v.amax(-1).clamp(min=0) if fault == "amax_without_abs" else v.abs().amax(-1)
    return _quant_f32(v, am, fault)


def emulate_add_rmsnorm(part, KS, Rb, ldr, xb, ldx, w, yb, ldy, B, N, eps, dtype, fp8=False, fault=None):
    """add_rmsnorm_kernel in fp32 torch on flat 16-bit buffers (windows at element 0; xb may be Rb): chunks summed in chunk order, eight at a time.
    Writes xb / yb, returns (codes, scales) or (None, None).  idle_threads_counted: the threads past N / 4 (N < 4096) add what follows the
    residual row in memory to the sum of squares."""
    lr, lx, ly = (N if fault == "ldr_ignored" else ldr), (N if fault == "ldx_ignored" else ldx), (N if fault == "ldy_ignored" else ldy)
    flat = part.reshape(-1)
    stride = (B if fault == "chunk_stride_is_B" else SK_ROWS) * N
    ks_read = KS - KS % 8 if fault == "chunk_tail_dropped" else KS
    a = torch.zeros((B, N), dtype=torch.float32, device=part.device)
    for k in range(ks_read):
        a = a + flat.as_strided((B, N), (N, 1), k * stride)
    Rflat = Rb.reshape(-1)
    R = Rflat.as_strided((B, N), (lr, 1), 0).float().clone()
    x32 = (a if fault == "inner_rounding_skipped" else a.to(dtype).float()) + R
    x = x32.to(dtype)
    v = x.float()
    sv = x32 if fault == "stats_from_unrounded_x" else v
    ss = (sv * sv).sum(-1, keepdim=True)
    if fault == "idle_threads_counted" and N < 4096:
        padded = torch.cat([Rflat.float(), torch.zeros(4096, device=part.device)])
        tail = padded.as_strided((B, 4096 - N), (lr, 1), N)
        ss = ss + (tail * tail).sum(-1, keepdim=True)
    rstd = torch.rsqrt(ss / (4096.0 if fault == "mean_over_4096" else float(N)) + (0.0 if fault == "eps_dropped" else eps))
    o = v * rstd * w.float()
    y = o.to(dtype)
    xb.reshape(-1).as_strided((B, N), (lx, 1), 0).copy_(x)
    yb.reshape(-1).as_strided((B, N), (ly, 1), 0).copy_(y)
    if not fp8:
        return None, None
    am = (o if fault == "amax_from_unrounded_y" else y.float()).abs().amax(-1)
    return _quant_f32(y.float(), am, fault)


def lay16(x, pad, fill):
    """x [rows, D] -> (flat buffer, window, ld): rows every D + pad elements, 2 guard rows; the rest holds `fill` (a number, or "sentinel")"""
    return EP.lay_rows(x, pad, x.dtype, fill, after=2)


def run_add(pr, fn, form, fp8):
    """one probe through `fn(pr, part, L, fp8) -> (y8, sy)` (a kernel call or an emulation; L: the buffers Rb / xb / yb, their windows Rv / xv / yv
    and row strides ldr / ldx / ldy).
    form 'pad': out of place, every row stride padded by a different amount, poison beside the residual rows, sentinel beside the outputs;
    form 'inplace': xout == R, all strides N (the decode step's call).  Returns (ratios, intact)."""
    part = lay_part(pr.vals)
    if form == "pad":
        Rb, Rv, ldr = lay16(pr.R, 12, EP.POISON)
        xb, xv, ldx = lay16(torch.zeros_like(pr.R), 4, "sentinel")
        yb, yv, ldy = lay16(torch.zeros_like(pr.R), 8, "sentinel")
    else:
        Rb, Rv, ldr = lay16(pr.R, 0, EP.POISON)
        xb, xv, ldx = Rb, Rv, ldr
        yb, yv, ldy = lay16(torch.zeros_like(pr.R), 0, "sentinel")
    snaps = [t.clone() for t in (Rb, xb, yb)]
    y8, sy = fn(pr, part, SimpleNamespace(Rb=Rb, Rv=Rv, ldr=ldr, xb=xb, xv=xv, ldx=ldx, yb=yb, yv=yv, ldy=ldy), fp8)
    ratios = judge_add(pr, xv, yv, y8, sy)
    intact = EP.outside_unchanged(xb, snaps[1], ldx, pr.B, pr.N) and EP.outside_unchanged(yb, snaps[2], ldy, pr.B, pr.N)
    if form == "pad":
        intact = intact and torch.equal(Rb.view(torch.int16), snaps[0].view(torch.int16))
    if pr.name == "zero-row":
        zb = zero_row_of(pr.B)
        zero = bool((yv[zb].float() == 0).all()) and (y8 is None or (bool(((y8[zb] & 0x7F) == 0).all()) and float(sy[zb]) == 1.0))
        ratios["zero-row"] = 0.0 if zero else INF
    return ratios, intact


# ---- quantiser: probes ------------------------------------------------------------------------------------------------------------------------------
QUANT_PROBES = ("code-table", "tiny-row", "zero-row", "last-ulp")
TABLE_SHIFTS = {torch.bfloat16: (0, 20, -60, -4), torch.float16: (0, -2, -4, -1)}       # row r holds the table times 2^-shift: 448 / amax = 2^shift exactly


def code_table_values(dtype, device="cpu"):
    """every e4m3 magnitude, every midpoint between neighbours and the midpoints +- one 16-bit ulp, both signs, and zero: all exact in the element
    type (a midpoint has 5 significant bits), 448 first"""
    t = e4m3_values(device)
    mid = (t[1:] + t[:-1]) / 2
    ulp = 2 * EP.half_ulp(mid, dtype)
    mag = torch.cat([t.flip(0), mid, mid + ulp, mid - ulp])
    return torch.cat([mag, -mag])


def quant_probe(name, K, dtype, device="cpu"):
    """-> x [rows, K] in the element type"""
    if name == "code-table":
        tv = code_table_values(dtype, device)
        per = K - 1                                           # element 0 of every row is 448 2^-shift and pins amax
        chunks = -(-tv.numel() // per)
        rows = []
        for r in range(max(chunks, len(TABLE_SHIFTS[dtype]))):
            seg = tv[torch.arange(r * per, (r + 1) * per, device=device) % tv.numel()]
            rows.append(torch.cat([torch.full((1,), 448.0, dtype=torch.float64, device=device), seg]) * 2.0 ** -TABLE_SHIFTS[dtype][r % 4])
        x = torch.stack(rows)
    elif name in ("tiny-row", "zero-row"):
        b, n = _idx(5, K, device)
        x = EP.norm_rows("ramp", 5, K, dtype, device).double()
        x[:, 0] = -16.0                                       # the largest magnitude of a neighbour row is negative; 448 / 16 = 28: not a power of two
        if name == "tiny-row":                                # amax = 2^-121 (fp16: its smallest subnormal), zeros and +-amax
            am = 2.0 ** -121 if dtype == torch.bfloat16 else 2.0 ** -24
            x[1] = (((n + 1) % 3) - 1).double()[0] * am
            x[3] = -x[1]
        else:
            x[1] = 0.0
    elif name == "last-ulp":                                  # amax whose fp32 product amax * fl(448 / amax) exceeds 448: the clamp's case
        m = torch.arange(128, 256, dtype=torch.float32)
        over = m[(m * (torch.tensor(448.0) / m)) > 448.0]
        assert over.numel() > 0
        b, n = _idx(int(over.numel()), K, device)
        x = (over.double().to(device)[:, None] / 64) * torch.where(n % 2 == 0, 1.0, -0.5)
    else:
        raise ValueError(name)
    xt = x.to(dtype)
    assert bool((xt.double() == x).all()), f"{name}: not exact in the element type"
    return xt


def judge_quant_probe(name, x, codes, sy):
    """ratios of one quantiser probe; tiny-row and zero-row name the rows they are about"""
    exact = name == "code-table"
    out = judge_quant(codes, sy, x, exact)
    if name in ("tiny-row", "zero-row"):
        rows = [1, 3] if name == "tiny-row" else [1]
        out[name] = judge_quant(codes[rows], sy[rows], x[rows], True)["codes"]
        if name == "zero-row":
            out[name] = out[name] if float(sy[1]) == 1.0 and bool((codes[1] == 0).all()) else INF
    return out


# ---- swiglu: probes, reference, emulation ------------------------------------------------------------------------------------------------------------
SWIGLU_PROBES = ("chunk-pointer", "gate-range", "gaussian")
SWIGLU_FAULTS = ("gate_up_swapped", "interleave_8_not_16", "chunk_tail_dropped", "silu_of_rounded_gate", "chunk_stride_is_B", "exp_overflow_unguarded")
GATES = (0.0, 2.0 ** -20, -2.0 ** -20, 1.0, -1.0, 16.0, -16.0, 87.0, -87.0, 89.0, -89.0, 128.0, -128.0)


def interleave(G, U):
    """gate / up [.., I] -> the 16-row interleaved columns [.., 2 I]: [32 p, 32 p + 16) gate, [32 p + 16, 32 p + 32) up of outputs [16 p, 16 p + 16)"""
    s = G.shape[:-1]
    return torch.stack([G.reshape(*s, -1, 16), U.reshape(*s, -1, 16)], dim=-2).reshape(*s, -1)


def swiglu_probe(name, B, N2, KS, dtype, device="cpu"):
    I = N2 // 2
    b, j = _idx(B, I, device)
    exact = True
    if name == "chunk-pointer":      # gate = a coarse and a fine term in two different chunks (not a 16-bit number), up in a third
        G = split_over_chunks(((j * 5 + b * 3) % 33 - 16).double() / 4, KS) + split_over_chunks(((j + b) % 7 - 3).double() * 2.0 ** -12, KS, 1)
        U = split_over_chunks(((j * 7 + b) % 13 - 6).double(), KS, 2)
    elif name == "gate-range":       # every gate of GATES against up = +1, -1, 0
        g = torch.tensor(GATES, dtype=torch.float64, device=device)[(j + b) % len(GATES)]
        u = (((j + b) // len(GATES)) % 3 - 1).double()
        G, U = split_over_chunks(g, KS), split_over_chunks(u, KS, 1)
    elif name == "gaussian":
        gen = torch.Generator().manual_seed(B * 17 + N2 + KS)
        G = (torch.randn((KS, B, I), generator=gen) * 1.5).double().to(device)
        U = torch.randn((KS, B, I), generator=gen).double().to(device)
        exact = False
    else:
        raise ValueError(name)
    Gs, Us = G.sum(0), U.sum(0)
    if not exact:                    # the sums as documented: fp32, in chunk order (every other probe's sums are exact in any order)
        Gs, Us = torch.zeros((B, I), dtype=torch.float32, device=device), torch.zeros((B, I), dtype=torch.float32, device=device)
        for k in range(KS):
            Gs, Us = Gs + G[k].float(), Us + U[k].float()
        Gs, Us = Gs.double(), Us.double()
    return SimpleNamespace(name=name, vals=interleave(G, U), G=Gs, U=Us, B=B, N2=N2, KS=KS, dtype=dtype, exact=exact)


def swiglu_reference(pr):
    """(float64 silu(G) U, bound): gemm_probes.act_bound, + one smallest normal where the gate is below -87 (fp32 exp overflows there)"""
    pre = pr.G / (1 + torch.exp(-pr.G)) * pr.U
    return pre, GP.act_bound(pre, pr.dtype) + torch.where(pr.G < -87, MIN_NORMAL[pr.dtype], 0.0)


def swiglu_ratio_map(got, pr):
    pre, bound = swiglu_reference(pr)
    return torch.nan_to_num((got.double() - pre).abs() / bound, nan=INF)


def swiglu_ratio(got, pr):
    return float(swiglu_ratio_map(got, pr).max())


def emulate_swiglu(part, KS, B, N2, dtype, fault=None):
    """swiglu_combine_kernel (and the SwiGLU prologue, which restates it) in fp32 torch: chunk order, silu(g) u = g / (1 + exp(-g)) u, one rounding.
    Where exp(-g) is inf in fp32 (g < -88.7) the kernels take g e^(g + 64) e^-64 u instead of the quotient's -0 (decode.hip silu_mul; fault
    exp_overflow_unguarded: they do not — bf16 still holds silu(-89) = -2e-37)."""
    flat = part.reshape(-1)
    stride = (B if fault == "chunk_stride_is_B" else SK_ROWS) * N2
    ks_read = KS - KS % 4 if fault == "chunk_tail_dropped" else KS
    a = torch.zeros((B, N2), dtype=torch.float32, device=part.device)
    for k in range(ks_read):
        a = a + flat.as_strided((B, N2), (N2, 1), k * stride)
    w = 8 if fault == "interleave_8_not_16" else 16
    v = a.reshape(B, -1, 2, w)
    g, u = v[:, :, 0].reshape(B, -1), v[:, :, 1].reshape(B, -1)
    if fault == "gate_up_swapped":
        g, u = u, g
    if fault == "silu_of_rounded_gate":
        g = g.to(dtype).float()
    e = torch.exp(-g)
    o = g / (1 + e) * u
    if fault != "exp_overflow_unguarded":
        o = torch.where(torch.isinf(e), g * torch.exp(g + 64.0) * 1.6038109e-28 * u, o)
    return o.to(dtype)


# ---- the fused GEMVs: selection matrix, emulation --------------------------------------------------------------------------------------------------------
def sel_of(N, K, offset=0, device="cpu"):
    """the k that output column n reads: a fixed bijection of [0, K) walked from `offset` (37 is coprime to every K used)"""
    n = torch.arange(N, device=device, dtype=torch.int64)
    return ((n + offset) * 37 + 11) % K


def selection_matrix(N, K, dtype, offset=0, device="cpu"):
    """W [N, K]: W[n][sel(n)] = 2^(n % 3), zero elsewhere — every output column is one parked activation times a power of two, exactly"""
    W = torch.zeros((N, K), dtype=dtype, device=device)
    n = torch.arange(N, device=device, dtype=torch.int64)
    W[n, sel_of(N, K, offset, device)] = torch.exp2((n % 3).double()).to(dtype)
    return W


def read_parked(out, B, N, K, chunk_units, offset=0):
    """out fp32 [ks, SK_ROWS, N] of a selection-matrix GEMV -> (parked [B, K] fp32 with NaN where no column looked, looked [K] bool,
    ok: every chunk but the one that owns sel(n) holds exactly zero in column n, and columns that read the same k (N > K) agree)"""
    dev = out.device
    sel = sel_of(N, K, offset, dev)
    n = torch.arange(N, device=dev, dtype=torch.int64)
    owner = (sel // 64) // chunk_units
    o = out[:, :B]                                                           # [ks, B, N]
    own = torch.arange(o.shape[0], device=dev)[:, None] == owner[None, :]    # [ks, N]
    zeros_ok = bool((torch.where(own[:, None, :], torch.zeros_like(o), o) == 0).all())
    val = o.sum(0) / torch.exp2((n % 3).float())[None, :]
    parked = torch.full((B, K), float("nan"), dtype=torch.float32, device=dev)
    parked[:, sel] = val
    looked = torch.zeros(K, dtype=torch.bool, device=dev)
    looked[sel] = True
    return parked, looked, zeros_ok and torch.equal(parked[:, sel], val)


def offsets_covering(N, K):
    """selection offsets after which every k has been read by some column"""
    return [i * N for i in range(-(-K // N))]


FUSED_NORM_FAULTS = ("stats_over_own_chunk", "half_swapped", "unit_shifted", "xout_from_every_row_group_with_stale_R", "xout_missing_last_chunk")


def emulate_fused_norm(part, ks_in, R, w, eps, dtype, KS_out, chunk_units, fault=None):
    """the RMSNorm prologue of skinny_lds_kernel: every workgroup (output chunk c of KS_out, units [c cu, (c + 1) cu) of 64 k) redoes the row's sum,
    parks ITS chunk of y and, as row-group 0, writes its share of xout.  -> (xout [B, K] with the sentinel where nothing was written, parked
    [B, K]).  stats_over_own_chunk: sum and mean of the squares run over the workgroup's own chunk.  half_swapped: the two 8-element
    halves of every 16 are parked in each other's place.  unit_shifted: a chunk's 64-k units are parked one unit late (rotating).
    xout_from_every_row_group_with_stale_R: a later row group adds the partial sums to the xout the first one stored (xout aliasing R)."""
    B, K = R.shape
    a = torch.zeros((B, K), dtype=torch.float32, device=R.device)
    for k in range(ks_in):
        a = a + part[k, :B]
    x = (a.to(dtype).float() + R.float()).to(dtype) if ks_in > 0 else R.clone()
    v = x.float()
    xout = torch.zeros_like(x)
    xout.view(torch.int16).fill_(SENTINEL)
    parked = torch.zeros((B, K), dtype=dtype, device=R.device)
    for c in range(KS_out):
        k0, k1 = c * chunk_units * 64, min(K, (c + 1) * chunk_units * 64)
        if k0 >= k1:
            continue
        sv = v[:, k0:k1] if fault == "stats_over_own_chunk" else v
        rstd = torch.rsqrt((sv * sv).sum(-1, keepdim=True) / float(sv.shape[1]) + eps)
        y = (v[:, k0:k1] * rstd * w.float()[k0:k1]).to(dtype)
        if fault == "half_swapped":
            y = y.reshape(B, -1, 2, 8).flip(2).reshape(B, -1)
        if fault == "unit_shifted":
            y = y.reshape(B, -1, 64).roll(1, 1).reshape(B, -1)
        parked[:, k0:k1] = y
        if not (fault == "xout_missing_last_chunk" and c == KS_out - 1):
            xout[:, k0:k1] = x[:, k0:k1]
    if fault == "xout_from_every_row_group_with_stale_R" and ks_in > 0:
        xout = (a.to(dtype).float() + x.float()).to(dtype)
    return xout, parked
