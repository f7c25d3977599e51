"""GEMM probes: inputs whose product is an exact integer whatever the order of the sums, a float64 reference with the documented roundings,
and buffers with strides, base offsets, poison and guard rows.

Gaussian operands hide most of what a hand-scheduled GEMM gets wrong: a lost product moves a sum of K random terms by one term, and a
tolerance of 2e-2 + 1e-2 |ref| stops noticing it once K is a few hundred; a truncating store or a residual added before the rounding is
always inside it.  Here every operand is a small integer (times a power of two), so every product and every partial sum is an exact fp32
value in any order: the result does not depend on tile shape, split, ring depth or MFMA k-slot order, and the expected output is the float64
product put through the documented roundings — bit for bit, for every kernel variant.

  pointer-A   A rows one-hot at k(m), W an integer table T[n][k] with distinct rows and columns: C[m, n] = T[n][k(m)].  The k(m) of one launch cover
              every k (a row carries ceil(K / M) ones when M < K: its outputs are the sums of that many table entries, still exact)
  pointer-W   the roles swapped (W rows one-hot, A / X the table): the form for the decode GEMVs, which have at most 64 rows
  hadamard    every 64-k tile of an A row / a W row is a (signed) row of the +-1 Hadamard matrix of order 64, the row index a function of
              (m, tile) / (n, tile): every tile contributes 0 or +-64, most outputs are exactly 0 although all K products are non-zero
  count       A = 1, W = 1 except one zero per 64-k tile at a place that depends on (n, tile): C = 63 K / 64, whose partial sums outgrow 16 bits
  ties        pointer-A plus an even integer bias in [2^p, 2^(p+1)): lin + bias lands on exact rounding ties where T is odd; an integer residual
              in [-3, 3] then pins the order "round, then add R"

Everything is parameterised by the element type (bf16: p = 8 significand bits, fp16: p = 11) and runs on the CPU as well as on a device;
nothing here imports the HIP library."""
import math
from types import SimpleNamespace

import torch

EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU = 0, 1, 2, 3
EPI_NAMES = {EPI_NONE: "none", EPI_RESIDUAL: "residual", EPI_QUICKGELU: "quickgelu", EPI_SWIGLU: "swiglu"}
P_BITS = {torch.bfloat16: 8, torch.float16: 11}
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
POISON = 2.0 ** 14                # pad columns of A and W, rows past M, guard rows: large, finite, exact in bf16 / fp16
SENTINEL = 0x4B5A                 # the 16-bit pattern C is pre-filled with (a finite value in both element types)
ACT_RTOL_SLACK = 2.0 ** -15       # the fp32 exp2 / rcp chain of the activation epilogues (a few 2^-23) and the product, over one output rounding
FP8 = torch.float8_e4m3fn


def act_bound(pre64, dtype, literal=False):
    """What an activation epilogue's output may be off by: ONE output rounding plus slack for the fp32 exp2 / rcp chain.  One round-to-nearest is at
    most half a unit in the last place, 2^(floor(log2 |ref|) - p): between 2^-(p+1) |ref| (just below a power of two) and 2^-p |ref| (just above one).
    The bound is therefore half an ulp of ref + 2^-15 |ref|, with a floor of one subnormal step.  `literal`: the flat (2^-(p+1) + 2^-15) |ref| — the
    lower end of that range; the correctly rounded reference itself exceeds it by up to 1.97 x (tests/test_gemm_probes_cpu.py shows it), so it is only
    reported next to the margins, not asserted."""
    p = P_BITS[dtype]
    a = pre64.abs()
    if literal:
        b = (2.0 ** -(p + 1) + ACT_RTOL_SLACK) * a
    else:
        half_ulp = torch.exp2(torch.floor(torch.log2(a.clamp(min=MIN_NORMAL[dtype]))) - p)
        b = half_ulp + ACT_RTOL_SLACK * a
    return torch.clamp(b, min=subnormal_step(dtype))


def subnormal_step(dtype):
    return MIN_NORMAL[dtype] * 2.0 ** -(P_BITS[dtype] - 1)


# ---- rounding -----------------------------------------------------------------------------------------------------------------------------
def round16(x, dtype, exact=True):
    """float64 -> the element type, round to nearest even.  torch converts through fp32; `exact` asserts that this first step changed nothing (true of
    every integer probe: |x| < 2^24), so the conversion is ONE rounding.  exact=False (the activation epilogues): the double rounding moves a result
    only where the float64 value is within 2^-24 relative of a tie, far inside their tolerance."""
    x32 = x.to(torch.float32)
    if exact:
        assert bool((x32.double() == x).all()), "the pre-rounding value is not an exact fp32 number"
    return x32.to(dtype)


def truncate16(x, dtype):
    """float64 (exact in fp32) -> the element type by dropping the low bits (round toward zero): what a store without rounding would do"""
    x32 = x.to(torch.float32)
    if dtype == torch.bfloat16:
        return (x32.view(torch.int32) & ~0xFFFF).view(torch.float32).to(dtype)
    r = x32.to(dtype)
    over = r.double().abs() > x.abs()
    return torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)      # one step toward zero = the bit pattern minus one, either sign


def significant_bits(x):
    """bits between the highest and the lowest set bit of |x| (x: integer-valued float64 / int64); 0 for 0"""
    v = x.to(torch.int64).abs()
    low = v & -v
    out = torch.zeros_like(v)
    nz = v > 0
    out[nz] = (torch.log2((v[nz] // low[nz]).double()).floor() + 1).to(torch.int64)
    return out


def pm1_visible(ref64, dtype):
    """fraction of outputs on which an error of +-1 in the exact sum changes the stored 16-bit value"""
    a = round16(ref64, dtype)
    return float(((round16(ref64 + 1, dtype) != a) & (round16(ref64 - 1, dtype) != a)).double().mean())


# ---- tables -------------------------------------------------------------------------------------------------------------------------------
def table(N, K, amp, device="cpu"):
    """integer table T[n][k] in [-amp, amp], 2 amp + 1 prime (257, 31).  With the base-(2 amp + 1) digits n = (n0, n1, n2), k = (k0, k1, k2):
    T = n0 k0 + n0^2 k1 + n0^3 k2 + n1 k0^2 + n2 k0^3 + 3 n0 + 5 k0 (mod 2 amp + 1) — a column is a cubic in n0 whose coefficients spell k, a row a cubic
    in k0 whose coefficients spell n, and two different cubics over a prime field agree in at most 3 places: rows and columns are all distinct
    (N, K >= 4; asserted by the CPU tests)."""
    p = 2 * amp + 1
    n = torch.arange(N, device=device, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=device, dtype=torch.int64)[None, :]
    n0, n1, n2 = n % p, (n // p) % p, n // (p * p)
    k0, k1, k2 = k % p, (k // p) % p, k // (p * p)
    return ((n0 * k0 + n0 * n0 * k1 + n0 * n0 * n0 * k2 + n1 * k0 * k0 + n2 * k0 * k0 * k0 + 3 * n0 + 5 * k0) % p - amp).double()


def hadamard64(device="cpu"):
    i = torch.arange(64, device=device, dtype=torch.int64)
    x = i[:, None] & i[None, :]
    par = torch.zeros_like(x)
    for b in range(6):
        par ^= (x >> b) & 1
    return (1 - 2 * par).double()


def k_of(M, K, device="cpu"):
    """hot columns of pointer-A: [M, h] with h = ceil(K / M) (entries >= K, when M does not divide K, are marked -1).  Row m is hot at
    perm(m + j M): every k of K is hit by exactly one row when M <= K; for M > K, k(m) = perm(m mod K)."""
    h = max(1, -(-K // M))
    m = torch.arange(M, device=device, dtype=torch.int64)[:, None]
    j = torch.arange(h, device=device, dtype=torch.int64)[None, :]
    raw = m + j * M
    ok = (raw < K) | (j == 0)
    k = ((raw % K) * 37 + 11) % K                 # 37 is coprime to every K used (multiples of 64): a bijection that separates row index and k-slot
    return torch.where(ok, k, torch.full_like(k, -1))


def _probe(name, A, W, dtype, bias=None, R=None, fp8=False, scale=0, **extra):
    """operands as the kernel gets them: A [M, K], W [N, K], bias [N], R [M, N] in the element type (fp8: A, W as e4m3 bytes; bias None).
    `scale`: W was multiplied by 2^-scale (exact) to bring the pre-activations of quickgelu / swiglu into the range where they are not saturated."""
    el = (lambda t: (t * 2.0 ** -scale).float().to(FP8).view(torch.uint8)) if fp8 else (lambda t: (t * 2.0 ** -scale).to(dtype))
    a = A.float().to(FP8).view(torch.uint8) if fp8 else A.to(dtype)
    w = el(W)
    assert bool((widen(a, fp8) == A).all()) and bool((widen(w, fp8) == W * 2.0 ** -scale).all()), f"{name}: operands not exact in the element type"
    return SimpleNamespace(name=name, A=a, W=w, bias=None if bias is None else bias.to(dtype), R=None if R is None else R.to(dtype), dtype=dtype,
                           fp8=fp8, M=A.shape[0], N=W.shape[0], K=A.shape[1], **extra)


def widen(t, fp8=False):
    return (t.view(FP8) if fp8 else t).double()


def small_bias(N, device="cpu"):
    return ((torch.arange(N, device=device, dtype=torch.int64) * 7) % 13 - 6).double()


def small_residual(M, N, device="cpu"):
    m = torch.arange(M, device=device, dtype=torch.int64)[:, None]
    n = torch.arange(N, device=device, dtype=torch.int64)[None, :]
    return ((3 * m + 5 * n + (m * n) // 7) % 7 - 3).double()


# ---- probes -------------------------------------------------------------------------------------------------------------------------------
def pointer_a(M, N, K, dtype, device="cpu", fp8=False, scale=0, bias=True):
    """C[m, n] = sum over the hot k of row m of T[n][k] (one k when M >= K).  Property: T's rows and columns are distinct, the hot k of all rows
    cover [0, K): a lost, doubled or permuted k-slot, a wrong row or column is a wrong integer."""
    ks = k_of(M, K, device)
    A = torch.zeros((M, K), dtype=torch.float64, device=device)
    rows = torch.arange(M, device=device)[:, None].expand_as(ks)
    A[rows[ks >= 0], ks[ks >= 0]] = 1.0
    T = table(N, K, 15 if fp8 else 128, device)
    return _probe("pointer-A", A, T, dtype, None if fp8 or not bias else small_bias(N, device), small_residual(M, N, device), fp8, scale, hot=ks, T=T)


def pointer_w(M, N, K, dtype, device="cpu", fp8=False, scale=0):
    """W rows one-hot (k_of with the roles swapped), A = the table: C[m, n] = sum over the hot k of row n of T[m][k]"""
    ks = k_of(N, K, device)
    W = torch.zeros((N, K), dtype=torch.float64, device=device)
    rows = torch.arange(N, device=device)[:, None].expand_as(ks)
    W[rows[ks >= 0], ks[ks >= 0]] = 1.0
    T = table(M, K, 15 if fp8 else 128, device)
    return _probe("pointer-W", T, W, dtype, None, small_residual(M, N, device), fp8, scale, hot=ks, T=T)


def hadamard_rows(rows, K, mul, tmul, signed, device="cpu"):
    H = hadamard64(device)
    r = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    t = torch.arange(K // 64, device=device, dtype=torch.int64)[None, :]
    X = H[(mul * r + tmul * t) % 64]                                     # [rows, K/64, 64]
    if signed:
        X = X * (1 - 2 * (((r >> 1) + t) & 1)).double()[:, :, None]
    return X.reshape(rows, K)


def hadamard(M, N, K, dtype, device="cpu", fp8=False, scale=0):
    """tile t of A row m is +-H[(7m + 3t) mod 64], of W row n H[(5n + 11t) mod 64]: a tile contributes +-64 where the two indices agree and 0
    elsewhere.  Properties: partial sums are multiples of 64 below 2^24 (exact in fp32), every output has at most p significant bits, and at
    least 85 % of the outputs are small enough that +-1 changes the stored value."""
    assert K % 64 == 0
    A, W = hadamard_rows(M, K, 7, 3, True, device), hadamard_rows(N, K, 5, 11, False, device)
    return _probe("hadamard", A, W, dtype, None if fp8 else small_bias(N, device), small_residual(M, N, device), fp8, scale)


def count_holes(M, N, K, dtype, device="cpu", fp8=False, scale=0):
    """C = 63 K / 64 for every output: the partial sums run through every multiple of 63, far more than 16 bits hold"""
    assert K % 64 == 0
    A = torch.ones((M, K), dtype=torch.float64, device=device)
    W = torch.ones((N, K // 64, 64), dtype=torch.float64, device=device)
    n = torch.arange(N, device=device, dtype=torch.int64)[:, None]
    t = torch.arange(K // 64, device=device, dtype=torch.int64)[None, :]
    W.scatter_(2, ((13 * n + 7 * t) % 64)[:, :, None], 0.0)
    return _probe("count", A, W.reshape(N, K), dtype, None, small_residual(M, N, device), fp8, scale)


def ties(M, N, K, dtype, device="cpu", scale=0):
    """pointer-A + an even integer bias in [2^p, 2^(p+1)) (the 16-bit grid there has spacing 2: an odd lin + bias is an exact tie) + an integer
    residual in [-3, 3] (rounded sum + odd residual is a tie again, so "round, then add R" and "add R, then round" differ)."""
    pr = pointer_a(M, N, K, dtype, device, bias=False, scale=scale)
    p = P_BITS[dtype]
    n = torch.arange(N, device=device, dtype=torch.int64)
    pr.bias = (2 ** p + 2 * ((n * 37 + 5) % 2 ** (p - 1))).double().to(dtype)
    pr.name = "ties"
    return pr


PROBES = {"pointer-A": pointer_a, "pointer-W": pointer_w, "hadamard": hadamard, "count": count_holes, "ties": ties}


def act_scale(name, K, fp8=False, hot_rows=None):
    """power of two that brings a probe's pre-activations to a few units (quickgelu / swiglu saturate beyond ~ +-17)"""
    if name == "hadamard":
        return 6
    if name == "count":
        return min(max(0, int(math.log2(K)) - 2), 6 if fp8 else 99)          # (e4m3: 2^-6 is the smallest normal number)
    h = max(1, -(-K // hot_rows)) if hot_rows else 1                          # table entries summed per output of a pointer probe
    return (1 if fp8 else 4) + (h - 1).bit_length()


def build(name, M, N, K, dtype, device="cpu", fp8=False, epi=EPI_NONE):
    # The activation epilogues get W scaled by a power of two so that the pre-activations stay within a few units: unscaled, a gate below -88 makes the
    # fp32 exp2 overflow and silu flush to 0 where float64 still has 1e-36 — outside what these probes are about.  (ties under quickgelu: the table
    # scaled, the bias kept — x >= 2^p - 8, the sigmoid is exactly 1 in fp32 and float64 alike, and the store rounds lin + bias once.)
    kw = dict(scale=act_scale(name, K, fp8, N if name == "pointer-W" else M)) if epi in (EPI_QUICKGELU, EPI_SWIGLU) else {}
    if fp8:
        kw["fp8"] = True
    return PROBES[name](M, N, K, dtype, device, **kw)


# ---- the plain reference ------------------------------------------------------------------------------------------------------------------
def swiglu_split(lin):
    """16-row interleaved gate|up columns [.., N] -> (gate, up) [.., N / 2]"""
    v = lin.reshape(*lin.shape[:-1], -1, 2, 16)
    return v[..., 0, :].reshape(*lin.shape[:-1], -1), v[..., 1, :].reshape(*lin.shape[:-1], -1)


def linear64(A, W, fp8=False, sa=None, sw=None):
    """the exact product in float64 (every operand an integer times a power of two, every sum far below 2^53)"""
    lin = widen(A, fp8) @ widen(W, fp8).t()
    if fp8:
        lin = lin * (sa.double()[:, None] * sw.double()[None, :])
    return lin


def reference(A, W, bias, R, epi, dtype, fp8=False, sa=None, sw=None):
    """What the GEMM must store, from float64: EPI_NONE round16(lin + bias); EPI_RESIDUAL round16(round16(lin + bias) + R) (the first rounding
    BEFORE the add); EPI_QUICKGELU / EPI_SWIGLU the float64 function of the exact pre-activation, rounded (these two are judged by act_bound).
    fp8: lin = (A8 . W8^T) sa[m] sw[n] with power-of-two scales.  Returns (stored values, float64 value before the last rounding)."""
    lin = linear64(A, W, fp8, sa, sw)
    if bias is not None and epi != EPI_SWIGLU:
        lin = lin + bias.double()[None, :]
    if epi == EPI_NONE:
        return round16(lin, dtype), lin
    if epi == EPI_RESIDUAL:
        pre = round16(lin, dtype).double() + R.double()
        return round16(pre, dtype), pre
    if epi == EPI_QUICKGELU:
        pre = lin * torch.sigmoid(1.702 * lin)
    elif epi == EPI_SWIGLU:
        g, u = swiglu_split(lin)
        pre = g * torch.sigmoid(g) * u
    else:
        raise ValueError(epi)
    return round16(pre, dtype, exact=False), pre


def probe_reference(pr, epi, sa=None, sw=None):
    return reference(pr.A, pr.W, pr.bias, pr.R if epi == EPI_RESIDUAL else None, epi, pr.dtype, pr.fp8, sa, sw)


def act_error_ratio(got, pre64, dtype, literal=False):
    """max over the outputs of |got - ref| / act_bound"""
    return float(((got.double() - pre64).abs() / act_bound(pre64, dtype, literal)).max())


def pow2_scales(n, lo, hi, mul, device="cpu"):
    """fp32 powers of two 2^e, e cycling through [lo, hi] with step `mul` (coprime to the range): exact multipliers"""
    e = lo + (torch.arange(n, device=device, dtype=torch.int64) * mul) % (hi - lo + 1)
    return (2.0 ** e.double()).float()


# ---- strides, base offsets, poison, guards ------------------------------------------------------------------------------------------------
def lay(x, ld, base, before, after, fill, tail=0):
    """lays the 2-D tensor x into a flat buffer: `before` guard rows, then `base` elements, then the rows of x every `ld` elements, then `after`
    guard rows (+ `tail` elements); everything that is not x holds fill(total elements).  Returns (buffer, the strided view of x's window, offset
    of the window in elements)."""
    rows, cols = x.shape
    assert ld >= cols
    off = before * ld + base
    total = off + (rows + after) * ld + tail
    buf = fill(total).to(x.dtype)
    win = buf.as_strided((rows, cols), (ld, 1), off)
    win.copy_(x)
    return buf, win, off


def poison_fill(device, as_bytes=False):
    """+-2^14, every third element negative (e4m3 bytes: +-448, the largest finite values)"""
    def f(total):
        s = 1 - 2 * (torch.arange(total, device=device, dtype=torch.int64) % 3 == 1).double()
        return (s * 448.0).float().to(FP8).view(torch.uint8) if as_bytes else s * POISON
    return f


STRIDE_CLASSES = {
    # extra leading-dimension elements (A, W, C, R) and base offsets (A, W, C, R), in elements of the operand
    "engine": dict(ld=(64, 128, 192, 64), base=(64, 128, 192, 64)),       # multiples of 64 elements; ldr != ldc
    "api": dict(ld=(8, 8, 8, 8), base=(8, 8, 8, 8)),                      # 16-byte row alignment only: the weakest gemm_shape_ok admits
}


def lay_probe(pr, epi, cls, tile_rows=256, in_place=False):
    """the probe's operands in strided, offset buffers with poison in every pad column and guard row, C pre-filled with the sentinel.  Guard rows
    after M - 1 reach past the end of the last `tile_rows`-row tile, so a store of any row of a tile lands in memory this buffer owns."""
    c = STRIDE_CLASSES[cls]
    dev = pr.A.device
    No = pr.N // 2 if epi == EPI_SWIGLU else pr.N
    after = (-pr.M) % tile_rows + 8
    pf = poison_fill(dev, pr.fp8)
    mul = 2 if pr.fp8 else 1                                               # e4m3 rows: 16-byte alignment is 16 elements
    Ab, Av, _ = lay(pr.A, pr.K + c["ld"][0] * mul, c["base"][0] * mul, 2, after, pf, tail=128)
    Wb, Wv, _ = lay(pr.W, pr.K + c["ld"][1] * mul, c["base"][1] * mul, 2, 2, pf, tail=128)
    ldc = No + c["ld"][2]
    Cb, Cv, coff = lay(torch.zeros((pr.M, No), dtype=pr.dtype, device=dev), ldc, c["base"][2], 2, after, lambda total: torch.zeros(total, device=dev))
    Cb.view(torch.int16).fill_(SENTINEL)                                   # the whole buffer, the window included, starts as sentinel
    out = SimpleNamespace(Ab=Ab, A=Av, Wb=Wb, W=Wv, Cb=Cb, C=Cv, coff=coff, ldc=ldc, Rb=None, R=None, No=No)
    if epi == EPI_RESIDUAL:
        if in_place:
            Cv.copy_(pr.R)
            out.Rb, out.R = Cb, Cv
        else:
            out.Rb, out.R, _ = lay(pr.R, pr.N + c["ld"][3], c["base"][3], 2, after, poison_fill(dev))
    out.snap = [t.clone() for t in (Ab, Wb) + ((out.Rb,) if out.Rb is not None and not in_place else ())]
    return out


def outside_window_intact(Cb, coff, ldc, M, No):
    """every 16-bit word of the C buffer outside the M x No window still holds the sentinel"""
    words = Cb.view(torch.int16)
    idx = torch.arange(words.numel(), device=words.device) - coff
    inside = (idx >= 0) & (idx < M * ldc) & (idx % ldc < No)
    return bool((words[~inside] == SENTINEL).all())
