"""STC connector row kernels (csrc/stc.hip) against float64: dwconv3x3, avgpool, bias_act, scale_rows, im2col3d, permute_conv3d_w — on inputs where
one lost tap, one border that reads the neighbouring row or frame, one dropped ragged pixel, one trailing zero of an even extent or a lost second
grid trip changes the answer.

  references   float64, from the 16-bit tensors exactly as the kernel receives them; every kernel has ONE rounding point, its store.
  bounds       nothing in them comes from a kernel's output.  u = 2^-24 is the unit roundoff of fp32, half_ulp(ref) the one output rounding.
                 im2col3d, permute_conv3d_w   bit equality: they move 16-bit words.
                 scale_rows   bit equality with round16(x gate): two p-bit significands (p = 8 / 11) multiply to at most 2 p <= 22 bits, so the fp32
                              product is exact and the store is the only rounding.  The probes keep |x|, |gate| in [2^-3, 2^3]: the product stays in
                              [2^-6, 2^6], clear of the fp16 subnormal range where a product would lose bits before the store.
                 dwconv3x3    the nine products are exact (as above); the only error is the 9-term fp32 sum, each of whose <= 9 additions rounds a
                              partial sum no larger than S = sum_taps |x w|: |fp32 sum - exact| <= 9 u S.  Bound: half_ulp(ref) + 9 * 2^-24 * S.
                              The integer probes (delta, count, cancel) have partial sums that are multiples of 2^-8 below 2^24 of them: every
                              addition is exact in any order, and they are judged by equality with round16(ref).
                 avgpool      an fp32 sum of HW terms in ANY order is off by at most (HW - 1) u A (A = sum_p |x_p|, first order: each of the HW - 1
                              additions rounds a partial sum <= A); the division by HW adds one more rounding of the quotient, <= u A / HW; the
                              conversion of HW to fp32 is exact (HW < 2^24).  Over HW: (HW - 1 + 1) u A / HW <= (HW + 1) * 2^-24 * mean_p |x_p|.
                              Bound: half_ulp(ref) + (HW + 1) * 2^-24 * mean |x|.  Integer probes with HW a power of two (exact sums, exact
                              division): equality with round16(ref).
                 bias_act     x + bias is one fp32 addition (relative u); the fast exp of |t| <= 88 carries the rounding of t log2(e) into the
                              exponent: |t| 2^-24 relative, <= 88 * 2^-24 < 2^-17.4; the division and the product a few u more.  All of it stays
                              below gemm_probes.ACT_RTOL_SLACK = 2^-15.  Bound: half_ulp(ref) + 2^-15 |ref|.  GELU adds 2^-22 |t|: 1 + erf(t / sqrt 2)
                              cancels in fp32 for negative t — the sum is known to 2^-24 absolute however small it is, erff itself to a few of those —
                              and 0.5 |t| times 8 * 2^-24 is 2^-22 |t|; the reference's own fp32 evaluation cancels the same way.  The float64
                              reference uses erfc for t < 0, which does not cancel.
               A bound never goes below one subnormal step of the element type.  Equality means equal VALUES (+0 == -0) and no NaN.
  emulations   plain torch restatements of each kernel's STRUCTURE: one item per 8-channel chunk, item i of a launch of min(ceil(items / 256), cap)
               workgroups x 256 threads handled by thread i mod (grid 256) on trip i div (grid 256) (cap = 8192 in the kernels; the CPU tests
               lower it to take the later trips at small shapes); 32 pixel lanes x 64-channel slabs for the pool; the tap bit order of the gather.
               Each takes fault=<name>: tests/test_stc_probes_cpu.py shows that every fault is rejected by a named probe.
  probes       delta (channel c's weight is 1 at tap c % 9: the output is a shifted copy with zeros at the border, every element names its source),
               count (integers in [-8, 8] x weights in [-4, 4]), cancel (+big and -big taps / pixels and a small remainder), gauss (judged by the
               bound), one-hot (the pool: one large pixel at each position in turn), the activation grid, ident (the movers: distinct non-zero words).
               Every output buffer is filled with SENTINEL and followed by guard words; every input is followed by POISON and checked unchanged.

Runs on the CPU and on a device; nothing here imports the HIP library."""
import math
from types import SimpleNamespace

import torch

import gemm_probes as GP
from encode_probes import POISON, half_ulp
from gemm_probes import SENTINEL, round16, subnormal_step

U32 = 2.0 ** -24
SLACK = GP.ACT_RTOL_SLACK            # 2^-15
GELU_EXTRA = 2.0 ** -22
CAP = 8192                           # grid_for's cap on the workgroups of a launch
GUARD = 256                          # guard words behind every buffer
ACT_NONE, ACT_SILU, ACT_SIGMOID, ACT_GELU = 0, 1, 2, 3
ACT_NAMES = {ACT_NONE: "none", ACT_SILU: "silu", ACT_SIGMOID: "sigmoid", ACT_GELU: "gelu"}
INF = float("inf")


# ---- buffers -------------------------------------------------------------------------------------------------------------------------------
def guarded(x, fill):
    """x -> (flat buffer of x.numel() + GUARD elements, view of x's shape at element 0); the guard holds `fill` (a number, or "sentinel")"""
    buf = torch.empty(x.numel() + GUARD, dtype=x.dtype, device=x.device)
    if fill == "sentinel":
        buf.view(torch.int16).fill_(SENTINEL)
    else:
        buf.fill_(fill)
    v = buf[:x.numel()].view(x.shape)
    v.copy_(x)
    return buf, v


def sentinel_out(shape, dtype, device):
    """(flat buffer, view): an output of `shape`, every word — the guard's too — SENTINEL"""
    n = int(math.prod(shape))
    buf = torch.empty(n + GUARD, dtype=dtype, device=device)
    buf.view(torch.int16).fill_(SENTINEL)
    return buf, buf[:n].view(shape)


def with_guard(v):
    """the flat buffer (guard included) that a view made by guarded() / sentinel_out() sits at the start of"""
    return v.as_strided((v.numel() + GUARD,), (1,), v.storage_offset())


def guard_intact(buf, n, snap=None):
    """the words behind the first n still hold what they held (`snap`: a copy of the buffer before the call; None: SENTINEL)"""
    tail = buf[n:].view(torch.int16)
    return bool((tail == SENTINEL).all()) if snap is None else bool((tail == snap[n:].view(torch.int16)).all())


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int16) == b.contiguous().view(torch.int16)).all())


def sentinel_words(v):
    """how many words of an output still hold SENTINEL (none of the probes' answers is that value)"""
    return int((v.contiguous().view(torch.int16) == SENTINEL).sum())


# ---- judges --------------------------------------------------------------------------------------------------------------------------------
def ratio_bound(got, ref64, bound64, dtype):
    """max |got - ref| / bound (inf for a NaN); the bound floored at one subnormal step"""
    b = torch.clamp(bound64, min=subnormal_step(dtype))
    q = torch.nan_to_num((got.double() - ref64).abs() / b, nan=INF, posinf=INF)
    return float(q.max())


def ratio_exact(got, ref64, dtype):
    """0 if got == round16(ref) in value everywhere, else inf (ref: exact in fp32)"""
    return 0.0 if bool((got.double() == round16(ref64, dtype).double()).all()) else INF


def describe(name, got, ref64, bound64=None):
    g = got.double()
    e = torch.nan_to_num((g - ref64).abs(), nan=INF)
    if bound64 is not None:
        e = e / bound64.clamp(min=1e-300)
    i = int(torch.argmax(e))
    idx = [int(v) for v in torch.unravel_index(torch.tensor(i), e.shape)]
    return f"{name}: worst at {idx}: got {float(g.flatten()[i]):.7g} ref {float(ref64.flatten()[i]):.7g}" + \
        (f" (error / bound {float(e.flatten()[i]):.3f})" if bound64 is not None else "")


# ---- generators ----------------------------------------------------------------------------------------------------------------------------
def _gauss(shape, seed, device):
    n = int(math.prod(shape))
    if n > (1 << 22) and torch.device(device).type != "cpu":
        g = torch.Generator(device=device).manual_seed(int(seed))
        return torch.randn(shape, generator=g, dtype=torch.float32, device=device)
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(shape, generator=g, dtype=torch.float32).to(device)


def _ar(n, device):
    return torch.arange(n, device=device, dtype=torch.int64)


def ident_words(shape, dtype, device, salt=0):
    """distinct non-zero finite values, by bit pattern: word i = 0x3001 + (i + salt) % 4093 (in [2^-31, 2) for bf16 and [1/8, 2) for fp16; never
    SENTINEL; two elements less than 4093 apart differ)"""
    n = int(math.prod(shape))
    return (0x3001 + (_ar(n, device) + salt) % 4093).to(torch.int16).view(dtype).view(shape)


def grid_of(items, cap=CAP):
    return min(-(-items // 256), cap)


def trips_of(items, cap=CAP):
    return -(-items // (grid_of(items, cap) * 256))


def _first_trip(items, cap, device):
    """mask over the items: handled on the first trip of a launch capped at `cap` workgroups"""
    return _ar(items, device) < grid_of(items, cap) * 256


# ---- dwconv3x3 -----------------------------------------------------------------------------------------------------------------------------
DWCONV_PROBES = ("delta", "count", "cancel", "gauss")
DWCONV_EXACT = ("delta", "count", "cancel")
DWCONV_FAULTS = ("taps_transposed", "taps_flipped", "wrap_row", "wrap_frame", "lost_tap", "weight_layout", "weight_chunk0", "second_trip_lost")


def _pos_ints(N, H, W, C, device):
    """a non-zero integer in [-254, 254] per (frame, row, column), offset per channel: any 508 consecutive positions are distinct"""
    pos = _ar(N * H * W, device).view(N, H, W, 1)
    k = (pos + 7 * _ar(C, device).view(1, 1, 1, C)) % 508 - 254
    return torch.where(k >= 0, k + 1, k).double()


def _hash(shape, device, mod, salt):
    idx = _ar(int(math.prod(shape)), device)
    return ((idx * 2654435761 + salt * 40503 + (idx // 7) * 97 + (idx // 61) * 31) % 1000003 % mod).view(shape)


def dwconv_probe(name, N, H, W, C, dtype, device="cpu"):
    """-> (x [N, H, W, C], w [C, 9])"""
    c = _ar(C, device)
    if name == "delta":
        w = (_ar(9, device)[None, :] == (c % 9)[:, None]).double()
        x = _pos_ints(N, H, W, C, device)
    elif name == "count":
        x = (_hash((N, H, W, C), device, 17, 1) - 8).double()
        w = (_hash((C, 9), device, 9, 2) - 4).double()
    elif name == "cancel":
        # the 8 outer taps +-1, four of each, the centre 2^-7; x = 64 + r / 2, r in {-1, 0, 1}: an interior output is sum +- r / 2 + x / 128 next to
        # taps of 64 — all multiples of 2^-8, so every partial sum is exact
        sgn = torch.tensor([1, -1, 1, -1, 0, -1, 1, -1, 1], device=device, dtype=torch.float64)
        w = (sgn[None, :] * (1 - 2 * (c % 2)).double()[:, None]).clone()
        w[:, 4] = 2.0 ** -7
        x = 64.0 + (_hash((N, H, W, C), device, 3, 3) - 1).double() / 2
    elif name == "gauss":
        x = _gauss((N, H, W, C), 101 + N + H * W + C, device).double()
        w = _gauss((C, 9), 103 + C, device).double() * 0.5
    else:
        raise ValueError(name)
    xo, wo = x.to(dtype), w.to(dtype)
    if name != "gauss":
        assert bool((xo.double() == x).all()) and bool((wo.double() == w).all())
    return xo, wo


def dwconv_reference(x, w):
    """-> (ref64, S = sum over the taps of |x w|) of the depthwise 3 x 3, pad 1, stride 1"""
    N, H, W, C = x.shape
    xp = torch.zeros((N, H + 2, W + 2, C), dtype=torch.float64, device=x.device)
    xp[:, 1:-1, 1:-1] = x.double()
    w64 = w.double().view(C, 9)
    ref = torch.zeros((N, H, W, C), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            t = xp[:, ky:ky + H, kx:kx + W] * w64[:, ky * 3 + kx]
            ref += t
            mag += t.abs()
    return ref, mag


def dwconv_bound(ref64, mag64, dtype):
    return half_ulp(ref64, dtype) + 9 * U32 * mag64


def emulate_dwconv(xbuf, w, ybuf, N, H, W, C, dtype, fault=None, cap=CAP):
    """dwconv3x3_kernel on flat buffers: item i = (pixel, 8-channel chunk), the chunk's 72 weights one block of w, the taps added in row-major order
    in fp32.  A read past the end of xbuf (a fault's) returns the last guard word."""
    dev = xbuf.device
    cpr = C // 8
    items = N * H * W * cpr
    i = _ar(items, dev)
    ch, pix = i % cpr, i // cpr
    px, py, n = pix % W, (pix // W) % H, pix // (W * H)
    e = _ar(8, dev)[None, :]
    xf, wf = xbuf.float(), w.reshape(-1).float()
    acc = torch.zeros((items, 8), dtype=torch.float32, device=dev)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            tap = (dy + 1) * 3 + (dx + 1)
            if fault == "lost_tap" and tap == 5:
                continue
            yy, xx = py + dy, px + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            src = (n * H + yy) * W + xx
            if fault == "wrap_row":                       # the column test is missing: the border reads the neighbouring row's pixel
                ok = (yy >= 0) & (yy < H) & (src >= 0) & (src < N * H * W)
            if fault == "wrap_frame":                     # the row test is missing: the border reads the neighbouring frame's row
                ok = (xx >= 0) & (xx < W) & (src >= 0) & (src < N * H * W)
            xi = (src[:, None] * C + ch[:, None] * 8 + e).clamp(0, xf.numel() - 1)
            v = torch.where(ok[:, None], xf[xi], torch.zeros((), dtype=torch.float32, device=dev))
            wt = {"taps_transposed": (dx + 1) * 3 + (dy + 1), "taps_flipped": 8 - tap}.get(fault, tap)
            wi = (e * 0 + wt * 8 + e) if fault == "weight_layout" else (e * 9 + wt)
            wi = wi + (0 if fault == "weight_chunk0" else ch[:, None] * 72)
            acc = acc + v * wf[wi]
    out = acc.to(dtype)
    yi = pix[:, None] * C + ch[:, None] * 8 + e
    if fault == "second_trip_lost":
        keep = _first_trip(items, cap, dev)
        yi, out = yi[keep], out[keep]
    ybuf[yi.reshape(-1)] = out.reshape(-1)
    return ybuf


def dwconv_case(name, N, H, W, C, dtype, device, run):
    """one probe through `run(x, w, y)` (views of guarded buffers) -> (error / bound, [problems])"""
    x, w = dwconv_probe(name, N, H, W, C, dtype, device)
    xb, xv = guarded(x, POISON)
    yb, yv = sentinel_out((N, H, W, C), dtype, device)
    snap_x, snap_w = xb.clone(), w.clone()
    run(xv, w, yv)
    ref, mag = dwconv_reference(x, w)
    r = ratio_exact(yv, ref, dtype) if name in DWCONV_EXACT else ratio_bound(yv, ref, dwconv_bound(ref, mag, dtype), dtype)
    bad = []
    if not (same_bits(xb, snap_x) and same_bits(w, snap_w)):
        bad.append("an input changed")
    if not guard_intact(yb, x.numel()):
        bad.append("a store behind the output")
    if r > 1:
        bad.append(describe(name, yv, ref, None if name in DWCONV_EXACT else dwconv_bound(ref, mag, dtype)))
    return r, bad


# ---- avgpool -------------------------------------------------------------------------------------------------------------------------------
AVGPOOL_PROBES = ("count", "cancel", "gauss", "onehot")
AVGPOOL_FAULTS = ("ragged_pixels_lost", "divide_by_padded", "slab_shift", "frame_mix")
ONEHOT_BIG = 192.0


def onehot_shifts(HW, C):
    """the shifts at which the one-hot probe's hot pixels (c + 7 n + shift) % HW visit every position of every frame"""
    return list(range(0, HW, C))


def avgpool_probe(name, N, HW, C, dtype, device="cpu", shift=0):
    """-> x [N, HW, C]"""
    n, p, c = _ar(N, device).view(N, 1, 1), _ar(HW, device).view(1, HW, 1), _ar(C, device).view(1, 1, C)
    if name == "count":
        x = (_hash((N, HW, C), device, 17, 5) - 8).double()
    elif name == "cancel":                    # +-64 alternating along the pixels (an odd HW leaves one over) + r / 2, r in {-1, 0, 1}
        x = 64.0 * (1 - 2 * ((p + c + n) % 2)).double() + (_hash((N, HW, C), device, 3, 6) - 1).double() / 2
    elif name == "gauss":
        x = _gauss((N, HW, C), 211 + N + HW + C, device).double() + 0.25
    elif name == "onehot":                    # one large pixel per (frame, channel), distinct in size per channel residue
        x = ((p == (c + 7 * n + shift) % HW).double() * ONEHOT_BIG * (1 + (c % 3)).double())
    else:
        raise ValueError(name)
    xo = x.to(dtype)
    if name != "gauss":
        assert bool((xo.double() == x).all())
    return xo


def avgpool_reference(x):
    x64 = x.double()
    return x64.sum(1) / x.shape[1], x64.abs().sum(1) / x.shape[1]


def avgpool_bound(ref64, meanabs64, HW, dtype):
    return half_ulp(ref64, dtype) + (HW + 1) * U32 * meanabs64


def avgpool_is_exact(name, HW):
    return name in ("count", "cancel") and HW & (HW - 1) == 0


def emulate_avgpool(xbuf, ybuf, N, HW, C, dtype, fault=None):
    """avgpool_kernel: one workgroup per (frame, 64-channel slab); pixel lane l of 32 adds pixels l, l + 32, ... in fp32, the 32 lane sums are added in
    lane order, one division by HW"""
    dev = xbuf.device
    nslab = C // 64
    trips = -(-HW // 32)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    xf = xbuf.float()
    nn, sl, l, cc = _ar(N, dev).view(N, 1, 1, 1), _ar(nslab, dev).view(1, nslab, 1, 1), _ar(32, dev).view(1, 1, 32, 1), _ar(64, dev).view(1, 1, 1, 64)
    src_slab = (sl + 1) % nslab if fault == "slab_shift" else sl
    acc = torch.zeros((N, nslab, 32, 64), dtype=torch.float32, device=dev)
    for t in range(trips):
        p = l + 32 * t
        ok = p < ((HW // 32) * 32 if fault == "ragged_pixels_lost" else HW)
        fr = (nn + 1) % N if (fault == "frame_mix" and t > 0) else nn
        xi = ((fr * HW + p) * C + src_slab * 64 + cc).clamp(0, xf.numel() - 1)
        acc = acc + torch.where(ok, xf[xi], zero)
    s = torch.zeros((N, nslab, 64), dtype=torch.float32, device=dev)
    for q in range(32):
        s = s + acc[:, :, q]
    den = float(trips * 32 if fault == "divide_by_padded" else HW)
    ybuf[:N * C] = (s / den).to(dtype).reshape(-1)
    return ybuf


def avgpool_case(name, N, HW, C, dtype, device, run, shift=0):
    """`run(x, y)` -> (error / bound, [problems])"""
    x = avgpool_probe(name, N, HW, C, dtype, device, shift)
    xb, xv = guarded(x, POISON)
    yb, yv = sentinel_out((N, C), dtype, device)
    snap = xb.clone()
    run(xv, yv)
    ref, ma = avgpool_reference(x)
    exact = avgpool_is_exact(name, HW)
    r = ratio_exact(yv, ref, dtype) if exact else ratio_bound(yv, ref, avgpool_bound(ref, ma, HW, dtype), dtype)
    bad = []
    if not same_bits(xb, snap):
        bad.append("the input changed")
    if not guard_intact(yb, N * C):
        bad.append("a store behind the output")
    if r > 1:
        bad.append(describe(name, yv, ref, None if exact else avgpool_bound(ref, ma, HW, dtype)))
    return r, bad


# ---- bias_act ------------------------------------------------------------------------------------------------------------------------------
BIAS_ACT_PROBES = ("grid", "gauss")
BIAS_ACT_FAULTS = ("act_swapped", "bias_skipped", "bias_chunk0", "act_before_bias", "second_trip_lost")
ACT_GRID = (0.0, 2.0 ** -14, 0.5, 1.0, 2.0, 5.0, 20.0, 88.0)


def act_bias(C, dtype, device="cpu"):
    """a non-zero bias that differs in every channel below 1280: +-(1 + m / 128) 2^(e - 3), m < 128, e < 5 (8 significand bits: exact in bf16 and fp16),
    the sign alternating from channel to channel"""
    c = _ar(C, device)
    return ((1 - 2 * (c % 2)).double() * (1 + ((c // 2) % 128).double() / 128) * torch.exp2(((c // 256) % 5 - 3).double())).to(dtype)


def bias_act_probe(name, rows, C, dtype, device="cpu", bias=None):
    """-> x [rows, C].  grid: the 15 values {0, +-2^-14, +-0.5, +-1, +-2, +-5, +-20, +-88} walked along the row, the walk shifted per row.  exp(|t|)
    leaves fp32 past |t| = 88.7 (and the bound's exp term is derived for |t| <= 88), so with a bias the +-88 entries take the sign that the
    channel's bias pulls back towards zero: |x + bias| stays below 88, on both sides (the bias alternates in sign)"""
    if name == "grid":
        g = torch.tensor([0.0] + [s * v for v in ACT_GRID[1:] for s in (1.0, -1.0)], dtype=torch.float64, device=device)
        r, c = _ar(rows, device)[:, None], _ar(C, device)[None, :]
        x = g[(c + 4 * r) % g.numel()]
        if bias is not None:
            x = torch.where(x.abs() == 88.0, -88.0 * torch.sign(bias.double())[None, :], x)
    elif name == "gauss":
        x = _gauss((rows, C), 307 + rows + C, device).double() * 2
    else:
        raise ValueError(name)
    return x.to(dtype)


def act64(t, act):
    if act == ACT_SILU:
        return t * torch.sigmoid(t)
    if act == ACT_SIGMOID:
        return torch.sigmoid(t)
    if act == ACT_GELU:           # 0.5 t (1 + erf(t / sqrt 2)); for t < 0 as 0.5 t erfc(-t / sqrt 2), which does not cancel
        z = t / math.sqrt(2.0)
        return 0.5 * t * torch.where(t < 0, torch.erfc(-z), 1 + torch.erf(z))
    return t


def bias_act_reference(x, bias, act):
    """-> (ref64, t = x + bias)"""
    t = x.double() + (0.0 if bias is None else bias.double()[None, :])
    return act64(t, act), t


def bias_act_bound(ref64, t64, act, dtype):
    return half_ulp(ref64, dtype) + SLACK * ref64.abs() + (GELU_EXTRA * t64.abs() if act == ACT_GELU else 0.0)


def _act32(t, act):
    if act == ACT_SILU:
        return t / (1 + torch.exp(-t))
    if act == ACT_SIGMOID:
        return 1 / (1 + torch.exp(-t))
    if act == ACT_GELU:
        return 0.5 * t * (1 + torch.erf(t * 0.70710678118654752))
    return t


def emulate_bias_act(xbuf, bias, rows, C, act, dtype, fault=None, cap=CAP):
    """bias_act_kernel in place on a flat buffer: item i = (row, 8-channel chunk), t = x + bias in fp32, the activation in fp32, one store"""
    dev = xbuf.device
    n = rows * C
    x = xbuf[:n].view(rows, C).float()
    b = torch.zeros(C, dtype=torch.float32, device=dev) if (bias is None or fault == "bias_skipped") else bias.float()
    if fault == "bias_chunk0":
        b = b[:8].repeat(C // 8)
    a = {ACT_SILU: ACT_SIGMOID, ACT_SIGMOID: ACT_SILU}.get(act, act) if fault == "act_swapped" else act
    out = (_act32(x, a) + b if fault == "act_before_bias" else _act32(x + b, a)).to(dtype)
    if fault == "second_trip_lost":
        keep = _first_trip(rows * (C // 8), cap, dev).repeat_interleave(8).view(rows, C)
        out = torch.where(keep, out, xbuf[:n].view(rows, C))
    xbuf[:n] = out.reshape(-1)
    return xbuf


def bias_act_case(name, rows, C, act, with_bias, dtype, device, run):
    """`run(x, bias_or_None, act)` in place -> (error / bound, [problems])"""
    bias = act_bias(C, dtype, device) if with_bias else None
    x = bias_act_probe(name, rows, C, dtype, device, bias)
    xb, xv = guarded(x, "sentinel")
    snap = xb.clone()
    snap_b = None if bias is None else bias.clone()
    run(xv, bias, act)
    ref, t = bias_act_reference(x, bias, act)
    bound = bias_act_bound(ref, t, act, dtype)
    r = ratio_bound(xv, ref, bound, dtype)
    bad = []
    if bias is not None and not same_bits(bias, snap_b):
        bad.append("the bias changed")
    if not guard_intact(xb, rows * C, snap):
        bad.append("a store behind the rows")
    if r > 1:
        bad.append(describe(f"{name} {ACT_NAMES[act]}", xv, ref, bound))
    return r, bad


# ---- scale_rows ----------------------------------------------------------------------------------------------------------------------------
SCALE_PROBES = ("ramp", "gauss")
SCALE_FAULTS = ("gate_frame0", "gate_frame_pow2", "second_trip_lost")


def _clear_of_subnormals(v64, dtype):
    """sign(v) * |v| clamped into [2^-3, 2^3], rounded to the element type"""
    s = torch.where(v64 < 0, -1.0, 1.0)
    return (s * v64.abs().clamp(2.0 ** -3, 2.0 ** 3)).to(dtype)


def scale_probe(name, N, HW, C, dtype, device="cpu"):
    """-> (x [N, HW, C], gate [N, C]); the gate differs in every (frame, channel) near by"""
    n, c = _ar(N, device)[:, None], _ar(C, device)[None, :]
    if name == "ramp":                       # full-significand values: products that need the rounding
        p = GP.P_BITS[dtype]
        gate = (1 + ((c * 37 + n * 101) % (2 ** (p - 1))).double() * 2.0 ** -(p - 1)) * torch.exp2(((n + c) % 5 - 3).double())
        x = (1 + ((_hash((N, HW, C), device, 2 ** (p - 1), 8)).double() * 2.0 ** -(p - 1))) * (1 - 2 * (_hash((N, HW, C), device, 2, 9))).double()
        return x.to(dtype), gate.to(dtype)
    if name == "gauss":
        return (_clear_of_subnormals(_gauss((N, HW, C), 401 + N + HW + C, device).double(), dtype),
                _clear_of_subnormals(torch.sigmoid(_gauss((N, C), 409 + N + C, device).double() * 2), dtype))
    raise ValueError(name)


def scale_reference(x, gate, dtype):
    """round16(x gate): the float64 product is exact, so this is one rounding"""
    pr = x.double() * gate.double()[:, None, :]
    assert bool((pr.float().double() == pr).all()), "the product of two 16-bit values is an exact fp32 number"
    return pr.float().to(dtype)


def emulate_scale_rows(xbuf, gate, N, HW, C, dtype, fault=None, cap=CAP):
    dev = xbuf.device
    cpr = C // 8
    items = N * HW * cpr
    i = _ar(items, dev)
    ch, pix = i % cpr, i // cpr
    n = pix // HW
    if fault == "gate_frame0":
        n = n * 0
    if fault == "gate_frame_pow2":           # the frame from a shift by ceil(log2 HW)
        n = (pix >> max(HW - 1, 0).bit_length()).clamp(max=N - 1)
    e = _ar(8, dev)[None, :]
    xi = pix[:, None] * C + ch[:, None] * 8 + e
    gi = n[:, None] * C + ch[:, None] * 8 + e
    out = (xbuf.float()[xi] * gate.reshape(-1).float()[gi]).to(dtype)
    if fault == "second_trip_lost":
        keep = _first_trip(items, cap, dev)
        xi, out = xi[keep], out[keep]
    xbuf[xi.reshape(-1)] = out.reshape(-1)
    return xbuf


def scale_case(name, N, HW, C, dtype, device, run):
    """`run(x, gate)` in place -> (0 or inf, [problems])"""
    x, gate = scale_probe(name, N, HW, C, dtype, device)
    xb, xv = guarded(x, "sentinel")
    snap, snap_g = xb.clone(), gate.clone()
    ref = scale_reference(x, gate, dtype)
    run(xv, gate)
    r = 0.0 if same_bits(xv, ref) else INF
    bad = []
    if not same_bits(gate, snap_g):
        bad.append("the gate changed")
    if not guard_intact(xb, x.numel(), snap):
        bad.append("a store behind the rows")
    if r > 1:
        bad.append(describe(name, xv, ref.double()))
    return r, bad


# ---- im2col3d ------------------------------------------------------------------------------------------------------------------------------
IM2COL_FAULTS = ("no_leading_pad", "tap_order", "trailing_clamped", "zeros_not_written", "second_trip_lost")


def out_extent(d):
    return d // 2 + 1


def im2col_reference(x):
    """x [T, H, W, C] -> A [To Ho Wo, 8 C] by slicing the zero-padded tensor (no index arithmetic shared with the emulation)"""
    T, H, W, C = x.shape
    To, Ho, Wo = out_extent(T), out_extent(H), out_extent(W)
    xp = torch.zeros((2 * To, 2 * Ho, 2 * Wo, C), dtype=x.dtype, device=x.device)
    xp[1:T + 1, 1:H + 1, 1:W + 1] = x
    A = torch.empty((To, Ho, Wo, 2, 2, 2, C), dtype=x.dtype, device=x.device)
    for kt in range(2):
        for kh in range(2):
            for kw in range(2):
                A[:, :, :, kt, kh, kw] = xp[kt::2, kh::2, kw::2]
    return A.view(To * Ho * Wo, 8 * C)


def emulate_im2col3d(xbuf, abuf, T, H, W, C, dtype, fault=None, cap=CAP):
    dev = xbuf.device
    To, Ho, Wo = out_extent(T), out_extent(H), out_extent(W)
    cpr = C // 8
    items = To * Ho * Wo * 8 * cpr
    i = _ar(items, dev)
    ch, rest = i % cpr, i // cpr
    tap, row = rest & 7, rest >> 3
    xo, yo, to = row % Wo, (row // Wo) % Ho, row // (Wo * Ho)
    kt, kh, kw = (tap & 1, (tap >> 1) & 1, tap >> 2) if fault == "tap_order" else (tap >> 2, (tap >> 1) & 1, tap & 1)
    lead = 0 if fault == "no_leading_pad" else 1
    t, yy, xx = 2 * to - lead + kt, 2 * yo - lead + kh, 2 * xo - lead + kw
    if fault == "trailing_clamped":
        t, yy, xx = t.clamp(max=T - 1), yy.clamp(max=H - 1), xx.clamp(max=W - 1)
    ok = (t >= 0) & (t < T) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    e = _ar(8, dev)[None, :]
    xi = ((((t * H + yy) * W + xx) * C + ch * 8)[:, None] + e).clamp(0, xbuf.numel() - 1)
    v = torch.where(ok[:, None], xbuf[xi], torch.zeros((), dtype=dtype, device=dev))
    ai = ((row * 8 + tap) * C + ch * 8)[:, None] + e
    keep = torch.ones(items, dtype=torch.bool, device=dev)
    if fault == "zeros_not_written":
        keep &= ok
    if fault == "second_trip_lost":
        keep &= _first_trip(items, cap, dev)
    abuf[ai[keep].reshape(-1)] = v[keep].reshape(-1)
    return abuf


def im2col_case(T, H, W, C, dtype, device, run):
    """`run(x, A_flat_buffer)`: ident words -> (0 or inf, [problems])"""
    x = ident_words((T, H, W, C), dtype, device, salt=T + H)
    xb, xv = guarded(x, POISON)
    rows = out_extent(T) * out_extent(H) * out_extent(W)
    ab, av = sentinel_out((rows, 8 * C), dtype, device)
    snap = xb.clone()
    run(xv, ab)
    ref = im2col_reference(x)
    r = 0.0 if same_bits(av, ref) else INF
    bad = []
    if not same_bits(xb, snap):
        bad.append("the input changed")
    if not guard_intact(ab, rows * 8 * C):
        bad.append("a store behind the matrix")
    if r > 1:
        bad.append(f"{sentinel_words(av)} words never written; " + describe("ident", av, ref.double()))
    return r, bad


# ---- permute_conv3d_w ----------------------------------------------------------------------------------------------------------------------
PERMUTE_FAULTS = ("co_ci_swapped", "tap_minor", "second_trip_lost")


def permute_reference(w):
    """Conv3d weight [Co, Ci, 2, 2, 2] -> [Co, 8 Ci], tap = (kt 2 + kh) 2 + kw major, ci minor"""
    Co, Ci = w.shape[:2]
    return w.reshape(Co, Ci, 8).permute(0, 2, 1).reshape(Co, 8 * Ci).contiguous()


def emulate_permute(wbuf, obuf, Co, Ci, dtype, fault=None, cap=CAP):
    dev = wbuf.device
    items = Co * Ci * 8
    i = _ar(items, dev)
    tap, rest = i & 7, i >> 3
    if fault == "co_ci_swapped":
        ci, co = rest % Co, rest // Co
        oi = (co * 8 + tap) * Co + ci
    else:
        ci, co = rest % Ci, rest // Ci
        oi = (co * 8 + tap) * Ci + ci
    if fault == "tap_minor":
        oi = (co * Ci + ci) * 8 + tap
    v = wbuf[:items]
    if fault == "second_trip_lost":
        keep = _first_trip(items, cap, dev)
        oi, v = oi[keep], v[keep]
    obuf[oi] = v
    return obuf


def permute_case(Co, Ci, dtype, device, run):
    """`run(w, out)` -> (0 or inf, [problems])"""
    w = ident_words((Co, Ci, 2, 2, 2), dtype, device, salt=Co)
    wb, wv = guarded(w, POISON)
    ob, ov = sentinel_out((Co, 8 * Ci), dtype, device)
    snap = wb.clone()
    run(wv, ov)
    ref = permute_reference(w)
    r = 0.0 if same_bits(ov, ref) else INF
    bad = []
    if not same_bits(wb, snap):
        bad.append("the input changed")
    if not guard_intact(ob, Co * Ci * 8):
        bad.append("a store behind the output")
    if r > 1:
        bad.append(f"{sentinel_words(ov)} words never written; " + describe("ident", ov, ref.double()))
    return r, bad


# ---- the shapes the GPU tests run (tests/test_stc_probes_cpu.py runs the emulations at the same ones) --------------------------------------------
DWCONV_SHAPES = [(1, 1, 1, 8), (2, 1, 5, 8), (2, 5, 1, 16), (2, 3, 5, 24), (3, 2, 2, 64), (2, 7, 7, 72), (3, 4, 4, 256), (2, 13, 13, 4096)]
DWCONV_TWO_TRIPS = (9, 24, 24, 4096)
AVGPOOL_HW, AVGPOOL_C, AVGPOOL_N = (1, 7, 31, 32, 33, 36, 169, 576), (64, 192, 4096), (1, 3, 32)
AVGPOOL_SHAPES = [(n, hw, 64) for hw in AVGPOOL_HW for n in AVGPOOL_N] + \
    [(AVGPOOL_N[i % 3], hw, c) for c in AVGPOOL_C[1:] for i, hw in enumerate(AVGPOOL_HW)]          # (N, HW, C): the product at C = 64, a diagonal elsewhere
BIAS_ACT_ROWS, BIAS_ACT_C = (1, 3, 17, 32), (8, 64, 256, 1024)
BIAS_ACT_TWO_TRIPS = (5184, 4096)
SCALE_SHAPES = [(3, 7, 8), (2, 36, 256), (17, 169, 4096)]
SCALE_TWO_TRIPS = (9, 576, 4096)
IM2COL_SHAPES = [(1, 1, 1, 8), (1, 2, 3, 8), (2, 2, 2, 16), (3, 5, 4, 8), (4, 6, 6, 256), (3, 7, 7, 64), (2, 24, 24, 1024)]
IM2COL_TWO_TRIPS = (8, 24, 24, 4096)
PERMUTE_SHAPES = [(16, 8), (8, 24), (256, 256)]
PERMUTE_TRIPS = (1024, 1024)


# ---- the chains: Conv3d and squeeze-excite as the engine computes them -----------------------------------------------------------------------
def conv3d_probe(T, H, W, C, Co, dtype, device="cpu"):
    """integer data: x [T, H, W, C] in {-2, -1, 1, 2}, Conv3d weight [Co, C, 2, 2, 2] in {-1, 0, 1}, bias [Co] in [-8, 8]: the pre-activation is an
    exact integer of at most 16 C + 8; at C = 8 it stays within the +-88 that the SiLU behind it is judged on (test_stc_probes_cpu.py checks both)"""
    x = _hash((T, H, W, C), device, 4, 11) - 2
    x = torch.where(x >= 0, x + 1, x).double()
    w = (_hash((Co, C, 2, 2, 2), device, 3, 12) - 1).double()
    b = (_hash((Co,), device, 17, 13) - 8).double()
    return x.to(dtype), w.to(dtype), b.to(dtype)


def conv3d_reference(x, w, b):
    """F.conv3d in float64 (stride 2, padding 1) on channels-first views -> [To Ho Wo, Co], rows ordered (to, yo, xo)"""
    y = torch.nn.functional.conv3d(x.double().permute(3, 0, 1, 2)[None], w.double(), b.double(), stride=2, padding=1)[0]      # [Co, To, Ho, Wo]
    return y.permute(1, 2, 3, 0).reshape(-1, w.shape[0])


def se_probe(N, HW, C, rd, dtype, device="cpu"):
    """z [N, HW, C], fc1 [rd, C] / bias [rd], fc2 [C, rd] / bias [C]: Gaussian, scaled so that the gates spread over (0, 1)"""
    z = _gauss((N, HW, C), 503 + N + C, device) + 0.5
    fc1w, fc1b = _gauss((rd, C), 509 + C, device) * (2.0 / math.sqrt(C)), _gauss((rd,), 521 + rd, device) * 0.5
    fc2w, fc2b = _gauss((C, rd), 523 + C, device) * (2.0 / math.sqrt(rd)), _gauss((C,), 541 + C, device) * 0.5
    return SimpleNamespace(z=z.to(dtype), fc1w=fc1w.to(dtype), fc1b=fc1b.to(dtype), fc2w=fc2w.to(dtype), fc2b=fc2b.to(dtype))


def linear_bound(x, w, ref64, dtype):
    """a K-term fp32 dot product in any order, stored once: half_ulp(ref) + K * 2^-24 * sum_k |x_k w_k|"""
    mag = x.double().abs() @ w.double().abs().t()
    return half_ulp(ref64, dtype) + x.shape[1] * U32 * mag
