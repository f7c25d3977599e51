"""Encode-side probes: the norms (csrc/norm.hip), the slot pool (csrc/slot_pool.hip) and the ViT front end (csrc/patch_embed.hip, and the
three-pass im2col / GEMM / assemble path of csrc/vit.hip) against float64, on inputs where one lost row, one shifted chunk or one wrong pixel
changes the answer.

  references   float64, from the 16-bit tensors exactly as the kernel receives them, with the documented rounding points only:
                 norms       y = el(LN(x)); silu / res forms: the LN output is rounded to 16 bits BEFORE the add and the SiLU
                 slot pool   LN, RoPE with the caller's tables, softmax over the patches, weighted sum; the rotated row is rounded to 16 bits for the
                             logit dot product ONLY
                 front end   pe = el(acc); e = el(pe + pos); two-pass LN; CLS row = LN(el(cls + pos[0]))
  one judge    |got - ref| <= half a 16-bit ulp of ref (one output rounding) + 2^-15 (|scaled term| + |bias|) (the fp32 rsqrt / exp chain: the form
               gemm_probes.act_bound uses) [+ 2 E for the slot pool].  Nothing in it comes from a kernel's output.
               Where a reference rounds an intermediate to 16 bits (silu / res forms), an fp32 value within that slack of a rounding tie may land on
               either side: the reference is evaluated for both and the nearer one counts.
               E (slot pool, float64, per case): elements of the rotated row within the slack of a 16-bit tie may flip by one ulp; with the fp32
               dot product's own 2^-20 sum_d |x_hat_d slot_d| (a 14-deep fixed-order sum) that moves a logit by at most dl, the softmax weights by at
               most a factor e^(2 max dl), and the output by at most (e^(2 max dl) - 1) sum_n p_n |x_hat_n|.  E carries attn_probes.E_FACTOR.
  emulations   plain torch restatements of the three kernels' STRUCTURE (one wave per row, and the clamped, unstored tail rows of the
               4-rows-per-wave form at D = 1024; 8 parts of ceil(n / 8) rows with a local softmax and a merge; K re-indexed (c, ky, j) with j padded 14 -> 16 and the shifted window at the last patch column), each taking
               fault=<name>: tests/test_encode_probes_cpu.py shows that every fault is rejected by a named probe.

Runs on the CPU and on a device; nothing here imports the HIP library."""
import math
from types import SimpleNamespace

import torch

import gemm_probes as GP
from attn_probes import E_FACTOR
from gemm_probes import MIN_NORMAL, P_BITS, SENTINEL, round16, subnormal_step, truncate16

SLACK = GP.ACT_RTOL_SLACK            # 2^-15
POISON = 3e4                         # what a kernel may read past a row's D elements / in a CLS row it must skip (finite in bf16 and fp16)
NPART, NSLOT = 8, 8
DOT_DEPTH = 2.0 ** -20               # 16 x 2^-24: the logit dot product is 8 dot2 steps + 6 reduction levels deep, in a fixed order
RAMP_NATS = 12.0


# ---- the judge ----------------------------------------------------------------------------------------------------------------------------
def half_ulp(ref64, dtype):
    return torch.exp2(torch.floor(torch.log2(ref64.abs().clamp(min=MIN_NORMAL[dtype]))) - P_BITS[dtype])


def bound(ref64, mag64, dtype, E=None):
    b = half_ulp(ref64, dtype) + SLACK * mag64
    if E is not None:
        b = b + E_FACTOR * E
    return torch.clamp(b, min=subnormal_step(dtype))


def _ref(cands, mags, dtype, E=None, **extra):
    """cands: the float64 values the output may be a rounding of (one, or two where an intermediate rounding sits on a tie)"""
    return SimpleNamespace(cands=cands, bounds=[bound(c, m, dtype, E) for c, m in zip(cands, mags)], ref=cands[0], dtype=dtype, **extra)


def ratio_map(got, R):
    g = got.double()
    r = None
    for c, b in zip(R.cands, R.bounds):
        q = torch.nan_to_num((g - c).abs() / b, nan=float("inf"), posinf=float("inf"))
        r = q if r is None else torch.minimum(r, q)
    wide = getattr(R, "wide", None)
    if wide is not None and bool(wide.any()):          # the intermediate's slack spans several 16-bit values: anything between the two ends
        lo, hi = torch.minimum(R.cands[0], R.cands[1]), torch.maximum(R.cands[0], R.cands[1])
        q = torch.clamp(torch.maximum(lo - g, g - hi), min=0.0) / torch.maximum(R.bounds[0], R.bounds[1])
        r = torch.where(wide, torch.minimum(r, torch.nan_to_num(q, nan=float("inf"))), r)
    return r


def error_ratio(got, R):
    """max over the elements of |got - ref| / bound (inf for a NaN)"""
    return float(ratio_map(got, R).max())


def describe(name, got, R):
    r = ratio_map(got, R)
    i = int(torch.argmax(r))
    idx = [int(v) for v in torch.unravel_index(torch.tensor(i), r.shape)]
    g = float(got.double().flatten()[i])
    k = min(range(len(R.cands)), key=lambda q: abs(g - float(R.cands[q].flatten()[i])))            # the nearer candidate
    return (f"{name}: {int((r > 1).sum())} of {r.numel()} elements off; worst at {idx}: got {g:.7g} ref "
            f"{float(R.cands[k].flatten()[i]):.7g} bound {float(R.bounds[k].flatten()[i]):.3g} (error / bound {float(r.flatten()[i]):.3f})")


def outside_unchanged(buf, snap, ld, rows, D, off=0):
    """every 16-bit word of `buf` outside the rows x D window (row stride ld, at element `off`) still equals `snap`"""
    a, b = buf.view(torch.int16), snap.view(torch.int16)
    idx = torch.arange(a.numel(), device=a.device) - off
    inside = (idx >= 0) & (idx < rows * ld) & (idx % ld < D)
    return bool((a[~inside] == b[~inside]).all())


# ---- norms: reference -----------------------------------------------------------------------------------------------------------------------
def _ln64(x64, w64, b64, eps, rms=False):
    n = x64.shape[-1]
    if rms:
        rstd = torch.rsqrt((x64 * x64).sum(-1, keepdim=True) / n + eps)
        sc = x64 * rstd * w64
        return sc, sc.abs()
    mu = x64.sum(-1, keepdim=True) / n
    var = ((x64 - mu) ** 2).sum(-1, keepdim=True) / n
    sc = (x64 - mu) * torch.rsqrt(var + eps) * w64
    return sc + b64, sc.abs() + b64.abs()


def _act64(t, silu):
    return t * torch.sigmoid(t) if silu else t


def norm_reference(x, w, b, eps, dtype, rms=False, silu=False, res=None):
    """x [rows, D] (a view of the 16-bit buffer), w / b [D], res [rows, D] or None -> the judge's reference"""
    ln, mag = _ln64(x.double(), w.double(), None if rms else b.double(), eps, rms)
    if not silu and res is None:
        return _ref([ln], [mag], dtype)
    cands, mags, ends = [], [], []
    for s in (-1.0, 1.0):                   # the 16-bit rounding of the LN output, for an fp32 value at either end of its slack
        t = round16(ln + s * SLACK * mag, dtype, exact=False).double()
        ends.append(t)
        if res is not None:
            t = t + res.double()
        cands.append(_act64(t, silu))
        mags.append(t.abs())
    # where the LN output cancels (|scaled + bias| << |scaled| + |bias|) the slack spans more than two neighbouring 16-bit values
    wide = (ends[1] - ends[0]) > 2.2 * half_ulp(torch.minimum(ends[0].abs(), ends[1].abs()), dtype)
    return _ref(cands, mags, dtype, wide=wide)


# ---- norms: probes ---------------------------------------------------------------------------------------------------------------------------
def ramp_weights(D, dtype, device="cpu"):
    """weight and bias: small integers, the pair distinct for every channel below 251 * 17 (a shifted or repeated chunk shows)"""
    c = torch.arange(D, device=device, dtype=torch.int64)
    return ((c % 251) - 125).double().to(dtype), ((c // 251) - 8).double().to(dtype)


OFFSET_M = 45.0 / 32.0               # not a power of two: the squares of m + spread need more than 24 bits once a few hundred are summed
OFFSET_RATIOS = (0, 4, 32, 256)


def offset_rows(rows, D, dtype, ratio, device="cpu"):
    """row = m +- spread with |m| / std = `ratio` to the nearest spread the element type can express (returned), the +- balanced so that the
    row sum is D m exactly: a two-pass fp32 LayerNorm has exact statistics on it, a one-pass one (sq / D - mean^2) cancels"""
    r = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    c = torch.arange(D, device=device, dtype=torch.int64)[None, :]
    if ratio == 0:
        x = (1 - 2 * ((c + r) % 2)).double()
        return x.to(dtype), 0.0
    u = 2.0 ** -(P_BITS[dtype] - 1)          # ulp in [1, 2)
    k = OFFSET_M / ratio / u                  # the spread in ulps
    if k >= 2:
        k = float(round(k))
        s = k * (1 - 2 * ((c + r) % 2)).double()
        real = OFFSET_M / (k * u)
    else:                                     # below 2 ulps: +-1 ulp on `hot` of the D elements
        hot = max(2, 2 * int(round(k * k * D / 2)))
        hot = min(hot, D)
        j = (c + 3 * r) % D
        s = torch.where(j < hot, (1 - 2 * (j % 2)).double(), torch.zeros((), dtype=torch.float64, device=device))
        real = OFFSET_M / (u * math.sqrt(hot / D))
    x = OFFSET_M + s * u
    out = x.to(dtype)
    assert bool((out.double() == x).all())
    return out, real


def norm_rows(name, rows, D, dtype, device="cpu", ratio=0):
    """the input rows of a norm probe (weights: ramp_weights for every probe)"""
    r = torch.arange(rows, device=device, dtype=torch.int64)[:, None]
    c = torch.arange(D, device=device, dtype=torch.int64)[None, :]
    if name == "onehot":                      # row r hot at (7 r + 3) % D
        return (c == (7 * r + 3) % D).double().to(dtype)
    if name == "balanced":                    # half +2^k, half -2^k (k = r % 5 - 2): mean 0 and variance 4^k exactly
        return ((1 - 2 * ((c + r) % 2)).double() * torch.exp2(((r % 5) - 2).double())).to(dtype)
    if name == "eps":                         # +-2^-10: variance 2^-20, the size of 1e-6 and a tenth of 1e-5
        return (_balanced_sign(r, c) * 2.0 ** -10).to(dtype)
    if name == "offset":
        return offset_rows(rows, D, dtype, ratio, device)[0]
    if name == "ramp":                        # small integers from a hash of (row, channel)
        return (((r * 131 + c * 29 + (r * c) // 5) % 17) - 8).double().to(dtype)
    raise ValueError(name)


def _balanced_sign(r, c):
    """+-1 alternating along the row (as many of each: D is even), the pattern shifted by the row index"""
    return (1 - 2 * ((c + r) % 2)).double()


NORM_PROBES = ("onehot", "balanced", "eps", "offset", "ramp")


def cancel_residual(x, w, b, eps, dtype):
    """a residual that cancels the LN output down to a small integer: res = -el(LN64(x)) + k, k in [-2, 2].  act(el(LN) + res) is then a small
    number next to a large LN value: an LN output that was not rounded to 16 bits before the add leaves its rounding residue in the result"""
    ln, _ = _ln64(x.double(), w.double(), b.double(), eps)
    r = torch.arange(x.shape[0], device=x.device, dtype=torch.int64)[:, None]
    c = torch.arange(x.shape[1], device=x.device, dtype=torch.int64)[None, :]
    return (-round16(ln, dtype, exact=False).double() + ((3 * r + c) % 5 - 2).double()).to(dtype)


def lay_rows(x, pad, dtype, fill, after=4):
    """x [rows, D] -> (flat buffer, view, ld): rows every D + pad elements starting at element 0, `after` guard rows; everything else holds `fill`
    (a number, or "sentinel")"""
    rows, D = x.shape
    ld = D + pad
    buf = torch.zeros((rows + after) * ld, dtype=dtype, device=x.device)
    if fill == "sentinel":
        buf.view(torch.int16).fill_(SENTINEL)
    else:
        buf.fill_(fill)
    win = buf.as_strided((rows, D), (ld, 1), 0)
    win.copy_(x)
    return buf, win, ld


# ---- norms: emulation ------------------------------------------------------------------------------------------------------------------------
NORM_FAULTS = ("eps_dropped", "mean_count", "tail_rows_written", "tail_neighbour_stats", "chunk_shift64", "ldx_ignored", "ldy_ignored",
               "silu_before_round", "res_before_round", "res_after_store")


def emulate_norm(xb, ldx, yb, ldy, w, b, rows, D, eps, dtype, rms=False, silu=False, resb=None, ldres=0, fault=None):
    """norm_kernel / norm1024_kernel in fp32 torch on flat buffers (windows at element 0).  norm_kernel: one wave per row holding chunks
    lane + 64 i of 8 elements; a wave whose row is past the last one returns, so it has no tail rows.  norm1024_kernel<false, 4> (the LayerNorm at
    D == 1024, rows >= 4096, no residual — the routing of launch_layernorm, restated here): 4 rows per wave, the rows past the last one clamped to
    it, normalised and not stored — the two tail faults exist in that form only.  Writes into yb."""
    lx = D if fault == "ldx_ignored" else ldx
    ly = D if fault == "ldy_ignored" else ldy
    x = xb.as_strided((rows, D), (lx, 1), 0).float()
    res = None if resb is None else resb.as_strided((rows, D), (ldres, 1), 0).float().clone()
    wf, bf = w.float(), (None if rms else b.float())
    if fault == "chunk_shift64" and D > 512:
        nch = D // 8
        ch = (torch.arange(D, device=x.device) // 8 + 64) % nch
        idx = ch * 8 + torch.arange(D, device=x.device) % 8
        wf, bf = wf[idx], (None if rms else bf[idx])
    cnt = float(D)
    if fault == "mean_count":
        cnt = float(512 * -(-D // 512))       # every lane's 8 chunks counted, present or not
    e = 0.0 if fault == "eps_dropped" else eps
    if rms:
        mean = torch.zeros((rows, 1), dtype=torch.float32, device=x.device)
        rstd = torch.rsqrt((x * x).sum(-1, keepdim=True) / cnt + e)
    else:
        mean = x.sum(-1, keepdim=True) / cnt
        rstd = torch.rsqrt(((x - mean) ** 2).sum(-1, keepdim=True) / cnt + e)
    wide1024 = D == 1024 and rows >= 4096 and resb is None and not rms          # launch_layernorm's routing to norm1024_kernel<false, 4>
    if fault == "tail_neighbour_stats" and wide1024 and rows % 4 != 1:
        mean, rstd = mean.clone(), rstd.clone()
        mean[rows - 1], rstd[rows - 1] = mean[rows - 2], rstd[rows - 2]
    o = (x - mean) * rstd * wf
    if not rms:
        o = o + bf
    if res is not None:
        if fault == "res_after_store" and resb is yb:
            res = o.to(dtype).float()                       # the store of LN(x) reached memory first
        t = (o if fault == "res_before_round" else o.to(dtype).float()) + res
        o = t * torch.sigmoid(t) if silu else t
    elif silu:
        t = o if fault == "silu_before_round" else o.to(dtype).float()
        o = t * torch.sigmoid(t)
    y = o.to(dtype)
    nrows = rows
    if fault == "tail_rows_written" and wide1024 and rows % 4:
        extra = 4 - rows % 4
        y = torch.cat([y, y[-1:].expand(extra, D)])
        nrows = rows + extra
    yb.as_strided((nrows, D), (ly, 1), 0).copy_(y)
    return yb


# ---- slot pool: reference ------------------------------------------------------------------------------------------------------------------
def rope_tables(n, D, base=10000.0, device="cpu"):
    """the engine's tables (trace_ctx_finalize): fp32 inv_freq, fp32 angle, cos / sin of that angle in double, stored as fp32 [n, D / 2]"""
    pw = torch.pow(torch.tensor(float(base), dtype=torch.float64), (torch.arange(0, D, 2, dtype=torch.float32) / D).double()).float()
    inv = (torch.ones((), dtype=torch.float32) / pw)
    ang = (torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]).double()
    return ang.cos().float().to(device), ang.sin().float().to(device)


def identity_tables(n, D, device="cpu"):
    return torch.ones((n, D // 2), dtype=torch.float32, device=device), torch.zeros((n, D // 2), dtype=torch.float32, device=device)


def _rotate64(xh, mg, cos_t, sin_t):
    H2 = xh.shape[-1] // 2
    c, s = cos_t.double()[None], sin_t.double()[None]
    a, b, ma, mb = xh[..., :H2], xh[..., H2:], mg[..., :H2], mg[..., H2:]
    return (torch.cat([a * c - b * s, b * c + a * s], -1), torch.cat([ma * c.abs() + mb * s.abs(), mb * c.abs() + ma * s.abs()], -1))


def slot_reference(feats, ln_w, ln_b, slots, cos_t, sin_t, eps, dtype, logit_rounding=True):
    """feats [T, n, D] (a view of the 16-bit buffer) -> reference of res [T, 8, D] with the bound's A and E folded in.  logit_rounding=False: the
    plain module (no 16-bit rounding of the rotated row before the logits), for the comparison with the oracle."""
    xh, mg = _ln64(feats.double(), ln_w.double(), ln_b.double(), eps)
    rot, mrot = _rotate64(xh, mg, cos_t, sin_t)
    D = rot.shape[-1]
    r16 = round16(rot, dtype, exact=False).double() if logit_rounding else rot
    sl = slots.double()
    logits = r16 @ sl                                           # [T, n, 8]
    p = torch.softmax(logits, dim=1)
    ref = torch.einsum("tns,tnd->tsd", p, rot)
    A = torch.einsum("tns,tnd->tsd", p, mrot)
    ulp = 2 * half_ulp(r16, dtype)
    near = (ulp / 2 - (rot - r16).abs()) <= SLACK * mrot       # within the fp32 slack of a rounding tie
    dl = (near.double() * ulp) @ sl.abs() + DOT_DEPTH * (r16.abs() @ sl.abs())
    E = torch.expm1(2 * dl.amax(1))[:, :, None] * torch.einsum("tns,tnd->tsd", p, rot.abs())
    return _ref([ref], [A], dtype, E, p=p, logits=logits, Eabs=E, rot=rot)


# ---- slot pool: probes ---------------------------------------------------------------------------------------------------------------------
def slot_weights(D, dtype, device="cpu"):
    """LN weight in [1, 1.875] and bias in [-1, 1], steps of 1/8 and 1/4, different in the two halves of the channel axis"""
    d = torch.arange(D, device=device, dtype=torch.int64)
    h = d // (D // 2)
    return (1 + ((3 * d + h) % 8).double() / 8).to(dtype), (((5 * d + 3 * h) % 9 - 4).double() / 4).to(dtype)


def slot_targets(n):
    """patches the pointer slots name: the first and last row of every part, the row each part's prefetch loads last (the last row a wave reaches by
    steps of 4), and patch n - 1"""
    RP = -(-n // NPART)
    t = []
    for g in range(NPART):
        beg, end = g * RP, min(n, (g + 1) * RP)
        if end > beg:
            np_ = end - beg
            t += [beg, end - 1, beg + max(((np_ - 1) // 4) * 4 - 1, 0)]
    t.append(n - 1)
    out = []
    for v in t:
        if v not in out:
            out.append(v)
    return out


def _gauss(shape, seed, device):
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.randn(shape, generator=g, dtype=torch.float32).to(device)


def _onehot_rows(T, n, D, dtype, device, mul=1, add=0):
    t = torch.arange(T, device=device)[:, None, None]
    p = torch.arange(n, device=device)[None, :, None]
    d = torch.arange(D, device=device)[None, None, :]
    return (d == (mul * p + add + 3 * t) % D).double().to(dtype)


def lay_feats(x, layout, dtype):
    """x [T, n, D] -> (buffer, view): "plain" contiguous; "internal" [T, n + 1, D] with a poisoned CLS row before every frame's patches (the
    engine's internal-feats form: frame_stride (n + 1) D, base pointer past the first CLS row); "padded" row_stride D + 64 with poison in the gaps"""
    T, n, D = x.shape
    if layout == "plain":
        buf = x.contiguous().clone().reshape(-1)
        return buf, buf.as_strided((T, n, D), (n * D, D, 1), 0)
    if layout == "internal":
        buf = torch.full((T * (n + 1) * D + 8,), POISON, dtype=dtype, device=x.device)
        v = buf.as_strided((T, n, D), ((n + 1) * D, D, 1), D)
    elif layout == "padded":
        rs = D + 64
        fs = n * rs + 64
        buf = torch.full((T * fs,), POISON, dtype=dtype, device=x.device)
        v = buf.as_strided((T, n, D), (fs, rs, 1), 0)
    else:
        raise ValueError(layout)
    v.copy_(x)
    return buf, v


SLOT_PROBES = ("uniform", "pointer", "ramp", "rope", "offset", "eps", "frames")


def slot_probe(name, T, n, D, dtype, device="cpu", ratio=0, layout=None):
    """-> namespace(feats view, buf, ln_w, ln_b, slots [D, 8], cos_t, sin_t, eps)"""
    w, b = slot_weights(D, dtype, device)
    cos_t, sin_t = identity_tables(n, D, device)
    eps = 1e-6
    slots = torch.zeros((D, NSLOT), dtype=dtype, device=device)
    lay = layout or "plain"
    if name == "uniform":                    # slots = 0: every patch weighs 1 / n; one-hot rows: patch p lives in channel (5 p + 1) % D
        x = _onehot_rows(T, n, D, dtype, device, 5, 1)
    elif name in ("pointer", "frames"):      # slot s = c x the rotated row of its target patch: that patch takes almost all of the weight
        x = _gauss((T, n, D), 11 + n + D, device).to(dtype)
        if name == "frames":
            lay = layout or "internal"
        tg = slot_targets(n)
        xh, mg = _ln64(x[0].double(), w.double(), b.double(), eps)
        rot, _ = _rotate64(xh[None], mg[None], cos_t, sin_t)
        for s in range(NSLOT):
            tp = tg[(s + 0) % len(tg)] if name == "pointer" else tg[(3 * s + 1) % len(tg)]
            r = rot[0, tp]
            slots[:, s] = (r * (16.0 / float((r * r).sum()))).to(dtype)
    elif name == "ramp":                     # channel 3 carries a ramp over the patches; slot s reads it with sign (-1)^s: logits span ~12 nats
        g = _gauss((T, n, D), 23 + n + D, device)
        g[:, :, 3] = 4.0 * (torch.arange(n, device=device, dtype=torch.float32) / max(n - 1, 1) - 0.5)[None, :]
        x = g.to(dtype)
        xh, _ = _ln64(x[0].double(), w.double(), b.double(), eps)
        span = float(xh[:, 3].max() - xh[:, 3].min()) if n > 1 else 1.0
        for s in range(NSLOT):
            slots[3, s] = (1 - 2 * (s % 2)) * RAMP_NATS / max(span, 1e-3)
    elif name == "rope":                     # real tables, one-hot rows: the output names the pair (d, d + D / 2), the sign of sin and the position
        x = _onehot_rows(T, n, D, dtype, device, 7, 2)
        cos_t, sin_t = rope_tables(n, D, device=device)
        w, b = torch.ones(D, dtype=dtype, device=device), torch.zeros(D, dtype=dtype, device=device)
        tg = slot_targets(n)
        xh, mg = _ln64(x[0].double(), w.double(), b.double(), eps)
        rot, _ = _rotate64(xh[None], mg[None], cos_t, sin_t)
        for s in range(4, NSLOT):            # slots 0..3 stay zero (uniform weights), 4..7 point
            r = rot[0, tg[(s * 2) % len(tg)]]
            slots[:, s] = (r * (16.0 / float((r * r).sum()))).to(dtype)
    elif name == "offset":
        rows, real = offset_rows(T * n, D, dtype, ratio, device)
        x = rows.reshape(T, n, D)
        slots = (_gauss((D, NSLOT), 5 + D, device) * (2.0 / math.sqrt(D))).to(dtype)
    elif name == "eps":
        r = torch.arange(T * n, device=device, dtype=torch.int64)[:, None]
        c = torch.arange(D, device=device, dtype=torch.int64)[None, :]
        x = (_balanced_sign(r, c) * 2.0 ** -10).to(dtype).reshape(T, n, D)
        slots = (_gauss((D, NSLOT), 7 + D, device) * (2.0 / math.sqrt(D))).to(dtype)
    else:
        raise ValueError(name)
    buf, v = lay_feats(x, lay, dtype)
    return SimpleNamespace(name=name, feats=v, buf=buf, ln_w=w, ln_b=b, slots=slots, cos_t=cos_t, sin_t=sin_t, eps=eps, dtype=dtype, T=T, n=n, D=D,
                           ratio=ratio, layout=lay)


def slot_probe_reference(pr):
    return slot_reference(pr.feats, pr.ln_w, pr.ln_b, pr.slots, pr.cos_t, pr.sin_t, pr.eps, pr.dtype)


# ---- slot pool: emulation ------------------------------------------------------------------------------------------------------------------
SLOT_FAULTS = ("part_drops_last_row", "clamped_row_counted", "empty_part_contributes", "merge_no_rescale", "merge_other_den", "softmax_over_slots",
               "rope_adjacent_pairs", "sin_sign", "position_off_by_one", "eps_dropped", "eps_1e-5", "idle_lanes_contribute", "row_stride_ignored",
               "frame_stride_ignored", "ln_second_half_from_first")


def _lane_sums(a, b):
    """sum_d a_d b_d over the last axis in the kernel's order: lane l owns d in [8 l, 8 l + 8) and D / 2 + [8 l, 8 l + 8) and adds its 8 element pairs
    one dot2 at a time (two exact products and the accumulator, rounded once to fp32), then the 64 lanes are added as a tree (6 levels, fp32)"""
    D = a.shape[-1]
    H2, NL = D // 2, D // 16
    pr = (a.double() * b.double())
    pr = torch.cat([pr[..., :H2].reshape(*a.shape[:-1], NL, 8), pr[..., H2:].reshape(*a.shape[:-1], NL, 8)], -1)      # [.., lane, 16]
    acc = torch.zeros(pr.shape[:-1], dtype=torch.float32, device=a.device)
    for j in range(8):
        acc = (acc.double() + pr[..., 2 * j] + pr[..., 2 * j + 1]).float()
    if NL < 64:
        acc = torch.cat([acc, torch.zeros((*acc.shape[:-1], 64 - NL), dtype=torch.float32, device=a.device)], -1)
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc


def emulate_slot_pool(pr, fault=None):
    """slot_pool_part_kernel + slot_pool_merge_kernel in fp32 torch: 8 parts of RP = ceil(n / 8) patch rows, one-pass LN statistics, the rotated row
    rounded to 16 bits for the logits, a local softmax per part (max, sum, weighted sums against the local max), the merge by exp(m_g - M)."""
    T, n, D, dtype = pr.T, pr.n, pr.D, pr.dtype
    H2, NL = D // 2, D // 16
    fs, rs, off = pr.feats.stride(0) if T > 1 else 0, pr.feats.stride(1), pr.feats.storage_offset()
    if fault == "row_stride_ignored":
        rs = D
    if fault == "frame_stride_ignored":
        fs = n * rs
    need = off + (T - 1) * fs + (n - 1) * rs + D
    buf = pr.buf if need <= pr.buf.numel() else torch.cat([pr.buf, torch.zeros(need - pr.buf.numel(), dtype=dtype, device=pr.buf.device)])
    x = buf.as_strided((T, n, D), (fs, rs, 1), off).float()
    w, b = pr.ln_w.float().clone(), pr.ln_b.float().clone()
    if fault == "ln_second_half_from_first":
        w[H2:], b[H2:] = w[:H2], b[:H2]
    eps = {"eps_dropped": 0.0, "eps_1e-5": 1e-5}.get(fault, pr.eps)
    sm, sq = _lane_sums(x, torch.ones_like(x)), _lane_sums(x, x)
    if fault == "idle_lanes_contribute" and NL < 64:            # lanes >= D / 16 hold lane 0's 16 features and add them again
        l0 = torch.cat([x[..., :8], x[..., H2:H2 + 8]], -1)
        sm, sq = sm + (64 - NL) * l0.sum(-1, keepdim=True), sq + (64 - NL) * (l0 * l0).sum(-1, keepdim=True)
    mean = sm / D
    rstd = torch.rsqrt(torch.clamp(sq / D - mean * mean, min=0.0) + eps)
    xh = (x - mean) * rstd * w + b
    cos_t, sin_t = pr.cos_t.float(), pr.sin_t.float()
    if fault == "position_off_by_one":
        cos_t, sin_t = torch.roll(cos_t, -1, 0), torch.roll(sin_t, -1, 0)
    if fault == "sin_sign":
        sin_t = -sin_t
    if fault == "rope_adjacent_pairs":
        a, bb = xh[..., 0::2], xh[..., 1::2]
        rot = torch.stack([a * cos_t - bb * sin_t, bb * cos_t + a * sin_t], -1).reshape(T, n, D)
    else:
        a, bb = xh[..., :H2], xh[..., H2:]
        rot = torch.cat([a * cos_t - bb * sin_t, bb * cos_t + a * sin_t], -1)
    logits = rot.to(dtype).float() @ pr.slots.float()            # [T, n, 8]
    if fault == "softmax_over_slots":
        p = torch.softmax(logits, dim=2)
        return (torch.einsum("tns,tnd->tsd", p, rot) / p.sum(1)[:, :, None]).to(dtype)
    RP = -(-n // NPART)
    pm = torch.full((T, NPART, NSLOT), -1e30, dtype=torch.float32, device=x.device)
    pl = torch.zeros((T, NPART, NSLOT), dtype=torch.float32, device=x.device)
    pres = torch.zeros((T, NPART, NSLOT, D), dtype=torch.float32, device=x.device)
    for g in range(NPART):
        rows = list(range(g * RP, min(n, (g + 1) * RP)))
        if fault == "part_drops_last_row" and rows:
            rows = rows[:-1]
        if fault == "clamped_row_counted" and len(rows) < RP:
            rows = rows + [n - 1]
        if not rows:
            if fault == "empty_part_contributes":
                pm[:, g], pl[:, g] = 0.0, 1.0
            continue
        idx = torch.tensor(rows, device=x.device)
        lg, rr = logits[:, idx], rot[:, idx]
        m = lg.amax(1)
        e = torch.exp(lg - m[:, None])
        pm[:, g], pl[:, g], pres[:, g] = m, e.sum(1), torch.einsum("tns,tnd->tsd", e, rr)
    M = pm.amax(1, keepdim=True)
    wgt = torch.exp(pm - M)
    if fault == "merge_no_rescale":
        wgt = (pm > -1e29).float()
    den = (wgt * pl).sum(1)
    if fault == "merge_other_den":
        den = torch.roll(den, 1, 1)
    return ((wgt / den[:, None])[..., None] * pres).sum(1).to(dtype)


# ---- front end: reference -------------------------------------------------------------------------------------------------------------------
def frontend_reference(frames, W, cls, pos, lw, lb, P, eps, dtype):
    """frames [T, 3, S, S] (16-bit, or fp32: rounded to the element type first), W [D, 3 P P] -> reference of X [T, G G + 1, D]; .pre: the rows
    before the LN (exact where the operands are integers)"""
    T, _, S, _ = frames.shape
    G, D = S // P, W.shape[0]
    f = frames.double() if frames.dtype == dtype else round16(frames.double(), dtype, exact=False).double()
    patches = f.reshape(T, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(T, G * G, 3 * P * P)
    acc = patches @ W.double().t()
    pe = round16(acc, dtype, exact=False).double()
    e = round16(pe + pos.double()[None, 1:], dtype, exact=False).double()
    c = round16(cls.double() + pos.double()[0], dtype, exact=False).double()
    pre = torch.cat([c[None, None].expand(T, 1, D), e], 1)
    ln, mag = _ln64(pre, lw.double(), lb.double(), eps)
    return _ref([ln], [mag], dtype, pre=pre)


# ---- front end: probes ----------------------------------------------------------------------------------------------------------------------
def hash_pixels(T, S, dtype, device="cpu", fp32=False):
    """small integers in [-4, 4] from a hash of (t, c, y, x); fp32: the same as fp32 values"""
    t = torch.arange(T, device=device, dtype=torch.int64)[:, None, None, None]
    c = torch.arange(3, device=device, dtype=torch.int64)[None, :, None, None]
    y = torch.arange(S, device=device, dtype=torch.int64)[None, None, :, None]
    x = torch.arange(S, device=device, dtype=torch.int64)[None, None, None, :]
    h = (t * 7919 + c * 104729 + y * 1299709 + x * 15485863 + (y * x) % 11 + ((y + 3 * c) * (x + 5 * t)) % 13) % 9 - 4
    return h.float() if fp32 else h.double().to(dtype)


def int_pos(G, D, dtype, device="cpu"):
    """integer position rows, distinct per patch (row 0: the CLS row's), and an integer class embedding"""
    p = torch.arange(G * G + 1, device=device, dtype=torch.int64)[:, None]
    n = torch.arange(D, device=device, dtype=torch.int64)[None, :]
    pos = ((p * 7 + n * 3 + (p * n) % 5 + p // 17) % 17 - 8).double()
    cls = ((n[0] * 5) % 11 - 5).double()
    return pos.to(dtype), cls.to(dtype)


def pre_ln_weights(D, dtype, device="cpu"):
    n = torch.arange(D, device=device, dtype=torch.int64)
    return (1 + ((3 * n) % 8).double() / 8).to(dtype), (((5 * n) % 9 - 4).double() / 4).to(dtype)


def pointer_shifts(D, P):
    K = 3 * P * P
    return list(range(0, K, D))


def frontend_probe(name, T, S, P, D, dtype, device="cpu", shift=0, fp32=False):
    """-> namespace(frames, W [D, 3 P P], cls, pos, lw, lb, eps, P)"""
    G, K = S // P, 3 * P * P
    pos, cls = int_pos(G, D, dtype, device)
    lw, lb = pre_ln_weights(D, dtype, device)
    frames = hash_pixels(T, S, dtype, device, fp32)
    n = torch.arange(D, device=device, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=device, dtype=torch.int64)[None, :]
    extra = {}
    if name in ("pointer", "pos", "poison", "round"):      # the weight of channel n is one-hot at k = (n + shift) % (3 P P)
        W = (k == (n + shift) % K).double()
        if name == "pos":                                  # no image: the rows are the position embeddings themselves
            frames = torch.zeros_like(frames)
        if name == "poison":
            # NaN pixels, each of which must stay in its own patch's row.  Per frame: one in the last patch column at j = P - 1 or P - 2 (read through
            # the early, shifted window); one at j = 0 or 1 of the last patch column and one at j = 0 or 1 of patch column 1 — these two are also what
            # the LEFT neighbour's second window loads as its pad columns 14 and 15 (P = 14), where only the zeroing of the pad pixels keeps
            # NaN x (zero pad weight) out of the neighbour's row
            pp, nb = [], []
            for t in range(T):
                q = [(t % 3, (S - 1 - 3 * t) % S, S - 1 - (t % 2))]
                if G >= 2:
                    q.append(((t + 1) % 3, (5 + 3 * t) % S, (G - 1) * P + (t % 2)))
                if G >= 3:
                    q.append(((t + 2) % 3, (P + 2 + t) % S, P + ((t + 1) % 2)))
                for c, y, x in q:
                    frames[t, c, y, x] = float("nan")
                own = [(y // P) * G + x // P for (_, y, x) in q]
                left = [(y // P) * G + x // P - 1 for (_, y, x) in q[1:]]
                assert not set(own) & set(left)
                pp.append(own)
                nb.append(left)
            extra["nan_patch"], extra["nan_left"] = pp, nb
        if name == "round":                                # fp32 pixels that are NOT 16-bit numbers: rounding up and truncating differ
            frames = (hash_pixels(T, S, dtype, device, True).double() * (1 + 3 * 2.0 ** -(P_BITS[dtype] + 2))).float()
    elif name == "count":                                  # all-ones over one patch row (even n) or column (odd n), one hole each
        kc, ky, kj = k // (P * P), (k // P) % P, k % P
        line = n // 2 % P
        ch = (n // (2 * P)) % 3
        on = (kc == ch) & torch.where(n % 2 == 0, ky == line, kj == line)
        hole = torch.where(n % 2 == 0, kj == (n * 5 + 1) % P, ky == (n * 5 + 1) % P)
        W = (on & ~hole).double()
    else:
        raise ValueError(name)
    return SimpleNamespace(name=name, frames=frames, W=W.to(dtype), cls=cls, pos=pos, lw=lw, lb=lb, eps=1e-5, P=P, T=T, S=S, D=D, G=G, dtype=dtype,
                           shift=shift, **extra)


FRONTEND_PROBES = ("pointer", "count", "pos", "poison", "round")


def frontend_probe_reference(pr):
    """the reference with the NaN pixels replaced by 0 (their own patches' rows, listed per frame in pr.nan_patch, are left out of the judgement)"""
    f = torch.nan_to_num(pr.frames, nan=0.0)
    return frontend_reference(f, pr.W, pr.cls, pr.pos, pr.lw, pr.lb, pr.P, pr.eps, pr.dtype)


def frontend_ratio(got, R, pr):
    """error / bound over X [T, G G + 1, D], the NaN pixels' own patch rows excepted (a NaN anywhere else counts as inf)"""
    r = ratio_map(got, R)
    for t, own in enumerate(getattr(pr, "nan_patch", [])):
        for p in own:
            r[t, 1 + p] = 0.0
    return float(r.max())


def nan_rows_ok(got, pr):
    """every NaN pixel's own patch row holds no finite value, and the row of the patch to its left (which loads the pixel as a pad column) only
    finite ones"""
    own = all(not bool(torch.isfinite(got[t, 1 + p]).any()) for t, ps in enumerate(getattr(pr, "nan_patch", [])) for p in ps)
    left = all(bool(torch.isfinite(got[t, 1 + p]).all()) for t, ps in enumerate(getattr(pr, "nan_left", [])) for p in ps)
    return own and left


# ---- front end: emulation -------------------------------------------------------------------------------------------------------------------
FRONTEND_FAULTS = ("pad_as_pixel", "pad_pixel_not_zeroed", "window_not_shifted", "ky_j_swapped", "channel_stride", "last_wg_stores_all_rows", "duplicate_row_stored",
                   "pos_row0_for_patch0", "cls_no_ln", "fp32_truncates")
FRONTEND_GUARD_ROWS = 64


def emulate_frontend(pr, fault=None):
    """patch_pack_kernel + cls_row_kernel + patch_embed_kernel in torch: K re-indexed (c, ky, j) with j padded to 16 (zero weights and zeroed pixels
    in the pad columns), each half row j0 in {0, 8} one 8-pixel window of the flat frame tensor, the window of the last patch column read `ov`
    pixels early and shifted, 64 patches per workgroup with the rows past G G clamped to the last patch and not stored.  Returns the flat X buffer
    [(T (G G + 1) + 64), D], sentinel-filled."""
    T, S, P, D, G, dtype = pr.T, pr.S, pr.P, pr.D, pr.G, pr.dtype
    GG, NT = G * G, G * G + 1
    dev = pr.W.device
    if pr.frames.dtype == dtype:
        f = pr.frames.double()
    elif fault == "fp32_truncates":
        f = truncate16(pr.frames.double(), dtype).double()
    else:
        f = round16(pr.frames.double(), dtype, exact=False).double()
    flat = torch.cat([f.reshape(-1), torch.zeros(16, dtype=torch.float64, device=dev)])
    t = torch.arange(T, device=dev).view(T, 1, 1, 1, 1, 1)
    patch = torch.arange(GG, device=dev).view(1, GG, 1, 1, 1, 1)
    c = torch.arange(3, device=dev).view(1, 1, 3, 1, 1, 1)
    ky = torch.arange(P, device=dev).view(1, 1, 1, P, 1, 1)
    h = torch.arange(2, device=dev).view(1, 1, 1, 1, 2, 1)
    e = torch.arange(8, device=dev).view(1, 1, 1, 1, 1, 8)
    gy, gx = patch // G, patch % G
    ov = torch.clamp(gx * P + 8 * h + 8 - S, min=0)
    cstride = S * S - S if fault == "channel_stride" else S * S
    base = t * 3 * S * S + c * cstride + (gy * P + ky) * S + gx * P + 8 * h - ov
    v = flat[(base + e).clamp(max=flat.numel() - 1)]                                     # [T, GG, 3, P, 2, 8]
    src = e if fault == "window_not_shifted" else e + ov                               # after the shift element e holds window element e + ov
    v = torch.where(src < 8, torch.gather(v, 5, src.clamp(max=7).expand_as(v)), torch.zeros((), dtype=torch.float64, device=dev))
    j = 8 * h + e
    if fault not in ("pad_as_pixel", "pad_pixel_not_zeroed"):      # (pad_pixel_not_zeroed: the pad weights stay zero, and NaN x 0 = NaN)
        v = torch.where(j < P, v, torch.zeros((), dtype=torch.float64, device=dev))
    A = v.reshape(T, GG, 3 * P * 16)
    W4 = pr.W.double().reshape(D, 3, P, P)
    if fault == "ky_j_swapped":
        W4 = W4.transpose(2, 3)
    Wp = torch.zeros((D, 3, P, 16), dtype=torch.float64, device=dev)
    Wp[..., :P] = W4
    if fault == "pad_as_pixel":
        Wp[..., P:] = W4[..., P - 1:P]
    A0 = torch.nan_to_num(A, nan=0.0)
    acc = A0 @ Wp.reshape(D, -1).t()
    nanrow = torch.isnan(A).any(-1)                                                    # a NaN operand makes every product of its row NaN
    acc = torch.where(nanrow[..., None], torch.full((), float("nan"), dtype=torch.float64, device=dev), acc)
    pe = acc.float().to(dtype).float()
    prow = pr.pos.float()[:GG] if fault == "pos_row0_for_patch0" else pr.pos.float()[1:]
    ee = (pe + prow[None]).to(dtype).float()
    ce = (pr.cls.float() + pr.pos.float()[0]).to(dtype).float()

    def ln(xx):
        m = xx.mean(-1, keepdim=True)
        q = ((xx - m) ** 2).mean(-1, keepdim=True)
        return ((xx - m) * torch.rsqrt(q + pr.eps) * pr.lw.float() + pr.lb.float()).to(dtype)

    y = ln(ee)
    crow = ce.to(dtype) if fault == "cls_no_ln" else ln(ce)
    X = torch.zeros((T * NT + FRONTEND_GUARD_ROWS, D), dtype=dtype, device=dev)
    X.view(torch.int16).fill_(SENTINEL)
    Xv = X[:T * NT].view(T, NT, D)
    Xv[:, 0], Xv[:, 1:] = crow, y
    stray = {"last_wg_stores_all_rows": -(-GG // 64) * 64 - GG, "duplicate_row_stored": 1 if GG % 64 else 0}.get(fault, 0)
    for tt in range(T):
        for q in range(stray):
            X[tt * NT + 1 + GG + q] = y[tt, GG - 1]
    return X
