"""Attention probes: inputs on which every key counts, a float64 reference with the mask stated explicitly, and one judge.

Gaussian q, k, v make the softmax nearly flat: an output element is an average of n unit-variance values (rms ~ sqrt(e / n)) and a fixed
absolute tolerance stops noticing a lost key once n is a few hundred.  The probes below keep the signal at the size of the tolerance's
relative part instead:

  uniform   q = 0, V one-hot (V[j, j % hd] = 1): every visible key weighs exactly 1 / n_visible, channel c is count_c / n_visible
  pointer   K Gaussian, q[i] = 3 k[target(i)]: one key takes almost all of the weight, the output is about v[target]
  ramp      scores rise (or fall) by 12 nats from the first to the last visible key along one direction; V one-hot
  poison    (decode) what the kernel reads but must not count holds large finite values

Layout used throughout ("canonical"): q [B, H, nq, hd], k / v [B, KVH, nkv, hd] (H = G * KVH, head h uses kv head h // G), 16-bit tensors exactly as
the kernel gets them; visible bool [B, nq, nkv].  Everything here runs on the CPU as well as on a device; nothing imports the HIP library."""
import math

import torch

RTOL = 2.0 ** -7                  # twice the unit roundoff of a bf16 output (2^-8); the same bound is used on the fp16 library
E_FACTOR = 2.0                    # margin on E for summation order and the hardware exp2 / exp
RAMP_NATS = 12.0
POISON_K_GAIN, POISON_V, POISON_OTHER_SLOT = 4.0, 1e4, 3e4
DECODE_CTX_EDGES = (1, 31, 32, 33, 64, 65, 127, 128, 129)


# ---- masks ------------------------------------------------------------------------------------------------------------------------------
def full_visible(B, nq, nkv, device="cpu"):
    return torch.ones((B, nq, nkv), dtype=torch.bool, device=device)


def causal_visible(B, nq, nkv, device="cpu"):
    """row i of the nq newest rows sees keys 0 .. i + (nkv - nq)"""
    off = nkv - nq
    vis = torch.arange(nkv, device=device)[None, :] <= (torch.arange(nq, device=device)[:, None] + off)
    return vis[None].expand(B, nq, nkv).contiguous()


def decode_visible(pos, max_ctx):
    """pos int [B] (index of the newest key): row b sees keys 0 .. pos[b]"""
    return (torch.arange(max_ctx, device=pos.device)[None, :] <= pos[:, None].long())[:, None, :].contiguous()


# ---- the decode kernel's split geometry, restated ---------------------------------------------------------------------------------------
def decode_nsplit(B):
    """the engine's split count for a decode batch: clamp((40 + B / 2) / B, 1, 16) in integers"""
    return max(1, min(16, (40 + B // 2) // B))


def decode_chunk(ctx, nsplit):
    """positions per split: ceil(ctx / nsplit) rounded up to whole 32-position blocks"""
    return (-(-ctx // nsplit) + 31) // 32 * 32


def decode_contexts(nsplit, max_ctx):
    """the contexts every decode batch has to contain: block edges, split edges, a last split of exactly one key, the full slot"""
    c = list(DECODE_CTX_EDGES) + [32 * nsplit, 32 * nsplit + 1, 32 * (nsplit - 1) + 1 if nsplit > 1 else 1, max_ctx - 1, max_ctx]
    return [min(max(x, 1), max_ctx) for x in c]


def decode_pointer_targets(ctx, nsplit):
    """key positions the heads of a decode row point at: 0, the newest and the one before it, 31 / 32, the first and last position of the last
    non-empty split and of a middle split, and of the last four 32-position blocks (consecutive blocks belong to different waves)"""
    pos = ctx - 1
    chunk = decode_chunk(ctx, nsplit)
    last = pos // chunk                                   # last non-empty split
    mid = last // 2
    t = [0, pos, pos - 1, 31, 32, last * chunk, pos, mid * chunk, min(mid * chunk + chunk - 1, pos)]
    for w in range(4):
        blk = pos // 32 - w
        if blk >= 0:
            t += [blk * 32, min(blk * 32 + 31, pos)]
    out = []
    for x in t:
        x = min(max(x, 0), pos)
        if x not in out:
            out.append(x)
    return out


# ---- probe inputs -----------------------------------------------------------------------------------------------------------------------
def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(int(seed))


def _randn(shape, seed, device):
    return torch.randn(shape, generator=_gen(seed, device), device=device, dtype=torch.float32)


def onehot_v(B, KVH, nkv, hd, dtype, device="cpu"):
    v = torch.zeros((B, KVH, nkv, hd), dtype=dtype, device=device)
    j = torch.arange(nkv, device=device)
    v[:, :, j, j % hd] = 1
    return v


def probe_uniform(B, H, KVH, nq, nkv, hd, dtype, seed=0, device="cpu"):
    return (torch.zeros((B, H, nq, hd), dtype=dtype, device=device), _randn((B, KVH, nkv, hd), seed, device).to(dtype),
            onehot_v(B, KVH, nkv, hd, dtype, device))


def probe_pointer(targets, H, KVH, nkv, hd, dtype, seed=0, device="cpu"):
    """targets long [B, H, nq]: the key each query points at.  K, V Gaussian; q[b, h, i] = 3 k[b, h // G, targets[b, h, i]]."""
    B, _, nq = targets.shape
    G = H // KVH
    k = _randn((B, KVH, nkv, hd), seed, device).to(dtype)
    v = _randn((B, KVH, nkv, hd), seed + 1, device).to(dtype)
    bi = torch.arange(B, device=device)[:, None, None]
    gi = (torch.arange(H, device=device) // G)[None, :, None]
    q = 3.0 * k[bi, gi, targets.to(device)].float()                                           # [B, H, nq, hd]
    return q.to(dtype), k, v


def probe_ramp(n_visible, B, H, KVH, nq, nkv, hd, scale, dtype, rising=True, seed=0, device="cpu"):
    """n_visible long [B]: keys 0 .. n_visible[b] - 1 carry the ramp (the rest of k is zero): k[j] = (j / n) b e, q = a e with a b |e|^2 scale = 12."""
    e = _randn((hd,), seed, device)
    e = e / e.norm()
    a = math.sqrt(RAMP_NATS / scale)
    n = n_visible.to(device).double().clamp(min=1)[:, None]
    j = torch.arange(nkv, device=device).double()[None, :]
    frac = (j / n) if rising else (1.0 - j / n)
    frac = torch.where(j < n, frac, torch.zeros_like(frac)).float()                           # [B, nkv]
    k = (frac[:, None, :, None] * (a * e)[None, None, None, :]).expand(B, KVH, nkv, hd).contiguous().to(dtype)
    q = (a * e)[None, None, None, :].expand(B, H, nq, hd).contiguous().to(dtype)
    return q, k, onehot_v(B, KVH, nkv, hd, dtype, device)


def causal_pointer_targets(B, H, nq, nkv, device="cpu"):
    """heads 0..2 of every group of 4 point near the diagonal (row i at i + off - ((i + h) % 3): every key of the new rows is some head's diagonal,
    the key before it and the one before that), head 3 at a position spread over everything the row sees (the past of an append included)"""
    off = nkv - nq
    i = torch.arange(nq, device=device)[None, :]
    h = torch.arange(H, device=device)[:, None]
    near = i + off - ((i + h) % 3)
    spread = (i * 7919 + h * 104729 + 13) % (i + off + 1)
    t = torch.where((h % 4) == 3, spread, near).clamp(min=0)
    t = torch.minimum(t, i + off)
    return t[None].expand(B, H, nq).contiguous()


def vit_pointer_targets(B, H, n, seed=0, device="cpu"):
    """every (batch, head) gets its own permutation of the keys: each key is exactly one query's target"""
    g = _gen(seed, "cpu")
    return torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(H)]) for _ in range(B)]).to(device)


def decode_pointer_target_tensor(ctxs, H, nsplit, device="cpu"):
    rows = []
    for c in ctxs:
        t = decode_pointer_targets(int(c), nsplit)
        rows.append([t[h % len(t)] for h in range(H)])
    return torch.tensor(rows, dtype=torch.long, device=device)[:, :, None]                   # [B, H, 1]


def poison_decode(q, k, v, pos):
    """in place: cache rows past pos[b] hold K = 4 q of the group's first head and V = 1e4 (finite: the kernel's contract excludes nothing else)"""
    B, H, _, hd = q.shape
    KVH, nkv = k.shape[1], k.shape[2]
    G = H // KVH
    past = (torch.arange(nkv, device=k.device)[None, :] > pos[:, None].long())[:, None, :, None]        # [B, 1, nkv, 1]
    kp = (POISON_K_GAIN * q.float()[:, ::G, 0, :])[:, :, None, :].to(k.dtype)                            # [B, KVH, 1, hd]
    k.copy_(torch.where(past, kp.expand_as(k), k))
    v.copy_(torch.where(past, torch.full_like(v, POISON_V), v))
    return k, v


# ---- float64 reference, its companion A and the reference-side error E --------------------------------------------------------------------
class Ref:
    """ref, A float64 [B, H, nq, hd]; E float (largest error of the float32 restatement of the kernels' roundings against ref)"""

    def __init__(self, ref, A, E, q, k, visible, scale):
        self.ref, self.A, self.E = ref, A, E
        self._q, self._k, self._vis, self._scale = q, k, visible, scale

    def weights(self, b, h, i):
        G = self._q.shape[1] // self._k.shape[1]
        s = (self._k[b, h // G].double() @ self._q[b, h, i].double()) * self._scale
        s = s.masked_fill(~self._vis[b, i], float("-inf"))
        return torch.softmax(s, -1)


def _round(x, dtype):
    return x.to(dtype).float()


def reference(q, k, v, visible, scale, fold_scale):
    """float64 attention of the 16-bit inputs under `visible`, A = sum_j w_j |v_j|, and E: the largest absolute error against it of a float32
    restatement of the roundings the kernels document — fold_scale: scale * log2(e) folded into a 16-bit copy of q and base-2 exponentials (the
    prefill-shaped kernels); else an fp32 scale and exp (decode); in both P is rounded to the element type before PV, the sums are fp32 and the
    output is rounded to the element type.  Computed in batch chunks."""
    B, H, nq, hd = q.shape
    KVH, nkv = k.shape[1], k.shape[2]
    G = H // KVH
    dtype = q.dtype
    ref = torch.empty((B, H, nq, hd), dtype=torch.float64, device=q.device)
    A = torch.empty_like(ref)
    E = 0.0
    step = max(1, min(B, (1 << 26) // max(1, H * nq * nkv)))
    for b0 in range(0, B, step):
        sl = slice(b0, min(B, b0 + step))
        nb = sl.stop - sl.start
        vis = visible[sl][:, None, None]                                                                 # [b, 1, 1, nq, nkv]
        q64 = q[sl].double().view(nb, KVH, G, nq, hd)
        k64, v64 = k[sl].double(), v[sl].double()
        s = torch.einsum("bkgqd,bkjd->bkgqj", q64, k64) * scale
        w = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
        r = torch.einsum("bkgqj,bkjd->bkgqd", w, v64)
        ref[sl] = r.view(nb, H, nq, hd)
        A[sl] = torch.einsum("bkgqj,bkjd->bkgqd", w, v64.abs()).view(nb, H, nq, hd)
        del s, w
        # the float32 restatement
        qf, kf, vf = q[sl].float().view(nb, KVH, G, nq, hd), k[sl].float(), v[sl].float()
        if fold_scale:
            s32 = torch.einsum("bkgqd,bkjd->bkgqj", _round(qf * (scale * 1.4426950408889634), dtype), kf)
        else:
            s32 = torch.einsum("bkgqd,bkjd->bkgqj", qf, kf) * scale
        s32 = s32.masked_fill(~vis, float("-inf"))
        m = s32.amax(-1, keepdim=True)
        p = torch.exp2(s32 - m) if fold_scale else torch.exp(s32 - m)
        l = p.sum(-1, keepdim=True)
        o = _round(torch.einsum("bkgqj,bkjd->bkgqd", _round(p, dtype), vf) / l, dtype)
        E = max(E, float((o.double() - r).abs().max()))
    return Ref(ref, A, E, q, k, visible, scale)


# ---- the judges ------------------------------------------------------------------------------------------------------------------------
def _describe(name, got, r, err, tol):
    bad = ~(err <= tol)                                   # NaN counts as bad
    ratio = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    b, h, i, c = [int(x) for x in torch.unravel_index(torch.argmax(ratio), ratio.shape)]
    w = r.weights(b, h, i)
    top = torch.topk(w, min(4, w.numel()))
    keys = ", ".join(f"{int(p)}: {float(x):.3g}" for x, p in zip(top.values, top.indices))
    nvis = int(r._vis[b, i].sum())
    return (f"{name}: {int(bad.sum())} of {bad.numel()} elements off; worst (batch {b}, head {h}, row {i}, channel {c}): got {float(got[b, h, i, c]):.6g} "
            f"ref {float(r.ref[b, h, i, c]):.6g} err {float(err[b, h, i, c]):.3g} bound {float(tol[b, h, i, c]):.3g}; the row sees {nvis} keys, its weight "
            f"sits on {{{keys}}}; E = {r.E:.3g}")


def attention_error_ratio(got, r, factor=E_FACTOR):
    """max over the elements of |got - ref| / (2^-7 (|ref| + A) + factor E), and max |got - ref|"""
    err = (got.double() - r.ref).abs()
    tol = RTOL * (r.ref.abs() + r.A) + factor * r.E
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)              # (0 / 0: a single visible key gives E = 0 and exact zeros)
    return float(torch.nan_to_num(ratio, nan=float("inf")).max()), float(torch.nan_to_num(err, nan=float("inf")).max())


def attention_close(got, r, name="attention", factor=E_FACTOR):
    """(ok, message): per element |got - ref| <= 2^-7 (|ref| + A) + 2 E, and every value finite"""
    g = got.double()
    err = (g - r.ref).abs()
    tol = RTOL * (r.ref.abs() + r.A) + factor * r.E
    ok = bool((err <= tol).all()) and bool(torch.isfinite(g).all())
    return ok, ("" if ok else _describe(name, g, r, err, tol))


def assert_attention_close(got, r, name="attention", factor=E_FACTOR):
    ok, msg = attention_close(got, r, name, factor)
    assert ok, msg


def uniform_close(got, r, name="uniform"):
    """the uniform probe's own bound: rtol 2^-7 and no absolute term on the channels that hold a key, exactly 0 on those that hold none"""
    g = got.double()
    err = (g - r.ref).abs()
    tol = RTOL * r.ref.abs()
    ok = bool((err <= tol).all()) and bool(torch.isfinite(g).all())
    return ok, ("" if ok else _describe(name, g, r, err, tol))


def assert_uniform_close(got, r, name="uniform"):
    ok, msg = uniform_close(got, r, name)
    assert ok, msg


# ---- 16-bit helpers -----------------------------------------------------------------------------------------------------------------------
def ulp_distance(a, b):
    """distance in units in the last place between two tensors of one 16-bit float type (0 = bit-equal up to the sign of zero)"""
    def key(x):
        u = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(u < 0, -(u & 0x7fff), u)
    return (key(a) - key(b)).abs()
