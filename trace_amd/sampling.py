"""Sampling parameters and the host-side statement of the device sampler (trace_amd/csrc/sample.h).

`SamplingParams` is what Engine.decode / generate / generate_stream and evaluate_videos take.  `sample_row_ref` restates the device
sampler in float32 numpy, operation by operation (the same exp polynomial, the same run sums and Hillis-Steele scan, the same rank
arithmetic), so it returns the device's id bit for bit; it also serves as the host path for the parameter combinations the device does not
take (top_k > 1024, or top_k = 0 with top_p < 1 or with min_p / typical_p / epsilon_cutoff / eta_cutoff armed), where it applies the same rules.  `philox_uniform` is the RNG contract in numpy.
`token_logprob_ref` restates the per-token log-probability (sample.h token_logprob_row) the same way: the device's float bits.
`LogitsParams` / `process_row_ref`: the logits processors of the decode step (repetition penalty, no-repeat n-grams, min_new_tokens:
trace_amd/csrc/logits.h) and their float32 restatement, again bit for bit.
`Constraints` / `constrain_row_ref` / `stop_match_ref` / `ends_stopped`: bad words, suppressed ids and stop sequences of the decode step
(trace_amd/csrc/constrain.h) and their restatement; only -inf is stored, so the device is bit for bit by construction.
`score_logprob_ref`: the log-probability of a GIVEN id as the scoring kernels (trace_amd/csrc/score.hip) form it from column-tile partial sums."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

DEVICE_MAX_K = 1024           # sample.h SAMPLE_MAX_K
_THREADS = 256                # sample.h SAMPLE_THREADS
_F = np.float32


@dataclass(frozen=True)
class SamplingParams:
    """HF sampling warpers in HF's order: temperature, top_k (50 = HF's default; 0 = off), top_p (1.0 = off), min_p (0 = off), typical_p
    (1.0 = off), epsilon_cutoff (0 = off), eta_cutoff (0 = off); None for one of the last four is stored as its off value.  seed: 64-bit Philox key; the counter of row b at decode step s is
    (s, 0, b, 0).  temperature <= 0 means greedy."""
    temperature: float = 1.0
    top_k: int = 50
    top_p: float = 1.0
    seed: int = 0
    min_p: float = 0.0
    typical_p: float = 1.0
    epsilon_cutoff: float = 0.0
    eta_cutoff: float = 0.0

    def __post_init__(self):
        for name, off in (("min_p", 0.0), ("typical_p", 1.0), ("epsilon_cutoff", 0.0), ("eta_cutoff", 0.0)):
            if getattr(self, name) is None:                       # HF's other spelling of "off"
                object.__setattr__(self, name, off)
        check_sampling(self.temperature, self.top_k, self.top_p, self.min_p, self.typical_p, self.epsilon_cutoff, self.eta_cutoff)
        if not 0 <= int(self.seed) < 1 << 64:
            raise ValueError(f"seed must be a 64-bit unsigned integer, got {self.seed}")

    @property
    def greedy(self) -> bool:
        return self.temperature <= 0

    @property
    def warpers(self) -> tuple:
        """(min_p, typical_p, epsilon_cutoff, eta_cutoff): what sample_row_ref takes behind u and info"""
        return float(self.min_p), float(self.typical_p), float(self.epsilon_cutoff), float(self.eta_cutoff)

    @property
    def warpers_armed(self) -> bool:
        return self.min_p > 0 or self.typical_p < 1.0 or self.epsilon_cutoff > 0 or self.eta_cutoff > 0

    @property
    def on_device(self) -> bool:
        """the device sampler's domain: top_k in [1, 1024] with anything else, or top_k = 0 with top_p = 1 and min_p / typical_p /
        epsilon_cutoff / eta_cutoff off"""
        return 1 <= self.top_k <= DEVICE_MAX_K or (self.top_k == 0 and self.top_p >= 1.0 and not self.warpers_armed)


def check_sampling(temperature, top_k, top_p, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0) -> None:
    """HF's own argument checks (Temperature / TopK / TopP / MinP / Typical / Epsilon / Eta LogitsWarper), HF's wording; the off values
    (None, or min_p 0, typical_p 1.0, the cutoffs 0) pass"""
    if min_p is not None and not 0.0 <= float(min_p) <= 1.0:
        raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {min_p}")
    if typical_p is not None and float(typical_p) != 1.0 and not 0.0 < float(typical_p) < 1.0:
        raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {typical_p}")
    for name, v in (("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)):
        if v is not None and float(v) != 0.0 and not 0.0 < float(v) < 1.0:
            raise ValueError(f"`{name}` has to be a float > 0 and < 1, but is {v}")
    t = float(temperature)
    if t != t or t in (float("inf"), float("-inf")):
        raise ValueError(f"`temperature` has to be a finite float, but is {temperature}")
    if not isinstance(top_k, (int, np.integer)) or isinstance(top_k, bool) or top_k < 0:
        raise ValueError(f"`top_k` has to be a non-negative integer, but is {top_k}")
    p = float(top_p)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"`top_p` has to be a float > 0 and <= 1, but is {top_p}")


# ---- RNG: Philox4x32-10, word 0 of counter (c0, c1, c2, c3) under the 64-bit key (vectorised over numpy arrays) ----
def philox_x(seed, c0, c1, c2, c3):
    seed = np.asarray(seed, np.uint64)
    k0 = (seed & np.uint64(0xFFFFFFFF)).astype(np.uint64)
    k1 = (seed >> np.uint64(32)).astype(np.uint64)
    c = [np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF) for v in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c, k0)[:4]
    k0, k1 = np.broadcast_arrays(k0, k1, c0)[:2]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        m0 = np.uint64(0xD2511F53) * c0
        m1 = np.uint64(0xCD9E8D57) * c2
        n0 = (m1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (m0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = m1 & m32, m0 & m32, n0, n2
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return c0.astype(np.uint32)


def philox_uniform(seed, step, row):
    """u in [0, 1) of row `row` at decode step `step` (float32)"""
    x = philox_x(seed, step, 0, row, 0)
    return ((x >> np.uint32(8)).astype(np.float32) * _F(1.0 / 16777216.0)).astype(np.float32)


# ---- the sampler ----
def _sexp(x):
    """sample.h sample_exp: exp(x), x <= 0, every operation rounded in float32"""
    x = np.asarray(x, np.float32)
    out = np.zeros_like(x)
    ok = x > _F(-80.0)
    v = x[ok]
    n = np.rint(v * _F(float.fromhex("0x1.715476p+0")))
    r = v - n * _F(float.fromhex("0x1.62e4p-1"))
    r = r - n * _F(float.fromhex("0x1.7f7d1cp-20"))
    p = np.full_like(v, _F(float.fromhex("0x1.6c16c2p-10")))
    for c in ("0x1.111112p-7", "0x1.555556p-5", "0x1.555556p-3"):
        p = p * r + _F(float.fromhex(c))
    p = p * r + _F(0.5)
    p = p * r + _F(1.0)
    p = p * r + _F(1.0)
    out[ok] = p * np.ldexp(_F(1.0), n.astype(np.int32)).astype(np.float32)
    return out


def _scan(v):
    """Hillis-Steele inclusive scan over 256 values (sample.h sample_scan): v[t] = v[t - d] + v[t]"""
    v = v.copy()
    d = 1
    while d < _THREADS:
        v[d:] = v[:-d] + v[d:]
        d <<= 1
    return v


def _keys(x):
    u = x.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _run_sums(w, per):
    """running sums of w in sample.h's order: runs of `per` per thread, then the scan over the run totals"""
    buf = np.zeros(_THREADS * per, np.float32)
    buf[: len(w)] = w
    runs = np.cumsum(buf.reshape(_THREADS, per), axis=1, dtype=np.float32)
    incl = _scan(runs[:, -1].copy())
    excl = np.concatenate([np.zeros(1, np.float32), incl[:-1]])
    return (excl[:, None] + runs).reshape(-1), incl[-1]


class _Kept:
    """What top_p leaves and the warpers behind it narrow (sample.h sample_warp): the sorted candidates [lo, hi) followed by mk tokens of
    the tie block.  xo / ko / w: the candidates' values, keys and weights in (value desc, id asc) order, cw their running sums; tv / wt the
    tie block's value and weight; per: the candidates per thread of the fixed-order sums (4 on the device)."""

    def __init__(self, xo, ko, cw, hi, mk, tv, wt, M, per):
        self.xo, self.ko, self.cw, self.lo, self.hi, self.mk, self.tv, self.wt, self.M, self.per = xo, ko, cw, 0, hi, mk, tv, wt, M, per
        self.w = _sexp(xo - M)
        self.margins = {}

    def z(self):
        cw, lo, hi = self.cw, self.lo, self.hi
        return ((cw[hi - 1] if hi else _F(0.0)) - (cw[lo - 1] if lo else _F(0.0))) + _F(self.mk) * self.wt

    def cut(self, thr, stage):
        """sample_cut: the first candidate of [lo, hi) below thr whose key is not the top's ends the candidates; the tie block follows if
        none went and it is the top itself or its weight is not below thr"""
        lo, hi, w = self.lo, self.hi, self.w
        low = (self.ko[lo:hi] != self.ko[lo]) if lo < hi else np.zeros(0, bool)
        bad = np.nonzero(low & (w[lo:hi] < thr))[0]
        r = lo + int(bad[0]) if len(bad) else hi
        dist = np.abs(w[lo:hi][low] - thr)
        if self.mk > 0 and lo < hi:
            dist = np.append(dist, abs(self.wt - thr))
        self.margins[stage] = float(dist.min() / thr) if len(dist) else np.inf
        if r < hi or (lo < hi and self.wt < thr):
            self.mk = 0
        self.hi = r

    def entropy(self, Z):
        """sample_entropy: log Z - (sum w (x - M)) / Z, the sum in runs of `per` per thread over the candidates' slots (0 outside [lo, hi)
        and where the weight is 0), then the scan, then the tie block's mk (wt (tv - M))"""
        with np.errstate(invalid="ignore"):
            e = np.where(self.w > 0, self.w * (self.xo - self.M), _F(0.0)).astype(np.float32)
            te = self.wt * (self.tv - self.M) if self.wt > 0 else _F(0.0)
        e[: self.lo] = 0
        e[self.hi:] = 0
        _, D = _run_sums(e, self.per)
        D = D + _F(self.mk) * te
        return _slog(np.array([Z], np.float32))[0] - D / Z

    def typical(self, tp):
        """sample_typical: s_j = (log Z - (x_j - M)) - H (non-decreasing), key a_j = |s_j|; a* = the smallest key v with
        mass{-v <= s <= v} >= tp Z, the mass as a difference of two running sums (+ the tie block's); keep a <= a*.
        This is the device's formulation restated, not a second algorithm: agreement with the device alone would not catch a shared misreading
        of HF's rule.  That rests on the comparison with transformers' own TypicalLogitsWarper (tests/test_sampling_warpers_cpu.py) and on the
        distribution test on the device (tests/test_gpu_sampling_warpers.py)."""
        hi, mk, cw = self.hi, self.mk, self.cw
        mkwt = _F(mk) * self.wt
        Z = self.z()
        H = self.entropy(Z)
        lZ = _slog(np.array([Z], np.float32))[0]
        nlp = (lZ - (self.xo[:hi] - self.M)).astype(np.float32)
        sk = (nlp - H).astype(np.float32)
        nlp_t = lZ - (self.tv - self.M)
        st = nlp_t - H
        tpZ = tp * Z
        s_all = np.append(sk, st).astype(np.float32) if mk > 0 else sk
        v = np.abs(s_all)
        l, r = np.searchsorted(sk, -v, "left"), np.searchsorted(sk, v, "right")
        cw0 = np.concatenate([np.zeros(1, np.float32), cw[:hi]])
        mass = (cw0[r] - cw0[l]).astype(np.float32)
        if mk > 0:
            mass = np.where(st <= v, mass + mkwt, mass).astype(np.float32)
        ok = mass >= tpZ
        a = v[ok].min() if ok.any() else _F(np.inf)
        # margins: every mass against tp Z; every key against a*, relative to the two terms its s was formed from (tokens of a*'s own value aside)
        x_all = np.append(self.xo[:hi], self.tv) if mk > 0 else self.xo[:hi]
        scale = (np.append(nlp, nlp_t) if mk > 0 else nlp) + H
        other = x_all != x_all[np.nonzero(ok & (v == a))[0][0]] if ok.any() else np.zeros(len(v), bool)
        da = (np.abs(v - a) / scale)[other]
        self.margins["typical_p"] = float(min((np.abs(mass - tpZ) / tpZ).min(), da.min() if len(da) else np.inf))
        l, r = int(np.searchsorted(sk, -a, "left")), int(np.searchsorted(sk, a, "right"))
        mt = mk if mk > 0 and st <= a else 0
        if l < r or mt > 0:
            self.lo, self.hi, self.mk = l, r, mt


def sample_row_ref(row, temperature, top_k, top_p, u, info=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """The device sampler on one head row (float32 [n]): the chosen offset in [0, n).  `info` (a dict, optional) receives the kept
    offsets in walk order ('kept'), the running sums ('cum'), and the target ('target') — for tests; behind top_k also 'stages': the kept
    offsets after top_p and after each armed warper, 'margins': per stage the smallest relative distance of a compared quantity to its
    threshold over the stage's keep-or-drop decisions, and 'margin': the smallest of those."""
    x = np.asarray(row, np.float32) / _F(temperature)
    n = len(x)
    u = _F(u)
    p = _F(top_p)
    armed = min_p > 0 or typical_p < 1.0 or epsilon_cutoff > 0 or eta_cutoff > 0
    if top_k <= 0 and p >= _F(1.0) and not armed:
        M = x.max()
        w = _sexp(x - M)
        C = (n + _THREADS - 1) // _THREADS
        buf = np.zeros(_THREADS * C, np.float32)
        buf[:n] = w
        runs = np.cumsum(buf.reshape(_THREADS, C), axis=1, dtype=np.float32)
        incl = _scan(runs[:, -1].copy())
        excl = np.concatenate([np.zeros(1, np.float32), incl[:-1]])
        run = (excl[:, None] + runs).reshape(-1)[:n]
        target = u * incl[-1]
        hit = np.nonzero(run > target)[0]
        if info is not None:
            info.update(kept=np.arange(n), cum=run, target=target, total=incl[-1])
        return int(hit[0]) if len(hit) else n - 1
    k = n if top_k <= 0 else min(int(top_k), n)
    keys = _keys(x)
    theta = np.sort(keys)[::-1][k - 1]
    above = np.nonzero(keys > theta)[0]
    ties = np.nonzero(keys == theta)[0]
    order = above[np.lexsort((above, ~keys[above]))]          # (value desc, id asc)
    na, m = len(order), len(ties)
    tv = x[ties[0]]
    M = x[order[0]] if na else tv
    per = max(4, -(-na // _THREADS))
    cw, _ = _run_sums(_sexp(x[order] - M), per)
    cw = cw[:na]
    A = cw[na - 1] if na else _F(0.0)
    wt = _sexp(np.array([tv - M], np.float32))[0]
    Z = A + _F(m) * wt
    na_keep, mk = na, m
    margins = {}
    if p < _F(1.0):
        pZ = p * Z
        above_mass = np.concatenate([np.zeros(1, np.float32), cw[:-1]]) if na else cw
        bad = np.nonzero(above_mass >= pZ)[0]
        na_keep = int(bad[0]) if len(bad) else na
        dist = np.abs(above_mass[1:] - pZ)
        if na_keep < na:
            mk = 0
        else:
            q = (pZ - A) / wt
            mk = 0 if q <= 0 else (m if q >= _F(m) else min(m, int(np.ceil(q))))
            if na == 0 and mk < 1:
                mk = 1
            if info is not None:
                with np.errstate(invalid="ignore"):
                    dist = np.append(dist, np.abs(A + np.arange(1 if na == 0 else 0, m, dtype=np.float32) * wt - pZ))
        margins["top_p"] = float(np.nanmin(dist) / pZ) if len(dist) else np.inf
    lo = 0
    stages = {"top_p": np.concatenate([order[:na_keep], ties[:mk]])}
    if armed:
        # ---- sample.h sample_warp: min_p -> typical_p -> epsilon -> eta, each on the set the one before it kept
        K = _Kept(x[order], keys[order], cw, na_keep, mk, tv, wt, M, per)
        with np.errstate(invalid="ignore", divide="ignore"):
            if min_p > 0:
                K.cut(_F(min_p), "min_p")                              # p_j < min_p p_max: the top's weight is exp(0) = 1
                stages["min_p"] = np.concatenate([order[K.lo:K.hi], ties[:K.mk]])
            if typical_p < 1.0:
                K.typical(_F(typical_p))
                stages["typical_p"] = np.concatenate([order[K.lo:K.hi], ties[:K.mk]])
            if epsilon_cutoff > 0:
                K.cut(_F(epsilon_cutoff) * K.z(), "epsilon_cutoff")
                stages["epsilon_cutoff"] = np.concatenate([order[K.lo:K.hi], ties[:K.mk]])
            if eta_cutoff > 0:
                Z3 = K.z()
                H3 = K.entropy(Z3)
                eta = min(_F(eta_cutoff), np.sqrt(_F(eta_cutoff)) * _sexp(np.array([-H3], np.float32))[0])
                K.cut(eta * Z3, "eta_cutoff")
                stages["eta_cutoff"] = np.concatenate([order[K.lo:K.hi], ties[:K.mk]])
        lo, na_keep, mk = K.lo, K.hi, K.mk
        margins.update(K.margins)
    base = cw[lo - 1] if lo else _F(0.0)
    Ak = (cw[na_keep - 1] if na_keep else _F(0.0)) - base
    target = u * (Ak + _F(mk) * wt)
    if info is not None:
        tcum = Ak + (np.arange(1, mk + 1, dtype=np.float32) * wt).astype(np.float32)
        info.update(kept=np.concatenate([order[lo:na_keep], ties[:mk]]), cum=np.concatenate([cw[lo:na_keep] - base, tcum]).astype(np.float32),
                    target=target, total=Ak + _F(mk) * wt, stages=stages, margins=margins, margin=min(margins.values(), default=np.inf))
    hit = np.nonzero(cw[lo:na_keep] - base > target)[0]
    if len(hit):
        return int(order[lo + hit[0]])
    if mk == 0:
        return int(order[na_keep - 1])
    r = (target - Ak) / wt
    jt = 0 if r <= 0 else (mk - 1 if r >= _F(mk - 1) else int(np.floor(r)))
    return int(ties[jt])


def _slog(s):
    """sample.h sample_log: log(s), s >= 1 finite, every operation rounded in float32"""
    s = np.asarray(s, np.float32)
    u = s.view(np.uint32)
    e = (u >> np.uint32(23)).astype(np.int32) - 127
    m = ((u & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32)
    big = m > _F(float.fromhex("0x1.6a09e6p+0"))
    m = np.where(big, m * _F(0.5), m).astype(np.float32)
    e = e + big.astype(np.int32)
    f = m - _F(1.0)
    t = f / (_F(2.0) + f)
    t2 = t * t
    p = np.full_like(t, _F(float.fromhex("0x1.c71c72p-4")))
    for c in ("0x1.24924ap-3", "0x1.99999ap-3", "0x1.555556p-2"):
        p = p * t2 + _F(float.fromhex(c))
    p = p * t2 + _F(1.0)
    lm = (t + t) * p
    fe = e.astype(np.float32)
    return (fe * _F(float.fromhex("0x1.62e4p-1")) + (fe * _F(float.fromhex("0x1.7f7d1cp-20")) + lm)).astype(np.float32)


def token_logprob_ref(row, i):
    """The device's log-probability of offset i of one head row (float32 [n], the raw masked logits of the head's range), bit for bit:
    (x[i] - M) - log(S), M = max x, S = sum exp(x - M) in sample.h's order (runs of C = ceil(n / 256) per thread in id order, then the scan
    over the 256 run totals).  An offset outside [0, n) gives -inf."""
    x = np.asarray(row, np.float32)
    n = len(x)
    M = x.max()
    with np.errstate(invalid="ignore"):
        _, S = _run_sums(_sexp(x - M), (n + _THREADS - 1) // _THREADS)
        if not 0 <= int(i) < n:
            return _F(-np.inf)
        return _F((x[int(i)] - M) - _slog(np.array([S], np.float32))[0])


# ---- scoring given tokens (csrc/score.hip) ----
SCORE_TILE = 128              # kernels.h SCORE_TILE = trace_op_score_tile()


def score_tile_partials(row, lo, hi):
    """(m, s) float32 per column tile of the head range [lo, hi) of one whole row of fp32 logits, as score_head_kernel's epilogue leaves them:
    tiles [j CT, (j + 1) CT) on ABSOLUTE columns clipped to the range, m_j = max x, s_j = h0 + h1 with h0 / h1 = the sums of exp(x - m_j) over the
    tile's lower / upper CT / 2 columns, each sequential in ascending column order from 0."""
    x = np.asarray(row, np.float32)
    ct = SCORE_TILE
    j0, j1 = lo // ct, (hi - 1) // ct
    buf = np.full((j1 - j0 + 1) * ct, -np.inf, np.float32)
    buf[lo - j0 * ct: hi - j0 * ct] = x[lo:hi]
    t = buf.reshape(-1, 2, ct // 2)
    m = t.max(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        w = _sexp(t - m[:, None, None])                                    # columns outside the range weigh exactly 0: adding them changes no bit
    h = np.cumsum(w, axis=2, dtype=np.float32)[:, :, -1]
    return m, (h[:, 0] + h[:, 1]).astype(np.float32)


def score_logprob_ref(row, lo, hi, t):
    """The device's log-probability (score.hip) of global id t under the head range [lo, hi) of one whole row of fp32 logits (float32 [NV]), bit
    for bit: M = max_j m_j, S = sum_j s_j * exp(m_j - M) sequentially in ascending j from 0 over score_tile_partials, (x[t] - M) - log S.
    t == -1 (ignore) gives 0.0, any other t outside [lo, hi) gives -inf."""
    t = int(t)
    if t == -1:
        return _F(0.0)
    if not lo <= t < hi:
        return _F(-np.inf)
    x = np.asarray(row, np.float32)
    m, s = score_tile_partials(x, lo, hi)
    M = m.max()
    with np.errstate(invalid="ignore"):
        terms = (s * _sexp(m - M)).astype(np.float32)
        S = np.cumsum(terms, dtype=np.float32)[-1]
        return _F((x[t] - M) - _slog(np.array([S], np.float32))[0])


# ---- logits processors (csrc/logits.h) ----
MAX_NGRAM = 64                # logits.h LOGITS_MAX_NGRAM


def check_logits_params(repetition_penalty, no_repeat_ngram_size, min_new_tokens) -> None:
    """HF's own argument checks (RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor / MinNewTokensLengthLogitsProcessor, with 0
    = off for the two integers as in GenerationConfig) and the device's bound on the n-gram size"""
    p = float(repetition_penalty)
    if not p > 0 or p != p or p == float("inf"):
        raise ValueError(f"`repetition_penalty` has to be a strictly positive finite float, but is {repetition_penalty}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0:
            raise ValueError(f"`{name}` has to be a non-negative integer, but is {v}")
    if no_repeat_ngram_size > MAX_NGRAM:
        raise ValueError(f"`no_repeat_ngram_size` is at most {MAX_NGRAM} on the device, but is {no_repeat_ngram_size}")


@dataclass(frozen=True)
class LogitsParams:
    """HF's logits processors in HF's order: repetition_penalty (1.0 = off), no_repeat_ngram_size (0 = off, at most 64), min_new_tokens
    (0 = off).  The history they look at is the ids a row has generated so far — never the prompt — as global vocabulary ids."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_new_tokens: int = 0

    def __post_init__(self):
        check_logits_params(self.repetition_penalty, self.no_repeat_ngram_size, self.min_new_tokens)

    @property
    def off(self) -> bool:
        return float(self.repetition_penalty) == 1.0 and self.no_repeat_ngram_size == 0 and self.min_new_tokens == 0


@dataclass(frozen=True)
class RowParams:
    """The generation parameters of ONE row of a decode batch (trace_row_params: TraceEngine.decode_begin / admit_rows_ex / decode / decode_queue
    row_params=, the sixth element of a generate_queue(per_request=True) request).  sampling: None or temperature <= 0 = this row is greedy; its seed
    is the row's own.  logits: None = no processors.  max_new_tokens: None = the batch's; else 1 .. the batch's — the row records, is fed forced ids
    and is log-scored up to its own bound, while the batch's stays the stride of every result row.  A None field of a queue request falls back to the
    call's own sampling= / logits= / max_new_tokens=."""
    sampling: Optional[SamplingParams] = None
    logits: Optional[LogitsParams] = None
    max_new_tokens: Optional[int] = None

    def check(self, max_new_tokens: Optional[int] = None) -> "RowParams":
        """ValueError unless the row can run on the device: HF's own checks of the sampling warpers (check_sampling), the device sampler's domain
        (SamplingParams.on_device) for a sampled row, the processors' domains (check_logits_params), and 1 <= max_new_tokens (<= the batch's, when
        given).  Returns self."""
        sp, lp, mn = self.sampling, self.logits, self.max_new_tokens
        if sp is not None:
            if not isinstance(sp, SamplingParams):
                raise ValueError(f"RowParams.sampling has to be a SamplingParams or None, but is {type(sp).__name__}")
            check_sampling(sp.temperature, sp.top_k, sp.top_p, sp.min_p, sp.typical_p, sp.epsilon_cutoff, sp.eta_cutoff)
            if not sp.greedy and not sp.on_device:
                raise ValueError("per-row sampling runs in the device decode loop: these sampling parameters lie outside the device sampler's domain "
                                 f"(top_k {sp.top_k}, top_p {sp.top_p})")
        if lp is not None:
            if not isinstance(lp, LogitsParams):
                raise ValueError(f"RowParams.logits has to be a LogitsParams or None, but is {type(lp).__name__}")
            check_logits_params(lp.repetition_penalty, lp.no_repeat_ngram_size, lp.min_new_tokens)
        if mn is not None:
            if not isinstance(mn, (int, np.integer)) or isinstance(mn, bool) or mn < 1:
                raise ValueError(f"`max_new_tokens` of a row has to be a positive integer, but is {mn}")
            if max_new_tokens is not None and mn > max_new_tokens:
                raise ValueError(f"`max_new_tokens` of a row is at most the batch's ({max_new_tokens}), but is {mn}")
        return self

    def over(self, sampling: Optional[SamplingParams], logits: Optional[LogitsParams], max_new_tokens: int) -> "RowParams":
        """self with every None field taken from the call's own values"""
        return RowParams(self.sampling if self.sampling is not None else sampling, self.logits if self.logits is not None else logits,
                         self.max_new_tokens if self.max_new_tokens is not None else int(max_new_tokens))

    @property
    def armed(self) -> bool:
        """the row's logits processors are on"""
        return self.logits is not None and not self.logits.off


def process_row_ref(row, hist, lo, hi, params: LogitsParams, step, eos):
    """The device's processed row (logits.h logits_process_row), bit for bit: row = one whole row of masked logits (float32 [NV]), hist = the ids
    the row has generated so far (global ids; ids outside [lo, hi) touch nothing), [lo, hi) the active head's range, step the device step, eos
    the decode batch's (< 0: none).  Returns a new float32 [NV]: the processed values on [lo, hi), -inf elsewhere.
      1. every DISTINCT id t of hist: y[t] = x[t] * p if x[t] < 0 else x[t] / p (float32, from the raw value);
      2. n-gram n, if len(hist) + 1 >= n: y[hist[i + n - 1]] = -inf for every i in [0, len(hist) - n] whose n - 1 ids equal the last n - 1;
      3. step < min_new_tokens and eos in the head: y[eos] = -inf."""
    x = np.asarray(row, np.float32)
    h = [int(t) for t in hist]
    out = np.full(len(x), -np.inf, np.float32)
    out[lo:hi] = x[lo:hi]
    p = _F(params.repetition_penalty)
    if p != _F(1.0):
        ids = np.array(sorted({t for t in h if lo <= t < hi}), np.int64)
        if len(ids):
            v = x[ids]
            with np.errstate(invalid="ignore"):
                out[ids] = np.where(v < 0, v * p, v / p).astype(np.float32)
    n, L = int(params.no_repeat_ngram_size), len(h)
    if n >= 1 and L + 1 >= n:
        suffix = h[L - (n - 1):] if n > 1 else []
        for i in range(0, L - n + 1):
            if h[i:i + n - 1] == suffix and lo <= h[i + n - 1] < hi:
                out[h[i + n - 1]] = -np.inf
    if int(step) < int(params.min_new_tokens) and lo <= int(eos) < hi:
        out[int(eos)] = -np.inf
    return out


# ---- constraints (csrc/constrain.h) ----
MAX_SEQS, MAX_SEQ_LEN, MAX_SUPPRESS = 64, 32, 1024          # constrain.h CONSTRAIN_MAX_SEQS / _SEQ_LEN / _SUPPRESS


def _is_id(t) -> bool:
    return isinstance(t, (int, np.integer)) and not isinstance(t, bool)


def check_constraints(stop_sequences, bad_words_ids, suppress_tokens, begin_suppress_tokens, n_vocab=None) -> None:
    """The device's bounds (at most 64 stop sequences and 64 bad words of 1..32 ids, at most 1024 ids per suppress list; nothing is truncated)
    and HF's own checks: no empty sequence, every id a non-negative integer - inside [0, n_vocab) where the vocabulary V+1+Tv+Sv is given."""
    def check_id(name, t):
        if not _is_id(t) or t < 0 or (n_vocab is not None and t >= n_vocab):
            raise ValueError(f"`{name}` holds {t!r}: every id has to be an integer in [0, {n_vocab if n_vocab is not None else 'vocabulary size'})")
    for name, seqs in (("stop_sequences", stop_sequences), ("bad_words_ids", bad_words_ids)):
        if len(seqs) > MAX_SEQS:
            raise ValueError(f"`{name}` holds {len(seqs)} sequences, at most {MAX_SEQS} on the device")
        for w in seqs:
            if len(w) == 0:
                raise ValueError(f"`{name}` holds an empty sequence")
            if len(w) > MAX_SEQ_LEN:
                raise ValueError(f"`{name}` holds a sequence of {len(w)} ids, at most {MAX_SEQ_LEN} on the device")
            for t in w:
                check_id(name, t)
    for name, ids in (("suppress_tokens", suppress_tokens), ("begin_suppress_tokens", begin_suppress_tokens)):
        if len(ids) > MAX_SUPPRESS:
            raise ValueError(f"`{name}` holds {len(ids)} ids, at most {MAX_SUPPRESS} on the device")
        for t in ids:
            check_id(name, t)


def _as_seqs(name, x):
    if x is None:
        return ()
    if isinstance(x, (str, bytes)) or any(isinstance(w, (str, bytes)) or _is_id(w) for w in x):
        raise ValueError(f"`{name}` has to be a list of lists of ids, but is {x!r}")
    return tuple(tuple(w.tolist() if hasattr(w, "tolist") else w) for w in x)


@dataclass(frozen=True)
class Constraints:
    """stop_sequences: id sequences that end a row like EOS once its generated ids end in one (the ids stay in the output); bad_words_ids: HF's
    NoBadWordsLogitsProcessor; suppress_tokens / begin_suppress_tokens: HF's SuppressTokens(AtBegin)LogitsProcessor, the latter at the first
    generated token only.  All ids are global vocabulary ids [text | <sync> | time | score]; the history the rules look at is the ids a row
    has generated so far, never the prompt.  Stored as tuples (hashable, comparable)."""
    stop_sequences: tuple = ()
    bad_words_ids: tuple = ()
    suppress_tokens: tuple = ()
    begin_suppress_tokens: tuple = ()

    def __post_init__(self):
        object.__setattr__(self, "stop_sequences", _as_seqs("stop_sequences", self.stop_sequences))
        object.__setattr__(self, "bad_words_ids", _as_seqs("bad_words_ids", self.bad_words_ids))
        for name in ("suppress_tokens", "begin_suppress_tokens"):
            v = getattr(self, name)
            object.__setattr__(self, name, () if v is None else tuple(v.tolist() if hasattr(v, "tolist") else v))
        check_constraints(self.stop_sequences, self.bad_words_ids, self.suppress_tokens, self.begin_suppress_tokens)

    @property
    def off(self) -> bool:
        return not (self.stop_sequences or self.bad_words_ids or self.suppress_tokens or self.begin_suppress_tokens)


def constrain_row_ref(row, hist, lo, hi, constraints: Constraints, step, min_new_tokens=0):
    """The ban rules of constrain.h on one whole row (float32 [NV]; the processed row where logits processors run first, process_row_ref's):
    a new float32 [NV], -inf outside [lo, hi).  hist: the ids the row has generated so far; step: the device step.
      4. bad word w: len 1: y[w[0]] = -inf; longer: if the last len(w) - 1 ids of hist equal w[:-1]: y[w[-1]] = -inf;
      5. suppress_tokens: y[t] = -inf at every step;   6. begin_suppress_tokens: at step 0 only;
      3. (widened) step < min_new_tokens: y[w[0]] = -inf for every stop sequence of one id.
    An id outside [lo, hi) touches nothing."""
    x = np.asarray(row, np.float32)
    h = [int(t) for t in hist]
    out = np.full(len(x), -np.inf, np.float32)
    out[lo:hi] = x[lo:hi]
    banned = []
    for w in constraints.bad_words_ids:
        k = len(w)
        if k == 1 or (len(h) >= k - 1 and h[len(h) - (k - 1):] == list(w[:-1])):
            banned.append(w[-1])
    banned += list(constraints.suppress_tokens)
    if int(step) == 0:
        banned += list(constraints.begin_suppress_tokens)
    if int(step) < int(min_new_tokens):
        banned += [w[0] for w in constraints.stop_sequences if len(w) == 1]
    for t in banned:
        if lo <= int(t) < hi:
            out[int(t)] = -np.inf
    return out


def stop_match_ref(hist, constraints: Constraints) -> bool:
    """the stop rule: some stop sequence w has len(hist) >= len(w) and equals the last len(w) ids of hist"""
    h = [int(t) for t in hist]
    return any(len(h) >= len(w) and h[len(h) - len(w):] == list(w) for w in constraints.stop_sequences)


def ends_stopped(ids, eos, constraints: Optional[Constraints] = None) -> bool:
    """'this row is finished': its recorded ids end in `eos` (>= 0) or in a stop sequence.  A row stops recording the moment either holds, so the
    tail of what it has recorded says it for good."""
    if len(ids) == 0:
        return False
    return (eos is not None and eos >= 0 and int(ids[-1]) == eos) or (constraints is not None and stop_match_ref(ids, constraints))


def head_bounds(head: int, V: int, Tv: int, Sv: int):
    return ((0, V + 1), (V + 1, V + 1 + Tv), (V + 1 + Tv, V + 1 + Tv + Sv))[int(head)]


def argmax_rows(logits, heads, V, Tv, Sv):
    """The greedy pick of a host-driven step: per row of masked logits [B, NV] (a torch tensor, taken where it lives, or numpy) the lowest id
    among equal maxima of the head's range - the device's rule (select_next_kernel); a range that is -inf throughout gives its first id.
    Only the B ids come back to the host."""
    import torch
    lg = logits.detach().float() if hasattr(logits, "detach") else torch.from_numpy(np.asarray(logits, np.float32))
    NV = lg.shape[1]
    lo, hi = (torch.tensor(x, device=lg.device).unsqueeze(1) for x in zip(*(head_bounds(h, V, Tv, Sv) for h in heads)))
    col = torch.arange(NV, device=lg.device).unsqueeze(0)
    inside = (col >= lo) & (col < hi)
    best = torch.where(inside, lg, torch.full_like(lg, -np.inf)).max(dim=1, keepdim=True).values
    return torch.where(inside & (lg == best), col, torch.full_like(col, NV)).min(dim=1).values.tolist()


def sample_rows_host(logits, heads, V, Tv, Sv, params: SamplingParams, steps):
    """The host path (parameters outside the device sampler's domain): one id per row of masked logits [B, NV] (numpy or a torch tensor)
    under the same rules and the same RNG contract as the device."""
    lg = logits.detach().float().cpu().numpy() if hasattr(logits, "detach") else np.asarray(logits, np.float32)
    out = []
    for b in range(lg.shape[0]):
        lo, hi = head_bounds(heads[b], V, Tv, Sv)
        u = philox_uniform(params.seed, int(steps[b]), b)
        out.append(lo + sample_row_ref(lg[b, lo:hi], params.temperature, params.top_k, params.top_p, u, None, *params.warpers))
    return out
