// The device sampler: one token from one row of masked fp32 head logits, HF's sampling warpers in HF's order
// (transformers 4.40.1 TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial):
//   1. x = logit / T (a true fp32 division: the same bits as torch's scores / T)
//   2. top_k (1..1024): keep x >= the k-th largest value (ties at the threshold kept); k >= the row width keeps everything
//   3. top_p (0 < p <= 1): order the survivors by (value desc, id asc); keep a token iff the mass ranked strictly above it is < p (the top
//      token always stays) — HF's "ascending cumsum <= 1 - p is removed" read from the other end
//   3b. min_p, typical_p, epsilon_cutoff, eta_cutoff (each optional, HF's order, top_k in [1, 1024] only): see sample_warp below
//   4. draw u in [0, 1) (philox.h, counter = (step, 0, row, 0)); walk the kept tokens in that order accumulating exp(x - max); take the first
//      whose running sum exceeds u * total, or the last kept token if rounding leaves none.
// top_k = 0 (off) is taken only with top_p = 1 and 3b off: the walk is then over the whole row in id order.
// One workgroup of 256 threads per row.  Top-k threshold: exact radix select (4 passes of 8 bits, per-wave LDS histograms) on the order-
// preserving uint32 key of x — no sort of the row.  The strictly-above set (< k <= 1024 entries) is bitonic-sorted in LDS; the tie class at the
// threshold (any size) is a block of equally probable ids in id order: the top-p cut and the draw inside it are rank arithmetic plus one
// counting pass.  Every sum has a fixed order (sequential runs per thread, then a Hillis-Steele scan over the 256 run totals) and no product
// is contracted into an FMA (contract(off) in every function below), so the result is a pure function of (row, T, k, p, seed, step, row index) — and a float32 numpy restatement of the
// same operations (trace_amd/sampling.py) reproduces it bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "philox.h"

struct SampleParams {            // device-resident next to the decode step's params (a captured graph reads them at replay)
    float temperature;           // > 0
    int32_t top_k;               // 0 = off (only with top_p == 1), else 1..1024
    float top_p;                 // (0, 1]
    uint32_t seed_lo, seed_hi;
    float min_p;                 // [0, 1], 0 = off          the four below need top_k in [1, 1024]
    float typical_p;             // (0, 1), >= 1 = off
    float epsilon;               // (0, 1), 0 = off
    float eta, sqrt_eta;         // (0, 1), 0 = off; sqrt_eta = sqrtf(eta), formed on the host (IEEE sqrt: one value everywhere)
};
constexpr int SAMPLE_MAX_K = 1024;
constexpr int SAMPLE_THREADS = 256;

struct SampleLds {
    union {                                  // (the same 4 KB: the histograms are done with before typical_p starts)
        uint32_t hist[4][256];
        float sk[SAMPLE_MAX_K];              // typical_p: (-log p_j) - H of the sorted candidates (non-decreasing in j)
    };
    unsigned long long cand[SAMPLE_MAX_K];   // (~key << 32 | id): ascending order = (value desc, id asc)
    float cw[SAMPLE_MAX_K];                  // running sums of the sorted candidates' weights
    float fbuf[SAMPLE_THREADS];
    uint32_t ubuf[SAMPLE_THREADS];
    float wmax[4];
    uint32_t n_above, n_tie, sel, krem, amin;
    int result;
};

__device__ __forceinline__ uint32_t sample_key(float f) {          // order-preserving: larger value -> larger key
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// exp(x) for x <= 0: Cody-Waite reduction + degree-6 Taylor polynomial, every operation rounded on its own (no FMA contraction), so
// a float32 restatement gives the same bits.  Relative error ~2e-7; below -80 (2^-115) the weight is 0, far below the top token's 1.
__device__ __forceinline__ float sample_exp(float x) {
#pragma clang fp contract(off)
    if (!(x > -80.f)) return 0.f;
    const float n = rintf(x * 0x1.715476p+0f);                    // log2(e); constants in hex: exact float32 values on both sides
    float r = x - n * 0x1.62e4p-1f;                               // ln 2, high part
    r = r - n * 0x1.7f7d1cp-20f;                                  //       low part
    float p = 0x1.6c16c2p-10f;                                    // 1/720, 1/120, 1/24, 1/6
    p = p * r + 0x1.111112p-7f;
    p = p * r + 0x1.555556p-5f;
    p = p * r + 0x1.555556p-3f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return p * __uint_as_float((uint32_t)((int)n + 127) << 23);
}

// inclusive Hillis-Steele scan over the 256 threads' values (fixed order); buf[t] holds the inclusive value of thread t afterwards
template <class V>
__device__ __forceinline__ V sample_scan(V v, V* buf) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < SAMPLE_THREADS; d <<= 1) {
        const V o = t >= d ? buf[t - d] : V(0);
        __syncthreads();
        if (t >= d) { v = o + v; buf[t] = v; }
        __syncthreads();
    }
    return v;
}

// log(s) for a normal s > 0 (the sums here are >= 1; the mass typical_p keeps can be less): s = m 2^e with m in (sqrt(1/2), sqrt(2)],
// log m = 2 atanh(t), t = (m - 1) / (m + 1), as the odd series up to t^9
// (|t| <= 0.1716: the first dropped term is below 2e-9 of the result); e ln 2 from the same two-part ln 2 as sample_exp.  Every operation is
// rounded on its own (a true fp32 division, no FMA contraction), constants in hex: a float32 restatement gives the same bits.
__device__ __forceinline__ float sample_log(float s) {
#pragma clang fp contract(off)
    const uint32_t u = __float_as_uint(s);
    int e = (int)(u >> 23) - 127;
    float m = __uint_as_float((u & 0x007fffffu) | 0x3f800000u);   // [1, 2)
    if (m > 0x1.6a09e6p+0f) { m = m * 0.5f; e += 1; }             // (sqrt 2 / 2, sqrt 2]
    const float f = m - 1.0f;                                     // exact
    const float t = f / (2.0f + f);
    const float t2 = t * t;
    float p = 0x1.c71c72p-4f;                                     // 1/9, 1/7, 1/5, 1/3
    p = p * t2 + 0x1.24924ap-3f;
    p = p * t2 + 0x1.99999ap-3f;
    p = p * t2 + 0x1.555556p-2f;
    p = p * t2 + 1.0f;
    const float lm = (t + t) * p;
    const float fe = (float)e;
    return fe * 0x1.62e4p-1f + (fe * 0x1.7f7d1cp-20f + lm);
}

// ---- the log-probability of one token of a row of masked head logits (trace_decode_set_logprobs / trace_op_token_logprob) ----
// row = the active head's RAW fp32 logits [0, n) as head_logits_kernel writes them (no temperature, no top-k / top-p: the model's own
// distribution), off = the token's offset in the row:
//     logprob = (x[off] - M) - log(S),   M = max x,   S = sum_i exp(x_i - M)
// S is formed as the sampler forms its sums: weights from sample_exp, thread t of 256 sums its id-order run [t C, (t + 1) C) sequentially,
// sample_scan runs over the 256 run totals, nothing is contracted into an FMA; log = sample_log (S >= 1: the maximum contributes exp(0)).
// An offset outside [0, n) gives -inf.  trace_amd/sampling.py token_logprob_ref restates it in float32 numpy bit for bit.
// One workgroup of SAMPLE_THREADS threads; every thread returns the value.  fbuf: SAMPLE_THREADS floats, wmax: 4 floats (LDS).
__device__ inline float token_logprob_row(const float* __restrict__ row, int n, int off, float* fbuf, float* wmax) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, wid = tid >> 6;
    float m = -INFINITY;
    for (int i = tid; i < n; i += 4 * SAMPLE_THREADS) {              // four loads in flight per thread (one row per workgroup: latency-bound)
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = i + q * SAMPLE_THREADS < n ? row[i + q * SAMPLE_THREADS] : -INFINITY;
        m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = wave_max(m);
    if ((tid & 63) == 0) wmax[wid] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const int C = (n + SAMPLE_THREADS - 1) / SAMPLE_THREADS;
    const int i0 = min(n, tid * C), i1 = min(n, i0 + C);
    float s = 0.f;
    int i = i0;
    for (; i + 4 <= i1; i += 4) {                                    // the run in id order; the four loads are issued together, the adds stay sequential
        const float a = row[i], b = row[i + 1], c = row[i + 2], d = row[i + 3];
        s = s + sample_exp(a - M);
        s = s + sample_exp(b - M);
        s = s + sample_exp(c - M);
        s = s + sample_exp(d - M);
    }
    for (; i < i1; ++i) s = s + sample_exp(row[i] - M);
    sample_scan(s, fbuf);
    const float S = fbuf[SAMPLE_THREADS - 1];
    if (off < 0 || off >= n) return -INFINITY;
    return (row[off] - M) - sample_log(S);
}

__device__ __forceinline__ void sample_min_result(SampleLds& L, int v) {
    __hip_atomic_fetch_min(&L.result, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ---- the warpers behind top_p: min_p, typical_p, epsilon_cutoff, eta_cutoff (HF's MinP / Typical / Epsilon / Eta LogitsWarper, in that order) ----
// What top_p leaves is the sorted candidates [lo, hi) (lo = 0) followed by mk tokens of the tie block (one value tv, weight wt each).  Every warper
// maps such a set to such a set: min_p, epsilon and eta cut the candidates' tail, typical_p keeps an interval of them (-log p is monotone along the
// order); the tie block has one value, hence one key under every rule: it stays or goes whole, and it stays only while the candidates reach hi.
// Each warper sees the distribution renormalised over what the earlier ones kept: Z = (cw[hi - 1] - cw[lo - 1]) + mk wt.
__device__ __forceinline__ float sample_cand_x(const SampleLds& L, int j) { return sample_unkey(~(uint32_t)(L.cand[j] >> 32)); }

__device__ __forceinline__ float sample_kept_z(const SampleLds& L, int lo, int hi, float mkwt) {
#pragma clang fp contract(off)
    return ((hi ? L.cw[hi - 1] : 0.f) - (lo ? L.cw[lo - 1] : 0.f)) + mkwt;
}

// Tail cut: the first j in [lo, hi) with w_j < thr whose value is below the top's (tokens equal to the maximum always stay), else hi; the tie block
// follows if no candidate went and it is the top itself or its weight is not below thr.  L.result is 0x7fffffff on entry and on exit.
__device__ __forceinline__ void sample_cut(SampleLds& L, int lo, int& hi, int& mk, float thr, float wt, float M) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const uint32_t top = lo < hi ? (uint32_t)(L.cand[lo] >> 32) : 0u;
    for (int j = lo + tid; j < hi; j += SAMPLE_THREADS) {
        const uint32_t kj = (uint32_t)(L.cand[j] >> 32);
        if (kj != top && sample_exp(sample_unkey(~kj) - M) < thr) sample_min_result(L, j);
    }
    __syncthreads();
    const int r = min(L.result, hi);
    __syncthreads();
    if (tid == 0) L.result = 0x7fffffff;
    if (r < hi || (lo < hi && wt < thr)) mk = 0;
    hi = r;
    __syncthreads();
}

// H = log Z - (sum_j w_j (x_j - M)) / Z over the kept set: thread t sums its candidates 4t .. 4t + 3 in order (0 outside [lo, hi)), sample_scan over
// the thread totals, then the tie block's mk (wt (tv - M)); a weight of exactly 0 contributes 0.
__device__ __forceinline__ float sample_entropy(SampleLds& L, int lo, int hi, int mk, float wt, float tv, float M, float Z) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * tid + q;
        float e = 0.f;
        if (j >= lo && j < hi) {
            const float d = sample_cand_x(L, j) - M, w = sample_exp(d);
            if (w > 0.f) e = w * d;
        }
        s = s + e;
    }
    sample_scan(s, L.fbuf);
    float D = L.fbuf[SAMPLE_THREADS - 1];
    __syncthreads();
    const float te = wt > 0.f ? wt * (tv - M) : 0.f;
    D = D + (float)mk * te;
    return sample_log(Z) - D / Z;
}

// #{i in [0, n): sk[i] < x} and #{i: sk[i] <= x} of the non-decreasing sk
__device__ __forceinline__ int sample_count_lt(const float* sk, int n, float x) {
    int a = 0, b = n;
    while (a < b) { const int c = (a + b) >> 1; if (sk[c] < x) a = c + 1; else b = c; }
    return a;
}
__device__ __forceinline__ int sample_count_le(const float* sk, int n, float x) {
    int a = 0, b = n;
    while (a < b) { const int c = (a + b) >> 1; if (sk[c] <= x) a = c + 1; else b = c; }
    return a;
}

// typical_p on candidates [0, hi) + mk ties: s_j = (log Z - (x_j - M)) - H is non-decreasing in j, a_j = |s_j| HF's sort key.  HF keeps a <= a*,
// a* = the smallest key v whose class {a <= v} holds mass >= typical_p — the interval {-v <= s <= v} of the order, its mass a difference of two
// running sums.  Every candidate (and the tie block) tries its own key; the smallest that qualifies wins (non-negative floats order as their bits).
__device__ __forceinline__ void sample_typical(SampleLds& L, int& lo, int& hi, int& mk, float tp, float wt, float tv, float M) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const float mkwt = (float)mk * wt;
    const float Z = sample_kept_z(L, 0, hi, mkwt);
    const float H = sample_entropy(L, 0, hi, mk, wt, tv, M, Z);
    const float lZ = sample_log(Z);
    for (int j = tid; j < hi; j += SAMPLE_THREADS) L.sk[j] = (lZ - (sample_cand_x(L, j) - M)) - H;
    if (tid == 0) L.amin = 0x7f800000u;
    __syncthreads();
    const float st = (lZ - (tv - M)) - H, tpZ = tp * Z;
    for (int j = tid; j < hi + (mk > 0 ? 1 : 0); j += SAMPLE_THREADS) {
        const float v = fabsf(j < hi ? L.sk[j] : st);
        const int l = sample_count_lt(L.sk, hi, -v), r = sample_count_le(L.sk, hi, v);
        float mass = (r ? L.cw[r - 1] : 0.f) - (l ? L.cw[l - 1] : 0.f);
        if (mk > 0 && st <= v) mass = mass + mkwt;
        if (mass >= tpZ) __hip_atomic_fetch_min(&L.amin, __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    const float a = __uint_as_float(L.amin);
    const int l = sample_count_lt(L.sk, hi, -a), r = sample_count_le(L.sk, hi, a);
    const int mt = mk > 0 && st <= a ? mk : 0;
    if (l < r || mt > 0) { lo = l; hi = r; mk = mt; }                 // (an empty result can come only from NaNs: keep everything then)
    __syncthreads();
}

// min_p -> typical_p -> epsilon -> eta over the set top_p left: candidates [0, hi) + mk ties in, candidates [lo, hi) + mk ties out
__device__ __forceinline__ void sample_warp(SampleLds& L, const SampleParams& sp, int& lo, int& hi, int& mk, float wt, float tv, float M) {
#pragma clang fp contract(off)
    if (sp.min_p > 0.f) sample_cut(L, 0, hi, mk, sp.min_p, wt, M);      // p_j < min_p p_max: the top's weight is exp(0) = 1
    if (sp.typical_p < 1.f) sample_typical(L, lo, hi, mk, sp.typical_p, wt, tv, M);
    if (sp.epsilon > 0.f) sample_cut(L, lo, hi, mk, sp.epsilon * sample_kept_z(L, lo, hi, (float)mk * wt), wt, M);
    if (sp.eta > 0.f) {
        const float Z = sample_kept_z(L, lo, hi, (float)mk * wt);
        const float H = sample_entropy(L, lo, hi, mk, wt, tv, M, Z);
        const float eta = fminf(sp.eta, sp.sqrt_eta * sample_exp(-H));
        sample_cut(L, lo, hi, mk, eta * Z, wt, M);
    }
}

// row = the active head's logits [0, n); returns the chosen offset in [0, n) (every thread).  step / rowid feed the Philox counter.
__device__ inline int sample_row(const float* __restrict__ row, int n, const SampleParams sp, uint32_t step, uint32_t rowid, SampleLds& L) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, wid = tid >> 6;
    const float T = sp.temperature;
    const float u = philox_uniform(((uint64_t)sp.seed_hi << 32) | sp.seed_lo, step, rowid);
    const int C = (n + SAMPLE_THREADS - 1) / SAMPLE_THREADS;         // id-order runs: thread t owns [t C, min(n, (t + 1) C))
    const int i0 = min(n, tid * C), i1 = min(n, i0 + C);
    if (tid == 0) { L.result = 0x7fffffff; L.n_above = 0; L.n_tie = 0; }

    if (sp.top_k <= 0) {
        // ---- whole row, id order: max, run sums, scan, first running sum above u * Z
        float m = -INFINITY;
        for (int i = tid; i < n; i += SAMPLE_THREADS) m = fmaxf(m, row[i] / T);
        m = wave_max(m);
        if ((tid & 63) == 0) L.wmax[wid] = m;
        __syncthreads();
        const float M = fmaxf(fmaxf(L.wmax[0], L.wmax[1]), fmaxf(L.wmax[2], L.wmax[3]));
        float s = 0.f;
        for (int i = i0; i < i1; ++i) s = s + sample_exp(row[i] / T - M);
        sample_scan(s, L.fbuf);
        const float Z = L.fbuf[SAMPLE_THREADS - 1];
        const float excl = tid ? L.fbuf[tid - 1] : 0.f;
        const float target = u * Z;
        float acc = 0.f;
        for (int i = i0; i < i1; ++i) {
            acc = acc + sample_exp(row[i] / T - M);
            if (excl + acc > target) { sample_min_result(L, i); break; }
        }
        __syncthreads();
        const int r = L.result;
        return r == 0x7fffffff ? n - 1 : r;
    }

    // ---- top-k threshold: the k-th largest key, 8 bits at a time
    const int k = min(sp.top_k, n);
    uint32_t prefix = 0, mask = 0, krem = (uint32_t)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int w = 0; w < 4; ++w) L.hist[w][tid] = 0u;
        __syncthreads();
        for (int i = tid; i < n; i += 4 * SAMPLE_THREADS) {          // four loads in flight per thread (one pass is latency-bound at batch 1)
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = i + q * SAMPLE_THREADS < n ? row[i + q * SAMPLE_THREADS] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t key = sample_key(v[q] / T);
                if (i + q * SAMPLE_THREADS < n && (key & mask) == prefix)
                    __hip_atomic_fetch_add(&L.hist[wid][(key >> shift) & 255u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        const int bin = 255 - tid;                   // thread t scans bins from the top: inclusive = #keys in bins >= bin
        const uint32_t h = L.hist[0][bin] + L.hist[1][bin] + L.hist[2][bin] + L.hist[3][bin];
        const uint32_t incl = sample_scan(h, L.ubuf);
        if (incl >= krem && incl - h < krem) { L.sel = (uint32_t)bin; L.krem = krem - (incl - h); }
        __syncthreads();
        prefix |= L.sel << shift;
        mask |= 255u << shift;
        krem = L.krem;
        __syncthreads();
    }
    const uint32_t theta = prefix;

    // ---- the strictly-above set (< k entries) and the tie class
    for (int i0q = tid; i0q < n; i0q += 4 * SAMPLE_THREADS) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = i0q + q * SAMPLE_THREADS < n ? row[i0q + q * SAMPLE_THREADS] : -INFINITY;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0q + q * SAMPLE_THREADS;
            const uint32_t key = sample_key(v[q] / T);
            if (i >= n) continue;
            if (key > theta) {
                const uint32_t slot = __hip_atomic_fetch_add(&L.n_above, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                L.cand[slot] = ((unsigned long long)(~key) << 32) | (uint32_t)i;
            } else if (key == theta) {
                __hip_atomic_fetch_add(&L.n_tie, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();
    const int na = (int)L.n_above, m = (int)L.n_tie;
    int P = 1;
    while (P < na) P <<= 1;
    for (int j = na + tid; j < P; j += SAMPLE_THREADS) L.cand[j] = ~0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)                       // bitonic sort, ascending
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += SAMPLE_THREADS) {
                const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                const unsigned long long a = L.cand[lo], b = L.cand[hi];
                if (((lo & size) == 0) == (a > b)) { L.cand[lo] = b; L.cand[hi] = a; }
            }
            __syncthreads();
        }
    const float tv = sample_unkey(theta);
    const float M = na ? sample_unkey(~(uint32_t)(L.cand[0] >> 32)) : tv;
    // running sums of the sorted candidates: thread t sums j = 4t .. 4t + 3 in order, then the scan over the thread totals
    float l[4], s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * tid + q;
        const float w = j < na ? sample_exp(sample_unkey(~(uint32_t)(L.cand[j] >> 32)) - M) : 0.f;
        s = s + w;
        l[q] = s;
    }
    sample_scan(s, L.fbuf);
    const float excl = tid ? L.fbuf[tid - 1] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) if (4 * tid + q < na) L.cw[4 * tid + q] = excl + l[q];
    __syncthreads();
    const float A = na ? L.cw[na - 1] : 0.f;
    const float wt = sample_exp(tv - M);
    const float Z = A + (float)m * wt;

    // ---- top-p: na_keep = the first candidate whose mass above is >= p Z; ties follow only if every candidate stays
    int na_keep = na, mk = m;
    if (sp.top_p < 1.f) {
        const float pZ = sp.top_p * Z;
        for (int j = tid; j < na; j += SAMPLE_THREADS)
            if ((j ? L.cw[j - 1] : 0.f) >= pZ) sample_min_result(L, j);
        __syncthreads();
        na_keep = min(L.result, na);                                  // (j = 0 never qualifies: the top token always stays)
        __syncthreads();
        if (tid == 0) L.result = 0x7fffffff;
        if (na_keep < na) mk = 0;
        else {
            const float q = (pZ - A) / wt;                            // tie j stays iff A + j wt < p Z
            mk = q <= 0.f ? 0 : (q >= (float)m ? m : min(m, (int)ceilf(q)));
            if (na == 0 && mk < 1) mk = 1;
        }
        __syncthreads();
    }
    // ---- min_p, typical_p, epsilon, eta: the kept candidates become [lo, na_keep); with all four off nothing below this line changes a bit
    int lo = 0;
    if (sp.min_p > 0.f || sp.typical_p < 1.f || sp.epsilon > 0.f || sp.eta > 0.f) sample_warp(L, sp, lo, na_keep, mk, wt, tv, M);
    const float base = lo ? L.cw[lo - 1] : 0.f;
    const float Ak = (na_keep ? L.cw[na_keep - 1] : 0.f) - base;
    const float target = u * (Ak + (float)mk * wt);

    // ---- draw: first kept candidate whose running sum exceeds the target, else inside the tie block
    for (int j = lo + tid; j < na_keep; j += SAMPLE_THREADS)
        if (L.cw[j] - base > target) sample_min_result(L, j);
    __syncthreads();
    const int jc = L.result;
    if (jc != 0x7fffffff) return (int)(uint32_t)L.cand[jc];
    if (mk == 0) return (int)(uint32_t)L.cand[na_keep - 1];
    const float r = (target - Ak) / wt;
    const int jt = r <= 0.f ? 0 : (r >= (float)(mk - 1) ? mk - 1 : (int)floorf(r));
    // counting pass: the jt-th tie in id order
    uint32_t cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += sample_key(row[i] / T) == theta;
    const uint32_t incl = sample_scan(cnt, L.ubuf);
    const uint32_t ex = incl - cnt;
    if ((uint32_t)jt >= ex && (uint32_t)jt < incl) {
        uint32_t c = ex;
        for (int i = i0; i < i1; ++i)
            if (sample_key(row[i] / T) == theta) { if (c == (uint32_t)jt) { L.result = i; break; } ++c; }
    }
    __syncthreads();
    return L.result;
}
