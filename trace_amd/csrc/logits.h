// Logits processors of the decode step: HF's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor
// (transformers 4.40.1, in HF's order) over one row of masked fp32 head logits, written to a row of its own: the raw row stays what the
// log-probabilities describe.  For row b with head range [lo, hi), history h = the ids the row has recorded so far (out_ids[b][0 .. out_len[b]): the
// generated ids only, the prompt is no part of it; global vocabulary ids, whichever head emitted them) and device step s:
//   1. penalty p != 1: for every DISTINCT id t of h inside [lo, hi): y[t] = x[t] < 0 ? x[t] * p : x[t] / p — one fp32 multiply or one true fp32
//      division of the RAW value, once per id however often it occurs (HF gathers from the unmodified row and scatters); -inf stays -inf, 0 stays 0;
//   2. no-repeat n-gram n in 1..64, if len(h) + 1 >= n: for every i in [0, len(h) - n] with h[i .. i + n - 2] == the last n - 1 ids of h:
//      y[h[i + n - 1]] = -inf (n = 1: every id of h);
//   3. min_new_tokens m: while s < m and eos lies in [lo, hi): y[eos] = -inf.
// Ids of h outside [lo, hi) touch nothing.  The three rules commute: 1 writes finite-or-unchanged values first, 2 and 3 only store -inf afterwards.
// Given a constraint table (constrain.h), its ban rules follow rule 2 behind the same barrier: 4 bad words, 5 suppress, 6 begin-suppress, and rule 3
// over every stop sequence of one id as well (HF bans every id of its EOS list).  They too only store -inf.
// One workgroup of 256 threads per row.  Rule 1 claims an id in a seen-bitmap in LDS (ceil((hi - lo) / 32) words of dynamic LDS) with a
// workgroup-scope atomic OR; only the thread that flips the bit writes, so no value is written twice and nothing on the row is read-modify-written.
// trace_amd/sampling.py process_row_ref restates it in float32 numpy bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "constrain.h"

struct LogitsParams {            // device-resident next to SampleParams (a captured graph reads them at replay)
    float penalty;               // > 0, 1 = off
    int32_t ngram;               // 0 = off, else 1..LOGITS_MAX_NGRAM
    int32_t min_new;             // 0 = off
};
constexpr int LOGITS_THREADS = 256;
constexpr int LOGITS_MAX_NGRAM = 64;

// src / dst: the head's range of the raw and of the processed row (dst != src), n = hi - lo; h: the row's history, L ids; seen: (n + 31) / 32
// words of LDS, suffix: LOGITS_MAX_NGRAM ints of LDS.  ct: the constraint table whose ban rules (constrain.h, rules 4 - 6 and rule 3 for every stop
// sequence of one id) follow rule 2 behind the same barrier, or null.  Every branch on lp / L / step / ct is uniform over the workgroup.
__device__ inline void logits_process_row(const float* __restrict__ src, float* __restrict__ dst, int lo, int n, const int32_t* __restrict__ h, int L,
                                          const LogitsParams lp, int step, int eos, uint32_t* seen, int32_t* suffix,
                                          const ConstrainTable* __restrict__ ct = nullptr) {
    const int tid = threadIdx.x;
    // ---- the copy: scalars up to the source's first 16-byte boundary, then float4 loads (and float4 stores where the destination is aligned alike)
    const int lead = min(n, (int)(((16u - (uint32_t)((uintptr_t)src & 15u)) & 15u) >> 2));
    const bool alike = ((((uintptr_t)src) ^ ((uintptr_t)dst)) & 15u) == 0;
    if (tid < lead) dst[tid] = src[tid];
    const int n4 = (n - lead) >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src + lead);
    if (alike) {
        float4* d4 = reinterpret_cast<float4*>(dst + lead);
        for (int i = tid; i < n4; i += LOGITS_THREADS) d4[i] = s4[i];
    } else {
        for (int i = tid; i < n4; i += LOGITS_THREADS) {
            const float4 x = s4[i];
            float* o = dst + lead + 4 * i;
            o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
        }
    }
    for (int i = lead + 4 * n4 + tid; i < n; i += LOGITS_THREADS) dst[i] = src[i];

    const bool pen = lp.penalty != 1.0f;
    const int ng = lp.ngram;
    const bool ngram_on = ng >= 1 && ng <= LOGITS_MAX_NGRAM && L + 1 >= ng;
    if (pen)
        for (int i = tid; i < (n + 31) >> 5; i += LOGITS_THREADS) seen[i] = 0u;
    if (ngram_on && tid < ng - 1) suffix[tid] = h[L - (ng - 1) + tid];
    __syncthreads();                    // the copy, the cleared bitmap and the suffix are in place

    if (pen) {
        const float p = lp.penalty;
        for (int i = tid; i < L; i += LOGITS_THREADS) {
            const int off = h[i] - lo;
            if (off < 0 || off >= n) continue;
            const uint32_t bit = 1u << (off & 31);
            const uint32_t old = __hip_atomic_fetch_or(&seen[off >> 5], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (old & bit) continue;                                   // another thread (or an earlier occurrence) owns this id
            const float x = src[off];
            dst[off] = x < 0.f ? x * p : x / p;
        }
    }
    __syncthreads();                    // every penalised value is stored before a ban may overwrite it

    if (ngram_on) {
        for (int i = tid; i + ng <= L; i += LOGITS_THREADS) {
            bool same = true;
            for (int j = 0; j < ng - 1 && same; ++j) same = h[i + j] == suffix[j];
            const int off = h[i + ng - 1] - lo;
            if (same && off >= 0 && off < n) dst[off] = -INFINITY;     // (several threads may ban one id: the same store)
        }
    }
    if (tid == 0 && step < lp.min_new && eos >= lo && eos - lo < n) dst[eos - lo] = -INFINITY;
    if (ct) constrain_ban_row(dst, lo, n, h, L, ct, step, lp.min_new);
}
