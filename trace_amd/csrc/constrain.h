// Constraints of the decode step over the ids a row has generated: HF's NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor and
// SuppressTokensAtBeginLogitsProcessor (transformers 4.40.1) as ban rules 4 - 6 behind rules 1 - 3 of logits.h, every EOS id of a list under
// min_new_tokens (rule 3, widened), and stop sequences in the selection.  For row b with head range [lo, hi), history h = out_ids[b][0 .. out_len[b])
// (generated ids only, global vocabulary ids, whichever head emitted them) and device step s:
//   4. bad word w of k ids: k == 1: y[w[0]] = -inf; k > 1: if len(h) >= k - 1 and the last k - 1 ids of h equal w[0 .. k - 1): y[w[k - 1]] = -inf;
//   5. suppress: y[t] = -inf for every listed t, at every step;
//   6. begin_suppress: the same at s == 0 only;
//   3. (widened) while s < min_new_tokens: y[w[0]] = -inf for every stop sequence of one id, as for eos.
// An id to ban outside [lo, hi) touches nothing.  Only -inf is stored, after the penalised values of rule 1 are in place (logits.h's second barrier).
// Stop rule (select_next_kernel, after the step's token is recorded for a row that was not done): stop sequence w of k ids fires iff out_len[b] >= k
// and the last k recorded ids equal w; the row is then done as an EOS row is: the ids stay, out_len counts them, nothing is recorded afterwards.
// The table lives in device memory and is read at replay: a captured step stays valid when it changes between batches.
// trace_amd/sampling.py constrain_row_ref / stop_match_ref restate both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int CONSTRAIN_MAX_SEQS = 64;          // stop sequences; bad-word sequences
constexpr int CONSTRAIN_MAX_SEQ_LEN = 32;       // ids per sequence
constexpr int CONSTRAIN_MAX_SUPPRESS = 1024;    // ids per suppress list
constexpr int CONSTRAIN_THREADS = 256;          // = LOGITS_THREADS = select_next_kernel's workgroup

struct ConstrainTable {          // device-resident; the host copy is built (and bounded) by trace_decode_set_constraints / the loose-row ops
    int32_t n_stop, n_bad, n_suppress, n_begin;                       // the header
    int32_t stop_off[CONSTRAIN_MAX_SEQS + 1], bad_off[CONSTRAIN_MAX_SEQS + 1];   // CSR: sequence i = ids[off[i] .. off[i + 1])
    int32_t stop_ids[CONSTRAIN_MAX_SEQS * CONSTRAIN_MAX_SEQ_LEN], bad_ids[CONSTRAIN_MAX_SEQS * CONSTRAIN_MAX_SEQ_LEN];
    int32_t suppress[CONSTRAIN_MAX_SUPPRESS], begin[CONSTRAIN_MAX_SUPPRESS];
};

// does sequence i of a CSR list (ids[off[i] .. off[i + 1]), at most CONSTRAIN_MAX_SEQ_LEN ids) minus its last `drop` ids equal the tail of h[0 .. L)?
__device__ inline bool constrain_tail_equals(const int32_t* h, int L, const int32_t* off, const int32_t* ids, int i, int drop, int& last) {
    const int o = off[i], k = off[i + 1] - o;
    if (k < 1 || k > CONSTRAIN_MAX_SEQ_LEN || o < 0 || o + k > CONSTRAIN_MAX_SEQS * CONSTRAIN_MAX_SEQ_LEN) return false;   // (the host never builds such a table)
    last = ids[o + k - 1];
    const int m = k - drop;
    if (L < m) return false;
    bool same = true;
    for (int j = 0; j < m && same; ++j) same = h[L - m + j] == ids[o + j];
    return same;
}

// Rules 4 - 6 and the widened rule 3 on dst, the head's range [lo, lo + n) of the processed row; every thread of the 256 calls it, after the barrier
// behind rule 1.  Threads 0 .. 63 take one bad word each, threads 64 .. 127 one stop sequence each (rule 3), and all 256 stride over the two flat lists.
__device__ inline void constrain_ban_row(float* __restrict__ dst, int lo, int n, const int32_t* __restrict__ h, int L, const ConstrainTable* __restrict__ t,
                                         int step, int min_new) {
    const int tid = threadIdx.x;
    const int nb = min(t->n_bad, CONSTRAIN_MAX_SEQS), ns = step < min_new ? min(t->n_stop, CONSTRAIN_MAX_SEQS) : 0;
    int last = -1;
    bool ban = false;
    if (tid < nb) ban = constrain_tail_equals(h, L, t->bad_off, t->bad_ids, tid, 1, last);
    else if (tid >= CONSTRAIN_MAX_SEQS && tid - CONSTRAIN_MAX_SEQS < ns)
        ban = t->stop_off[tid - CONSTRAIN_MAX_SEQS + 1] - t->stop_off[tid - CONSTRAIN_MAX_SEQS] == 1 &&
              constrain_tail_equals(h, L, t->stop_off, t->stop_ids, tid - CONSTRAIN_MAX_SEQS, 1, last);
    if (ban && last >= lo && last - lo < n) dst[last - lo] = -INFINITY;
    const int nsup = min(t->n_suppress, CONSTRAIN_MAX_SUPPRESS), nbeg = step == 0 ? min(t->n_begin, CONSTRAIN_MAX_SUPPRESS) : 0;
    for (int i = tid; i < nsup; i += CONSTRAIN_THREADS) {
        const int off = t->suppress[i] - lo;
        if (off >= 0 && off < n) dst[off] = -INFINITY;
    }
    for (int i = tid; i < nbeg; i += CONSTRAIN_THREADS) {
        const int off = t->begin[i] - lo;
        if (off >= 0 && off < n) dst[off] = -INFINITY;
    }
}

// The stop rule over one row's history h[0 .. L): true in every thread of the workgroup iff some stop sequence equals the tail of h.  Thread i
// compares sequence i (at most 32 ids); the workgroup's OR decides.  Every thread of the 256 must call it (it holds a barrier).
__device__ inline bool stop_match_row(const int32_t* h, int L, const ConstrainTable* __restrict__ t) {
    const int tid = threadIdx.x;
    int last;
    const bool hit = tid < min(t->n_stop, CONSTRAIN_MAX_SEQS) && constrain_tail_equals(h, L, t->stop_off, t->stop_ids, tid, 0, last);
    return __syncthreads_or(hit ? 1 : 0) != 0;
}
