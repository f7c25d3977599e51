// logits_process_kernel: the logits processors (logits.h) as a launch between head_logits_kernel and select_next_kernel, and over loose rows
// (trace_op_logits_process: the unit tests and the host-driven decode loop) — the same device code.  The tile partials of head_logits_kernel
// describe the raw row, so a greedy step with processors takes its arg-max from the processed one: select_next_kernel<SELECT_ROW> (select.hip).
// The ban rules of constrain.h ride in the same kernel (a device-resident table, or none).
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "logits.h"

namespace {

// One workgroup per row, in two forms that share every line of the processing:
//   loose rows (dparams == null): history hist[b][0 .. hist_len[b]) at stride ld_hist, step steps[b], eos and the params by value; the whole
//     output row [0, V+1+Tv+Sv) is written, -inf outside the head.
//   decode step (dparams != null): launched before select_next_kernel of the same step, so *steps is this step's counter (the previous step's
//     selection finished earlier on the stream), and *steps - step0[b] the row's own step (min_new_tokens and begin-suppress count from it); the history is out_ids / out_len, its stride max_new = dparams[0], eos = dparams[1], the params
//     *dlp, or row_lp[b] where the batch carries per-row params (StepState::row_lp) — everything a captured graph must not freeze is read from device memory.  Only the head's range of the output row is written.
__global__ __launch_bounds__(LOGITS_THREADS) void logits_process_kernel(const float* __restrict__ logits, int ld, const int32_t* __restrict__ heads,
                                                                        int V, int Tv, int Sv, const int32_t* __restrict__ hist, int ld_hist,
                                                                        const int32_t* __restrict__ hist_len, const int32_t* __restrict__ steps,
                                                                        int eos, LogitsParams lpv, const int32_t* __restrict__ dparams,
                                                                        const LogitsParams* __restrict__ dlp, float* __restrict__ out, int ldo,
                                                                        int seen_words, const ConstrainTable* __restrict__ ct,
                                                                        const int32_t* __restrict__ step0,
                                                                        const LogitsParams* __restrict__ row_lp) {
    extern __shared__ __attribute__((aligned(16))) uint32_t seen[];
    __shared__ int32_t suffix[LOGITS_MAX_NGRAM];
    const int b = blockIdx.x, tid = threadIdx.x;
    int lo, hi;
    head_bounds(heads[b], V, Tv, Sv, lo, hi);
    if (((hi - lo + 31) >> 5) > seen_words) return;                     // (the launcher sizes the bitmap for the widest head: never taken)
    int step;
    LogitsParams lp;
    if (dparams) { ld_hist = dparams[0]; eos = dparams[1]; lp = row_lp ? row_lp[b] : *dlp; step = steps[0] - (step0 ? step0[b] : 0); }      // the row's own step (StepState::step0)
    else { lp = lpv; step = steps[b]; }
    const int L = max(0, min(hist_len[b], ld_hist));
    float* orow = out + (size_t)b * ldo;
    if (!dparams) {
        const int NV = V + 1 + Tv + Sv;
        for (int i = tid; i < lo; i += LOGITS_THREADS) orow[i] = -INFINITY;
        for (int i = hi + tid; i < NV; i += LOGITS_THREADS) orow[i] = -INFINITY;
    }
    logits_process_row(logits + (size_t)b * ld + lo, orow + lo, lo, hi - lo, hist + (size_t)b * ld_hist, L, lp, step, eos, seen, suffix, ct);
}

int seen_bytes(int V, int Tv, int Sv) { return (std::max(V + 1, std::max(Tv, Sv)) + 31) / 32 * 4; }

}  // namespace

int launch_logits_process(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* hist, int ld_hist,
                          const int32_t* hist_len, const int32_t* steps, int eos, const LogitsParams& lp, float* out, int ldo, hipStream_t s,
                          const ConstrainTable* ct) {
    const int NV = V + 1 + Tv + Sv;
    if (B < 1 || B > 65535 || ld < NV || ldo < NV || ld_hist < 0 || V < 1 || Tv < 1 || Sv < 1) return TRACE_ERR_ARG;
    const int lds = seen_bytes(V, Tv, Sv);
    if (lds > 32768) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(logits_process_kernel, dim3(B), dim3(LOGITS_THREADS), lds, s, logits, ld, heads, V, Tv, Sv, hist, ld_hist, hist_len, steps, eos, lp,
                       nullptr, nullptr, out, ldo, lds / 4, ct, nullptr, nullptr);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_step_logits_process(const float* logits, const StepState& st, int B, int V, int Tv, int Sv, const LogitsParams* dlp, float* out, hipStream_t s,
                               const ConstrainTable* ct) {
    if (B < 1 || B > SK_ROWS || !logits || !out || !dlp || !ct) return TRACE_ERR_ARG;
    const int NV = V + 1 + Tv + Sv, lds = seen_bytes(V, Tv, Sv);
    if (lds > 32768) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(logits_process_kernel, dim3(B), dim3(LOGITS_THREADS), lds, s, logits, NV, st.heads, V, Tv, Sv, st.out_ids, 0, st.out_len, st.step, -1,
                       LogitsParams{1.f, 0, 0}, st.params, dlp, out, NV, lds / 4, ct, st.step0, st.row_lp);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
