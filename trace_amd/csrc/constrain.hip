// The stop rule of constrain.h on the device: the forms of select_next_kernel that match stop sequences against the ids a row has recorded (select.h,
// STOP), and stop_match_kernel, the same matcher over loose histories (trace_op_stop_match: the unit tests).  The ban rules of constrain.h live in
// logits_process_kernel (logits.hip).
#include "select.h"

namespace {

// fired[b] = 1 iff a stop sequence of *ct equals the tail of hist[b][0 .. hist_len[b]); one workgroup per row
__global__ __launch_bounds__(CONSTRAIN_THREADS) void stop_match_kernel(const int32_t* __restrict__ hist, int ld_hist, const int32_t* __restrict__ hist_len,
                                                                       const ConstrainTable* __restrict__ ct, int32_t* __restrict__ fired) {
    const int b = blockIdx.x;
    const int L = max(0, min(hist_len[b], ld_hist));
    const bool hit = stop_match_row(hist + (size_t)b * ld_hist, L, ct);
    if (threadIdx.x == 0) fired[b] = hit ? 1 : 0;
}

}  // namespace

int launch_select_stop(int form, const float* part_val, const int32_t* part_idx, const float* logits, const SampleParams* sp, const StepState& st,
                       const bf16_t* embed, const bf16_t* time_tab, const bf16_t* score_tab, const bf16_t* sync_row, bf16_t* xnext, int ldx, int B, int H,
                       int V, int Tv, int Sv, int advance, hipStream_t s, const ConstrainTable* ct) {
    if (!ct) return TRACE_ERR_ARG;
    return launch_select_forms<true>(form, part_val, part_idx, logits, sp, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H, V, Tv, Sv, advance, s, ct);
}

int launch_stop_match(const int32_t* hist, int ld_hist, const int32_t* hist_len, int B, const ConstrainTable* ct, int32_t* fired, hipStream_t s) {
    if (B < 1 || B > 65535 || ld_hist < 0 || !hist || !hist_len || !ct || !fired) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(stop_match_kernel, dim3(B), dim3(CONSTRAIN_THREADS), 0, s, hist, ld_hist, hist_len, ct, fired);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
