// trace_op_sample: the device sampler (sample.h) over loose rows of masked head logits — the kernel-level entry of the tests and the sampler of
// the host-driven (stopping-criteria) decode loop.  The decode step itself samples inside select_next_kernel<SELECT_SAMPLE> (select.hip): the same
// sample_row, so both paths pick the same id from the same row, params, step and row index.
#include "common.h"
#include "kernels.h"
#include "sample.h"

namespace {

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_rows_kernel(const float* __restrict__ logits, int ld, const int32_t* __restrict__ heads,
                                                                     int V, int Tv, int Sv, SampleParams sp, const int32_t* __restrict__ steps,
                                                                     int32_t* __restrict__ out_ids) {
    __shared__ SampleLds L;
    const int b = blockIdx.x;
    const int head = heads[b];
    const int lo = head == 0 ? 0 : (head == 1 ? V + 1 : V + 1 + Tv);       // head_bounds (common.h), written out: the call compiles to another stream here
    const int hi = head == 0 ? V + 1 : (head == 1 ? V + 1 + Tv : V + 1 + Tv + Sv);
    const int id = lo + sample_row(logits + (size_t)b * ld + lo, hi - lo, sp, (uint32_t)steps[b], (uint32_t)b, L);
    if (threadIdx.x == 0) out_ids[b] = id;
}

// The log-probability of one token per row (sample.h token_logprob_row), one workgroup per row, in two forms that share every line of arithmetic:
//   loose rows (heads != null): row b's token is ids[b], its head heads[b]; out[b].  An id outside the head's range gives -inf.
//   decode step (heads == null): launched after select_next_kernel, which has recorded this step's token and advanced the counter: the row's step is
//     *step - 1 - step0[b], the token out_ids[b][step]; the head it was drawn from is the one whose id range holds it (the three ranges are disjoint).
//     Only rows select_next recorded a token for in this step (out_len[b] == step + 1) write out[b][step]; rows that finished earlier and
//     steps at or past max_new (the row's own, where the batch carries per-row bounds) leave `out` untouched.
__global__ __launch_bounds__(SAMPLE_THREADS) void token_logprob_kernel(const float* __restrict__ logits, int ld, const int32_t* __restrict__ heads,
                                                                       int V, int Tv, int Sv, const int32_t* __restrict__ ids,
                                                                       float* __restrict__ out, const int32_t* __restrict__ step_ctr,
                                                                       const int32_t* __restrict__ out_len, const int32_t* __restrict__ params,
                                                                       const int32_t* __restrict__ step0,
                                                                       const int32_t* __restrict__ row_max_new) {
    __shared__ float fbuf[SAMPLE_THREADS];
    __shared__ float wmax[4];
    const int b = blockIdx.x;
    int id, head;
    size_t o;
    if (heads) {
        id = ids[b];
        head = heads[b];
        o = (size_t)b;
    } else {
        const int step = step_ctr[0] - 1 - (step0 ? step0[b] : 0), max_new = params[0];     // the row's own step (StepState::step0)
        if (step < 0 || step >= (row_max_new ? row_max_new[b] : max_new) || out_len[b] != step + 1) return;       // (uniform over the workgroup; the row's own bound where the batch carries one, StepState::row_max_new)
        id = ids[(size_t)b * max_new + step];
        head = id <= V ? 0 : (id < V + 1 + Tv ? 1 : 2);
        o = (size_t)b * max_new + step;
    }
    const int lo = head == 0 ? 0 : (head == 1 ? V + 1 : V + 1 + Tv);       // (head_bounds written out, as above)
    const int hi = head == 0 ? V + 1 : (head == 1 ? V + 1 + Tv : V + 1 + Tv + Sv);
    const float lp = token_logprob_row(logits + (size_t)b * ld + lo, hi - lo, id >= lo && id < hi ? id - lo : -1, fbuf, wmax);
    if (threadIdx.x == 0) out[o] = lp;
}

}  // namespace

int launch_sample_rows(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const SampleParams& sp, const int32_t* steps,
                       int32_t* out_ids, hipStream_t s) {
    if (B < 1 || B > 65535 || ld < V + 1 + Tv + Sv || V < 1 || Tv < 1 || Sv < 1) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, s, logits, ld, heads, V, Tv, Sv, sp, steps, out_ids);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_token_logprob(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const int32_t* ids, float* out, hipStream_t s) {
    if (B < 1 || B > 65535 || ld < V + 1 + Tv + Sv || V < 1 || Tv < 1 || Sv < 1 || !heads) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(token_logprob_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, s, logits, ld, heads, V, Tv, Sv, ids, out, nullptr, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_step_logprob(const float* logits, const StepState& st, int B, int V, int Tv, int Sv, float* out_logprobs, hipStream_t s) {
    if (B < 1 || B > SK_ROWS || !logits || !out_logprobs) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(token_logprob_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, s, logits, V + 1 + Tv + Sv, nullptr, V, Tv, Sv, st.out_ids, out_logprobs,
                       st.step, st.out_len, st.params, st.step0, st.row_max_new);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
