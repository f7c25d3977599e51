// trace_op_sample: the device sampler (sample.h) over loose rows of masked head logits — the kernel-level entry of the tests and the sampler of
// the host-driven (stopping-criteria) decode loop.  The decode step itself samples inside select_next_kernel<true> (decode.hip): the same
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
    const int lo = head == 0 ? 0 : (head == 1 ? V + 1 : V + 1 + Tv);
    const int hi = head == 0 ? V + 1 : (head == 1 ? V + 1 + Tv : V + 1 + Tv + Sv);
    const int id = lo + sample_row(logits + (size_t)b * ld + lo, hi - lo, sp, (uint32_t)steps[b], (uint32_t)b, L);
    if (threadIdx.x == 0) out_ids[b] = id;
}

}  // namespace

int launch_sample_rows(const float* logits, int ld, int B, const int32_t* heads, int V, int Tv, int Sv, const SampleParams& sp, const int32_t* steps,
                       int32_t* out_ids, hipStream_t s) {
    if (B < 1 || B > 65535 || ld < V + 1 + Tv + Sv || V < 1 || Tv < 1 || Sv < 1) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(sample_rows_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, s, logits, ld, heads, V, Tv, Sv, sp, steps, out_ids);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
