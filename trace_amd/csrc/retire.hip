// Retiring rows of a running decode batch (trace_decode_retire): new row i of every per-row array of the decode step is former row keep[i].
// An in-place gather would race — row i is at once the destination of keep[i] and the source of some j < i, in another workgroup — so the rows go
// through a scratch copy: phase 0 reads array row keep[i] into scratch row i, phase 1 (the next launch on the stream) writes scratch row i to array
// row i.  The arrays keep their addresses, which the captured step graphs hold.  One workgroup per (kept row, segment):
//   segment 0: the seven one-int-per-row arrays (slots, pos, heads, done, out_len, row_id, step0);
//   segments 1-3: the rows at stride max_new (out_ids, forced, log-probabilities where armed), 16 bytes per lane when max_new % 4 == 0 (every row
//     then starts on a 16-byte boundary), 4 bytes per lane otherwise;
//   segment 4: the row of the next step's input embedding (H 16-bit elements, H % 8 == 0), 16 bytes per lane;
//   segment 5 (a batch begun with per-row parameters only): the row's SampleParams, LogitsParams and max_new, 14 ints.
// A row that stays where it is (keep[i] == i: the rows in front of the first retired one) is not touched in either phase.
#include "common.h"
#include "kernels.h"

namespace {

__device__ __forceinline__ void retire_copy(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int n, bool vec, int tid) {
    if (vec) {
        for (int c = tid; c < (n >> 2); c += 256) reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(src)[c];
    } else {
        for (int c = tid; c < n; c += 256) dst[c] = src[c];
    }
}

__global__ __launch_bounds__(256) void retire_rows_kernel(RetireArgs a, const int32_t* __restrict__ keep, int32_t* __restrict__ scratch, int B, int phase) {
    const int i = blockIdx.x, seg = blockIdx.y, tid = threadIdx.x;
    const int k = keep[i];
    if (k == i || (unsigned)k >= (unsigned)B) return;      // in place already / (the host checked the list: never out of range)
    const int mn4 = (a.max_new + 3) & ~3;
    int32_t* srow = scratch + (size_t)i * retire_row_ints(a.max_new, a.H);
    const int r = phase == 0 ? k : i;                       // the array row this workgroup reads (phase 0) or writes (phase 1)
    if (seg == 0) {
        int32_t* p = nullptr;
#pragma unroll
        for (int q = 0; q < RETIRE_SMALL; ++q)
            if (tid == q) p = a.small[q];
        if (p) {
            if (phase == 0) srow[tid] = p[r];
            else p[r] = srow[tid];
        }
    } else if (seg <= 3) {
        int32_t* w = seg == 1 ? a.wide[0] : seg == 2 ? a.wide[1] : a.wide[2];
        if (!w) return;
        int32_t* arow = w + (size_t)r * a.max_new;
        int32_t* s = srow + 8 + (seg - 1) * mn4;
        if (phase == 0) retire_copy(arow, s, a.max_new, (a.max_new & 3) == 0, tid);
        else retire_copy(s, arow, a.max_new, (a.max_new & 3) == 0, tid);
    } else if (seg == 5) {
        // the per-row generation parameters (launched only for a batch that carries them): three arrays of 10, 3 and 1 ints per row, one lane per int
        int q = 0, off = tid;
        while (q < 3 && off >= retire_rowp_ints(q)) off -= retire_rowp_ints(q++);
        if (q < 3 && a.rowp[q]) {
            int32_t* p = a.rowp[q] + (size_t)r * retire_rowp_ints(q) + off;
            int32_t* s = srow + 8 + 3 * mn4 + (a.H >> 1) + tid;
            if (phase == 0) *s = *p;
            else *p = *s;
        }
    } else {
        int32_t* arow = reinterpret_cast<int32_t*>(a.x + (size_t)r * a.H);
        int32_t* s = srow + 8 + 3 * mn4;
        if (phase == 0) retire_copy(arow, s, a.H >> 1, true, tid);
        else retire_copy(s, arow, a.H >> 1, true, tid);
    }
}

}  // namespace

int launch_retire(const RetireArgs& a, const int32_t* keep, int n_keep, int B, int32_t* scratch, hipStream_t s) {
    if (B < 1 || B > SK_ROWS || n_keep < 1 || n_keep > B || a.max_new < 1 || a.H < 8 || a.H % 8 || !keep || !scratch || !a.x) return TRACE_ERR_ARG;
    for (int q = 0; q < RETIRE_SMALL; ++q)
        if (!a.small[q]) return TRACE_ERR_ARG;
    if (!a.wide[0] || !a.wide[1] || (a.rowp[0] != nullptr) != (a.rowp[1] != nullptr) || (a.rowp[0] != nullptr) != (a.rowp[2] != nullptr)) return TRACE_ERR_ARG;
    for (int phase = 0; phase < 2; ++phase)
        hipLaunchKernelGGL(retire_rows_kernel, dim3(n_keep, a.rowp[0] ? 6 : 5), dim3(256), 0, s, a, keep, scratch, B, phase);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
