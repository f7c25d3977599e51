// select_next_kernel, the token selection of a decode step, as a template three translation units instantiate: select.hip the plain forms, constrain.hip
// the forms with the stop match of constrain.h (STOP), select_rows.hip the per-row form with and without it.  One workgroup per sequence.
#pragma once
#include "common.h"
#include "constrain.h"
#include "kernels.h"
#include "sample.h"

namespace {

// one workgroup per sequence.  `step` is shared: every workgroup reads it first, then checks in; the last one to
// check in advances it (so no workgroup can observe the next step's value).  `local` = step - st.step0[b] is the row's own step (a row admitted into a
// running batch, trace_decode_admit, began later than the counter): the index into out_ids / forced, out_len, the max_new guards, the Philox counter
// and the stop match's length are the row's; only the check-in works on the shared value.
// SELECT_TILES: the arg-max over head_logits_kernel's tile partials (greedy).  SELECT_SAMPLE: the token is drawn by sample_row (sample.h)
// from the masked logits in `logits` [B, V+1+Tv+Sv] (head_logits_kernel's rows, or logits_process_kernel's) under the device-resident params
// *sp, with the step counter and the row index as the Philox counter.  SELECT_ROW: the arg-max over the row's head range [lo, hi) of `logits`
// (logits_process_kernel's rows), the lowest id among equal maxima as the tile partials have it; a range that is -inf throughout gives lo.
// SELECT_PER_ROW: the generation parameters are the row's own (trace_decode_set_row_params) — st.row_sp[b].temperature > 0: SELECT_SAMPLE's draw
// under st.row_sp[b] (its params, its seed; the same counter); otherwise SELECT_ROW's arg-max — and st.row_max_new[b] stands in every max_new guard
// (the record, the advance of pos, the forced-id read, the stop match's length) while params[0] stays the stride of out_ids / forced: a row that has
// recorded its own max_new ids is stepped on as a row past max_new is after an admission.  An instantiation of its own: the other three compile as before.
// Forced ids, EOS, record_feed and the head switch are the same code in all four.
// STOP: the stop rule of constrain.h over the table *ct.  Once thread 0 has recorded the token and the workgroup has met at the barrier below, thread i
// compares stop sequence i with the tail of out_ids[b] (stop_match_row) and the workgroup's OR sets done[b] — before the kernel ends, so the next
// step's selection sees it in stream order.  Only a row that recorded in this step is matched.  Without STOP nothing of it is compiled.
template <int MODE, bool STOP>
__global__ __launch_bounds__(256) void select_next_kernel(const float* __restrict__ part_val, const int32_t* __restrict__ part_idx,
                                                          StepState st, const bf16_t* __restrict__ embed,
                                                          const bf16_t* __restrict__ time_tab, const bf16_t* __restrict__ score_tab,
                                                          const bf16_t* __restrict__ sync_row, bf16_t* __restrict__ xnext, int ldx,
                                                          int B, int H, int V, int Tv, int Sv, int ntiles, int advance,
                                                          const float* __restrict__ logits, const SampleParams* __restrict__ sp,
                                                          const ConstrainTable* __restrict__ ct) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int s_feed;
    __shared__ int s_len;              // STOP: the row's length if it recorded in this step, else 0
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int b = blockIdx.x;
    const int step = __hip_atomic_load(st.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int local = step - (st.step0 ? st.step0[b] : 0);     // the row's own step: everything below that belongs to the row uses it, the check-in alone the shared value
    const int max_new = st.params[0], eos = st.params[1], record_feed = st.params[2];
    __syncthreads();
    if (tid == 0) {
        const int arrived = __hip_atomic_fetch_add(st.step + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == B - 1) {
            __hip_atomic_store(st.step + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(st.step, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    float v = -INFINITY;
    int idx = 0x7fffffff;
    bool sampled = MODE == SELECT_SAMPLE;                     // SELECT_PER_ROW: the row's own temperature decides — one workgroup is one row, so the branch is uniform
    int own_max = max_new;                                    // the bound of every max_new guard below; max_new itself stays the stride of out_ids / forced
    if constexpr (MODE == SELECT_PER_ROW) { sampled = st.row_sp[b].temperature > 0.f; own_max = st.row_max_new[b]; }
    if constexpr (MODE == SELECT_SAMPLE || MODE == SELECT_PER_ROW) {
        __shared__ SampleLds L;
        if (sampled) {
            int lo, hi;
            head_bounds(st.heads[b], V, Tv, Sv, lo, hi);
            const SampleParams* rp = sp;
            if constexpr (MODE == SELECT_PER_ROW) rp = st.row_sp + b;            // ITS params and ITS seed; the counter stays (local, 0, row_id[b], 0)
            [[clang::always_inline]] idx = lo + sample_row(logits + (size_t)b * (V + 1 + Tv + Sv) + lo, hi - lo, *rp, (uint32_t)local,
                                   (uint32_t)(st.row_id ? st.row_id[b] : b), L);      // (a row keeps the index it had at trace_decode_begin: trace_decode_retire)
        }
    }
    if constexpr (MODE != SELECT_SAMPLE) {
    if (!sampled) {
    if constexpr (MODE == SELECT_ROW || MODE == SELECT_PER_ROW) {
        int lo, hi;
        head_bounds(st.heads[b], V, Tv, Sv, lo, hi);
        const float* row = logits + (size_t)b * (V + 1 + Tv + Sv);
        for (int i0 = lo + tid; i0 < hi; i0 += 4 * 256) {                // four loads in flight per thread (one row per workgroup: latency-bound)
            float x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = i0 + q * 256 < hi ? row[i0 + q * 256] : -INFINITY;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int oi = i0 + q * 256;
                if (oi < hi && (x[q] > v || (x[q] == v && oi < idx))) { v = x[q]; idx = oi; }
            }
        }
    } else {
    for (int t = tid; t < ntiles; t += 256) {
        const float ov = part_val[(size_t)b * ntiles + t];
        const int oi = part_idx[(size_t)b * ntiles + t];
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    if (lane == 0) { sv[wid] = v; si[wid] = idx; }
    __syncthreads();
    }
    }
    if (tid == 0) {
        if (!sampled)
        for (int w = 1; w < 4; ++w)
            if (sv[w] > v || (sv[w] == v && si[w] < idx)) { v = sv[w]; idx = si[w]; }
        int tok = idx;
        if (advance && local < own_max) st.pos[b] += 1;     // (the host bounds the step count too: engine.hip trace_decode_steps)
        int feed = tok;
        if (local < own_max) {
            const int f = st.forced[(size_t)b * max_new + local];
            if (f >= 0) feed = f;
        }
        if (record_feed) tok = feed;          // host-driven sampling: the emitted token is the one fed back
        const bool was_done = st.done[b] != 0;
        if constexpr (STOP) s_len = !was_done && local < own_max ? local + 1 : 0;
        if (!was_done && local < own_max) {
            st.out_ids[(size_t)b * max_new + local] = tok;
            st.out_len[b] = local + 1;
            if (eos >= 0 && tok == eos) st.done[b] = 1;
        }
        // head switch (trace_mistral.py:86-88): V -> time(1), V+1 -> score(2), V+Tv+1 -> text(0)
        int hd = st.heads[b];
        if (feed == V) hd = 1; else if (feed == V + 1) hd = 2; else if (feed == V + Tv + 1) hd = 0;
        st.heads[b] = hd;
        s_feed = feed;
    }
    __syncthreads();
    if constexpr (STOP) {
        const int len = s_len;                                           // (uniform: 0 = nothing recorded, nothing to match)
        if (len > 0 && stop_match_row(st.out_ids + (size_t)b * max_new, len, ct) && tid == 0) st.done[b] = 1;
    }
    const int feed = s_feed;
    const bf16_t* src;
    if (feed == V) src = sync_row;
    else if (feed > V && feed < V + 1 + Tv) src = time_tab + (size_t)(feed - V - 1) * H;
    else if (feed >= V + 1 + Tv) src = score_tab + (size_t)(feed - V - 1 - Tv) * H;
    else src = embed + (size_t)(feed % V) * H;
    for (int c = tid; c < (H >> 3); c += 256)
        *reinterpret_cast<uint4*>(xnext + (size_t)b * ldx + c * 8) = *reinterpret_cast<const uint4*>(src + c * 8);
}

}  // namespace

// the launch of one of the three batch-wide forms (launch_select's argument checks come first); SELECT_PER_ROW is select_rows.hip's
template <bool STOP>
inline int launch_select_forms(int form, const float* part_val, const int32_t* part_idx, const float* logits, const SampleParams* sp, const StepState& st,
                               const bf16_t* embed, const bf16_t* time_tab, const bf16_t* score_tab, const bf16_t* sync_row, bf16_t* xnext, int ldx, int B,
                               int H, int V, int Tv, int Sv, int advance, hipStream_t s, const ConstrainTable* ct) {
    const int ntiles = (V + 1 + Tv + Sv + 15) / 16;
    const dim3 grid(B), block(256);
#define SELECT_LAUNCH(MODE)                                                                                                                             \
    hipLaunchKernelGGL((select_next_kernel<MODE, STOP>), grid, block, 0, s, part_val, part_idx, st, embed, time_tab, score_tab, sync_row, xnext, ldx, B, H, V, \
                       Tv, Sv, ntiles, advance, logits, sp, ct)
    if (form == SELECT_TILES) SELECT_LAUNCH(SELECT_TILES);
    else if (form == SELECT_SAMPLE) SELECT_LAUNCH(SELECT_SAMPLE);
    else if (form == SELECT_ROW) SELECT_LAUNCH(SELECT_ROW);
    else return TRACE_ERR_ARG;
#undef SELECT_LAUNCH
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
