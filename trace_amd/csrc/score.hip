// Scoring GIVEN tokens: log-probabilities of thousands of final-norm hidden rows at once, each row under a head of its own, without ever
// writing the [R, V + 1 + Tv + Sv] fp32 logits (1 GB at the 8192-row prefill workspace).  The semantics are stated in include/trace_hip.h
// (trace_llm_score_append); trace_amd/sampling.py score_logprob_ref restates the sums below in float32 numpy bit for bit.
//
//   score_head_kernel   text-head rows x the V + 1 rows of the lm | sync block of the head matrix: a 16-bit MFMA GEMM (K = hidden, fp32 accumulators)
//                       on 128 x 128 tiles.  Column tile j covers the absolute columns [j CT, (j + 1) CT), CT = 128, clipped to the head's range.
//                       The accumulators go to LDS as an fp32 [128][128] tile; two threads per row (one per 64-column HALF of the tile) then form
//                         m_j = max x                                       over the tile's in-range columns
//                         s_j = h0 + h1,  h = sum exp(x_c - m_j)            each half summed sequentially in ascending column order from 0
//                         x_t                                               if the row's target column lies in the tile
//                       and store them with ordinary vector stores: exactly one workgroup writes each (row, tile) cell, no atomics.
//   score_merge_kernel  one wave per row: M = max_j m_j, S = sum_j s_j exp(m_j - M) sequentially in ascending j from 0, logprob = (x_t - M) - log S.
//                       Rows under the time / score head (at most 128 ids wide, so at most two column tiles) never meet the GEMM: the wave computes
//                       their few dot products straight from the hidden row and forms the same tile sums itself.
// exp / log are sample.h's sample_exp / sample_log; nothing below is contracted into an FMA.
//
// Why a main loop of its own and not an epilogue of gemm.hip's kernel: that kernel's N must be a multiple of its tile (the head block has
// V + 1 = 32001 rows: the last tile's weight rows are clamped here and its columns masked), its epilogue is a 16-bit LDS image sharing one
// template with five other epilogues, and its workgroups must be able to leave early (a row panel without text rows does no work here).  The loop
// is gemm.hip's 128 x 128 x 64 double-buffered LDS-DMA loop (same swizzle, same fragment reads, same MFMA order), stripped of its fp8 / tiled-weight /
// ring forms.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "sample.h"

namespace {

constexpr int SC_BM = 128, SC_CT = SCORE_TILE, SC_THR = 256;
constexpr int SC_HALF = SC_CT / 2;
constexpr int SC_HSTRIDE = SC_HALF + 1, SC_TSTRIDE = 2 * SC_HSTRIDE;      // fp32 tile in LDS: [row][half][65] — the 64 lanes of a wave (32 rows x 2 halves) read 64 different banks
constexpr int SC_LOOP_BYTES = 2 * (SC_BM + SC_CT) * 128, SC_TILE_BYTES = SC_BM * SC_TSTRIDE * 4;
constexpr int SC_LDS = SC_LOOP_BYTES > SC_TILE_BYTES ? SC_LOOP_BYTES : SC_TILE_BYTES;
constexpr int SC_SMALL_MAX = 128;                                          // widest time / score head the merge kernel computes itself
static_assert(SC_CT == 128 && SC_BM == 128, "the wave layout below is 2 x 2 waves of 64 x 64");

struct ScoreArgs {
    const bf16_t* X; int ld;         // [R, K] final-norm hidden rows
    const bf16_t* W; int ldw;        // [V + 1 + Tv + Sv, K] head rows in global vocabulary order
    int K, R;
    const int32_t* heads;            // [R] 0 text, 1 time, 2 score
    const int32_t* ids;              // [R] target id, -1 = ignore
    int V, Tv, Sv, NT;               // NT = column tiles of the text head
    float* tm; float* ts; float* xt; // workspace: [R][NT], [R][NT], [R]
    float* out;                      // [R]
};

__device__ __forceinline__ int sc_swz(int row, int kc) { return row * 128 + ((kc ^ ((row >> 1) & 7)) << 4); }

__global__ __launch_bounds__(SC_THR) void score_head_kernel(ScoreArgs p) {
#pragma clang fp contract(off)
    constexpr int TM = 4, TN = 4, A_BYTES = SC_BM * 128, STAGE = A_BYTES + SC_CT * 128, IT = SC_BM * 8 / SC_THR;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = lane & 15, g = lane >> 4, wm = wid >> 1, wn = wid & 1;
    const int ntn = p.NT, ntm = (p.R + SC_BM - 1) / SC_BM;
    const int t = xcd_remap(blockIdx.x, ntm * ntn);
    int tm, tn;
    {                                                           // gemm.hip's order: 8 row panels x all column tiles share their panels through one XCD's L2
        constexpr int GM = 8;
        const int per_group = GM * ntn;
        const int gid = t / per_group, first = gid * GM;
        const int gsz = min(ntm - first, GM);
        const int in_g = t - gid * per_group;
        tm = first + in_g % gsz;
        tn = in_g / gsz;
    }
    const int m0 = tm * SC_BM, n0 = tn * SC_CT;
    const int hi = p.V + 1;                                     // the text head's range is [0, V + 1)
    // a row takes part iff it is a text row whose target lies in the head: every other row's answer (0, -inf, or a small head) is the merge kernel's
    int active = 0;
    if (tid < SC_BM && m0 + tid < p.R) {
        const int id = p.ids[m0 + tid];
        active = p.heads[m0 + tid] == 0 && id >= 0 && id < hi;
    }
    if (!__syncthreads_or(active)) return;

    const char* asrc[IT];
    const char* wsrc[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const int slot = i * SC_THR + tid, row = slot >> 3, kc = (slot & 7) ^ ((row >> 1) & 7);
        asrc[i] = reinterpret_cast<const char*>(p.X) + ((size_t)min(m0 + row, p.R - 1) * p.ld + kc * 8) * 2;
        wsrc[i] = reinterpret_cast<const char*>(p.W) + ((size_t)min(n0 + row, hi - 1) * p.ldw + kc * 8) * 2;      // rows past <sync> are clamped, their columns masked below
    }
    auto issue = [&](int kt) {
        char* sa = smem + (kt & 1) * STAGE;
        char* sw = sa + A_BYTES;
        const int ko = kt * 128;
#pragma unroll
        for (int i = 0; i < IT; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + ko),
                                             (__attribute__((address_space(3))) void*)(sa + (i * SC_THR + wid * 64) * 16), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < IT; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[i] + ko),
                                             (__attribute__((address_space(3))) void*)(sw + (i * SC_THR + wid * 64) * 16), 16, 0, 0);
    };
    f32x4_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int aoff[TM], woff[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aoff[i] = sc_swz(wm * 64 + i * 16 + r, g);
#pragma unroll
    for (int j = 0; j < TN; ++j) woff[j] = sc_swz(wn * 64 + j * 16 + r, g);

    const int nk = p.K / 64;
    issue(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                                        // tile kt landed (vmcnt(0) + barrier); everyone is done with tile kt - 1
        if (kt + 1 < nk) issue(kt + 1);
        const char* sa = smem + (kt & 1) * STAGE;
        const char* sw = sa + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8_t wf[TN], af[TM];
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[j] = *reinterpret_cast<const bf16x8_t*>(sw + (woff[j] ^ (ks << 6)));
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(sa + (aoff[i] ^ (ks << 6)));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = mfma16(wf[j], af[i], acc[i][j]);
        }
    }
    __syncthreads();                                            // every wave is done reading the last K-tile: the fp32 tile takes the buffers' place
    float* T = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = wm * 64 + i * 16 + r;                   // lane (r, g) holds 4 consecutive columns of this row per column block
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = wn * 64 + j * 16 + g * 4;
            float* dst = T + row * SC_TSTRIDE + (col >> 6) * SC_HSTRIDE + (col & 63);
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = acc[i][j][q];
        }
    }
    __syncthreads();
    // two threads per row (neighbouring lanes): thread `half` owns the tile's columns [half 64, half 64 + 64)
    const int row = tid >> 1, half = tid & 1;
    const int gr = min(m0 + row, p.R - 1);
    const int id = p.ids[gr];
    const bool live = m0 + row < p.R && p.heads[gr] == 0 && id >= 0 && id < hi;
    const float* th = T + row * SC_TSTRIDE + half * SC_HSTRIDE;
    const int nvalid = max(0, min(SC_HALF, hi - (n0 + half * SC_HALF)));      // in-range columns of this half (the head starts at column 0)
    float m = -INFINITY;
    for (int c = 0; c < nvalid; ++c) m = fmaxf(m, th[c]);
    m = fmaxf(m, __shfl_xor(m, 1, 64));
    float s = 0.f;
    for (int c = 0; c < nvalid; ++c) s = s + sample_exp(th[c] - m);
    const float so = __shfl_xor(s, 1, 64);
    if (!live) return;
    if (half == 0) {
        p.tm[(size_t)gr * p.NT + tn] = m;
        p.ts[(size_t)gr * p.NT + tn] = s + so;                 // h0 + h1
    }
    const int tc = id - n0 - half * SC_HALF;
    if (tc >= 0 && tc < SC_HALF) p.xt[gr] = th[tc];
}

// One wave per row.  lds: max(NT, SC_SMALL_MAX) floats.
__global__ __launch_bounds__(64) void score_merge_kernel(ScoreArgs p) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float buf[];
    const int row = blockIdx.x, lane = threadIdx.x;
    const int head = p.heads[row], id = p.ids[row];
    const int lo = head == 0 ? 0 : (head == 1 ? p.V + 1 : p.V + 1 + p.Tv);   // head_bounds (common.h), written out: the call compiles to another stream here
    const int hi = head == 0 ? p.V + 1 : (head == 1 ? p.V + 1 + p.Tv : p.V + 1 + p.Tv + p.Sv);
    if (id < lo || id >= hi) {                                  // (uniform over the wave)
        if (lane == 0) p.out[row] = id == -1 ? 0.f : -INFINITY;
        return;
    }
    if (head == 0) {
        const float* tm = p.tm + (size_t)row * p.NT;
        const float* ts = p.ts + (size_t)row * p.NT;
        float M = -INFINITY;
        for (int j = lane; j < p.NT; j += 64) M = fmaxf(M, tm[j]);
        M = wave_max(M);
        for (int j = lane; j < p.NT; j += 64) buf[j] = ts[j] * sample_exp(tm[j] - M);
        __syncthreads();
        if (lane == 0) {
            float S = 0.f;
            int j = 0;
            for (; j + 4 <= p.NT; j += 4) {                     // ascending j; the four reads are issued together, the adds stay sequential
                const float a = buf[j], b = buf[j + 1], c = buf[j + 2], d = buf[j + 3];
                S = S + a; S = S + b; S = S + c; S = S + d;
            }
            for (; j < p.NT; ++j) S = S + buf[j];
            p.out[row] = (p.xt[row] - M) - sample_log(S);
        }
        return;
    }
    // time / score head: the hi - lo dot products straight from the hidden row (fp32 products and sums, lanes stride the 16-byte chunks of K)
    const bf16_t* x = p.X + (size_t)row * p.ld;
    for (int c = lo; c < hi; ++c) {
        const bf16_t* w = p.W + (size_t)c * p.ldw;
        float a = 0.f;
        for (int k = lane * 8; k < p.K; k += 512) {
            const uint4 xv = *reinterpret_cast<const uint4*>(x + k), wv = *reinterpret_cast<const uint4*>(w + k);
            a = a + bflo(xv.x) * bflo(wv.x); a = a + bfhi(xv.x) * bfhi(wv.x);
            a = a + bflo(xv.y) * bflo(wv.y); a = a + bfhi(xv.y) * bfhi(wv.y);
            a = a + bflo(xv.z) * bflo(wv.z); a = a + bfhi(xv.z) * bfhi(wv.z);
            a = a + bflo(xv.w) * bflo(wv.w); a = a + bfhi(xv.w) * bfhi(wv.w);
        }
        a = wave_sum(a);
        if (lane == 0) buf[c - lo] = a;
    }
    __syncthreads();
    if (lane != 0) return;
    // the same tile rule on absolute columns: at most two tiles (hi - lo <= 128), each as two halves
    float mj[2] = {-INFINITY, -INFINITY}, sj[2] = {0.f, 0.f};
    const int j0 = lo / SC_CT, j1 = (hi - 1) / SC_CT;
    for (int j = j0; j <= j1; ++j) {
        const int a = max(lo, j * SC_CT), b = min(hi, (j + 1) * SC_CT), mid = j * SC_CT + SC_HALF;
        float m = -INFINITY;
        for (int c = a; c < b; ++c) m = fmaxf(m, buf[c - lo]);
        float h0 = 0.f, h1 = 0.f;
        for (int c = a; c < min(b, mid); ++c) h0 = h0 + sample_exp(buf[c - lo] - m);
        for (int c = max(a, mid); c < b; ++c) h1 = h1 + sample_exp(buf[c - lo] - m);
        mj[j - j0] = m;
        sj[j - j0] = h0 + h1;
    }
    const float M = fmaxf(mj[0], mj[1]);
    float S = 0.f;
    for (int j = j0; j <= j1; ++j) S = S + sj[j - j0] * sample_exp(mj[j - j0] - M);
    p.out[row] = (buf[id - lo] - M) - sample_log(S);
}

}  // namespace

int score_tiles(int V) { return (V + 1 + SC_CT - 1) / SC_CT; }
size_t score_ws_floats(int R, int V) { return (size_t)R * (2 * (size_t)score_tiles(V) + 1); }

int launch_score_rows(const bf16_t* X, int ld, const bf16_t* W, int ldw, int K, int R, const int32_t* heads, const int32_t* ids, int V, int Tv, int Sv,
                      float* ws, float* out, hipStream_t s) {
    if (!X || !W || !heads || !ids || !ws || !out) return TRACE_ERR_ARG;
    if (R < 1 || R > SCORE_MAX_ROWS || V < 1 || Tv < 1 || Sv < 1 || Tv > SC_SMALL_MAX || Sv > SC_SMALL_MAX) return TRACE_ERR_ARG;
    if (K < 64 || K % 64 || ld < K || ldw < K || (ld % 8) || (ldw % 8)) return TRACE_ERR_ARG;
    ScoreArgs p{};
    p.X = X; p.ld = ld; p.W = W; p.ldw = ldw; p.K = K; p.R = R; p.heads = heads; p.ids = ids; p.V = V; p.Tv = Tv; p.Sv = Sv;
    p.NT = score_tiles(V);
    p.tm = ws; p.ts = ws + (size_t)R * p.NT; p.xt = ws + 2 * (size_t)R * p.NT; p.out = out;
    static LdsGrant grant;
    if (!grant_dynamic_lds(grant, reinterpret_cast<const void*>(score_head_kernel), SC_LDS)) return TRACE_ERR_HIP;
    const int nblk = ((R + SC_BM - 1) / SC_BM) * p.NT;
    hipLaunchKernelGGL(score_head_kernel, dim3(nblk), dim3(SC_THR), SC_LDS, s, p);
    if (hipGetLastError() != hipSuccess) return TRACE_ERR_HIP;
    const int mlds = std::max(p.NT, SC_SMALL_MAX) * 4;
    hipLaunchKernelGGL(score_merge_kernel, dim3(R), dim3(64), mlds, s, p);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
