// The e4m3 KV cache ("kv8", include/trace_hip.h states the format): K and V as OCP e4m3fn bytes with one fp32 scale per position and kv head,
// quantised by the rule of fp8.hip's quant_rows_fp8 over the 128 values of a row (amax / 448, 1 for an all-zero row).  264 bytes per position and
// kv head instead of 512.  Layouts:
//   K8 [slot][kvh][ctx_pad][128]          bytes, row-major like the 16-bit K cache
//   V8 [slot][kvh][ctx_pad / 32][128][32] bytes, position-blocked V^T: a 32-position block is 4 KB contiguous, byte (d, p % 32) of block p / 32
//   ks, vs [slot][kvh][ctx_pad]           fp32
// The payload is widened to the element type in registers (exact: every finite e4m3 value is a bf16 and an fp16 value) and goes through the 16-bit
// MFMAs; q and P are never narrowed.  The scales never touch the payload: ks[j] multiplies the score of position j, vs[j] its probability on the way
// into the PV product, and l sums the unscaled probabilities.
// This file: the decode attention over such a cache, the decode step's append (qkv_finish), and the two movers between the 16-bit layouts and kv8.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
constexpr float FP8_MAX = 448.f;
constexpr int HD = 128;

__device__ __forceinline__ uint32_t cvt4_fp8(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}
// 8 e4m3 bytes (two dwords, element order = byte order) -> 8 elements of the build's 16-bit type
__device__ __forceinline__ bf16x8_t widen8(uint32_t d0, uint32_t d1) {
#ifdef TRACE_F16
    typedef __attribute__((ext_vector_type(2))) _Float16 pair_t;
#define KV8_WIDEN __builtin_amdgcn_cvt_scalef32_pk_f16_fp8
#else
    typedef __attribute__((ext_vector_type(2))) __bf16 pair_t;
#define KV8_WIDEN __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8
#endif
    union { bf16x8_t v; pair_t p[4]; } u;
    u.p[0] = KV8_WIDEN(d0, 1.0f, false);
    u.p[1] = KV8_WIDEN(d0, 1.0f, true);
    u.p[2] = KV8_WIDEN(d1, 1.0f, false);
    u.p[3] = KV8_WIDEN(d1, 1.0f, true);
#undef KV8_WIDEN
    return u.v;
}
// the four e4m3 bytes of a dword as fp32
__device__ __forceinline__ void f32_of_fp8x4(uint32_t w, float (&f)[4]) {
    f[0] = __builtin_amdgcn_cvt_f32_fp8((int)w, 0);
    f[1] = __builtin_amdgcn_cvt_f32_fp8((int)w, 1);
    f[2] = __builtin_amdgcn_cvt_f32_fp8((int)w, 2);
    f[3] = __builtin_amdgcn_cvt_f32_fp8((int)w, 3);
}
// the row rule on 16 values a lane holds of a 128-wide row shared by 8 consecutive lanes: amax over the row -> scale, 16 bytes (value order)
__device__ __forceinline__ float quant16_of_row(const float (&x)[16], uint32_t (&q)[4]) {
    float am = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) am = fmaxf(am, fabsf(x[e]));
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    am = fmaxf(am, __shfl_xor(am, 2, 64));
    am = fmaxf(am, __shfl_xor(am, 4, 64));
    const float inv = am > 0.f ? FP8_MAX / am : 1.f;
    float f[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) f[e] = fminf(fmaxf(x[e] * inv, -FP8_MAX), FP8_MAX);
#pragma unroll
    for (int w = 0; w < 4; ++w) q[w] = cvt4_fp8(f[4 * w], f[4 * w + 1], f[4 * w + 2], f[4 * w + 3]);
    return am > 0.f ? am / FP8_MAX : 1.f;
}
__device__ __forceinline__ void unpack_pairs(const uint32_t (&u)[4], float* x) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = bflo(u[e]); x[2 * e + 1] = bfhi(u[e]); }
}

// ---------------------------------------------------------------------------------------------------------
// Single-query GQA attention over a kv8 cache: the structure of decode.hip's attn_decode_kernel in its 4-wave form without the fused prologue — grid
// (nsplit, nkv, B), wave w takes the 32-position blocks w, w + 4, ... of the split's chunk, the same A-row -> position map (so a lane's eight scores are
// eight consecutive positions and P never leaves registers), unconditional block loads with the steady iterations and the last block apart, write-through
// partials, ticket merge, re-zeroed tickets.  Per block a lane loads 2 x 2 x 16 B of K8, 8 x 8 B of V8 and its 8 ks and 8 vs values:
//   score_j = (acc_j * scale) * ks[j]      acc = fp32 MFMA sum of q . widen(K8[j])
//   p_j     = exp(score_j - m);  l += p_j  (the unscaled p)
//   P_j     = round16(p_j * vs[j])         operand of the PV MFMA against widen(V8)
// q [B][ldq] holds the rotated q heads; the newest position is already in the cache.  Positions past pos[b] inside a block are read and weigh exactly 0:
// they must hold finite bytes and finite scales (the arrays are zero-filled at creation and only ever hold finite values).
constexpr int NW = 4;
__global__ __launch_bounds__(NW * 64, 3) void attn_decode_kv8_kernel(const bf16_t* __restrict__ q, int ldq, const uint8_t* __restrict__ k8,
                                                                     const uint8_t* __restrict__ v8, const float* __restrict__ ksc,
                                                                     const float* __restrict__ vsc, long slot_stride, long kv_head_stride,
                                                                     const int32_t* __restrict__ slots, const int32_t* __restrict__ pos,
                                                                     float* __restrict__ ws, unsigned int* __restrict__ tickets, bf16_t* __restrict__ O,
                                                                     int ldo, int nq, int nkv, int nsplit, float scale) {
    constexpr int GQ = 4;
    __shared__ __attribute__((aligned(16))) float s_acc[NW][GQ][HD];
    __shared__ float s_m[NW][GQ], s_l[NW][GQ];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i = lane & 15, g = lane >> 4;          // i: A-row / head column; g: k-group
    const int sp = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
    const int ctx = pos[b] + 1;
    int chunk = (ctx + nsplit - 1) / nsplit;
    chunk = (chunk + 31) & ~31;
    const int beg = sp * chunk, end = min(ctx, beg + chunk);
    const int len = max(end - beg, 0);
    const int nit = (len + 31) >> 5;                  // 32-position blocks in this split
    const size_t base = (size_t)slots[b] * slot_stride + (size_t)kvh * kv_head_stride;
    const uint8_t* kb = k8 + base;
    const uint8_t* vb = v8 + base;
    const float* ksb = ksc + base / HD;
    const float* vsb = vsc + base / HD;

    const int prow = (i >> 2) * 8 + (i & 3);          // + 4 t: position (within the block) of A-row i of S tile t
    u32x4_t kr[2][2];                                 // tile t, half h: d = h*64 + g*16 .. +16 of the row
    u32x2_t vr[8];                                    // d = dt*16 + i, positions g*8 .. +8 of the block
    f32x4_t ksr[2], vsr[2];                           // the scales of positions g*8 .. +8
    // unconditional loads: a block's 32 positions lie below round_up(end, 32) <= ctx_pad, inside the slot's rows
    auto load_k = [&](int it) {
        const int P0 = beg + it * 32;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint8_t* src = kb + (size_t)(P0 + prow + 4 * t) * HD + g * 16;
            kr[t][0] = *reinterpret_cast<const u32x4_t*>(src);
            kr[t][1] = *reinterpret_cast<const u32x4_t*>(src + 64);
        }
        ksr[0] = *reinterpret_cast<const f32x4_t*>(ksb + P0 + g * 8);
        ksr[1] = *reinterpret_cast<const f32x4_t*>(ksb + P0 + g * 8 + 4);
    };
    auto load_v = [&](int it) {
        const int P0 = beg + it * 32;
        const uint8_t* vsrc = vb + ((size_t)(P0 >> 5) * HD + i) * 32 + g * 8;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) vr[dt] = *reinterpret_cast<const u32x2_t*>(vsrc + dt * 16 * 32);
        vsr[0] = *reinterpret_cast<const f32x4_t*>(vsb + P0 + g * 8);
        vsr[1] = *reinterpret_cast<const f32x4_t*>(vsb + P0 + g * 8 + 4);
    };
    if (wid < nit) { load_k(wid); load_v(wid); }      // cache blocks start streaming before anything else

    u32x4_t qf[4];                                    // B operand of S: q of head i (i < 4), zero columns otherwise
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
        qf[s4] = i < GQ ? *reinterpret_cast<const u32x4_t*>(q + (size_t)b * ldq + (kvh * GQ + i) * HD + (s4 >> 1) * 64 + g * 16 + (s4 & 1) * 8)
                        : u32x4_t{0u, 0u, 0u, 0u};

    float m = -1e30f, l = 0.f;                        // running max (per head = per column i) and this lane's partial sum
    f32x4_t acc[8];                                   // O^T tile dt: lane (i, g) reg r  <->  d = dt*16 + g*4 + r, head i
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) acc[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // one register set, refilled as soon as what read it has issued; a steady part whose every iteration requests the next block without a condition, and the
    // wave's last block, which requests nothing (so the wait in front of the QK products covers the K block only: see attn_decode_kernel)
    auto block = [&](const int it, auto prefetch) {
        const int P0 = beg + it * 32;
        f32x4_t S[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            S[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
                S[t] = mfma16(widen8(kr[t][s4 >> 1][2 * (s4 & 1)], kr[t][s4 >> 1][2 * (s4 & 1) + 1]), __builtin_bit_cast(bf16x8_t, qf[s4]), S[t]);
        }
        // lane (head i, group g): S[t][r] is the score of position P0 + g*8 + t*4 + r
        float sv[8];
        float mx = -1e30f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool ok = P0 + g * 8 + e < end;
            sv[e] = ok ? (S[e >> 2][e & 3] * scale) * ksr[e >> 2][e & 3] : -1e30f;
            mx = fmaxf(mx, sv[e]);
        }
        if constexpr (decltype(prefetch)::value) {
            load_k(it + NW);
            // left alone the scheduler sinks these requests to the end of the iteration, beside the V8 ones, and the next block's K streams under nothing:
            // pinned here it streams under this block's softmax and PV products
            __builtin_amdgcn_sched_barrier(0);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m, mx);
        const float a = __expf(m - mn);
        m = mn;
        float p[8], pv[8], ps = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool ok = P0 + g * 8 + e < end;
            p[e] = ok ? __expf(sv[e] - mn) : 0.f;
            pv[e] = ok ? p[e] * vsr[e >> 2][e & 3] : 0.f;
            ps += p[e];
        }
        l = l * a + ps;
        const u32x4_t pf = {pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3]), pack2bf(pv[4], pv[5]), pack2bf(pv[6], pv[7])};
        if constexpr (!decltype(prefetch)::value) {
            // only a wave's last block can reach past `end`: 8-position groups wholly past it count as zeros
            const bool vok = P0 + g * 8 < end;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) vr[dt] = vok ? vr[dt] : u32x2_t{0u, 0u};
        }
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            acc[dt] *= a;
            acc[dt] = mfma16(widen8(vr[dt][0], vr[dt][1]), __builtin_bit_cast(bf16x8_t, pf), acc[dt]);
        }
        if constexpr (decltype(prefetch)::value) load_v(it + NW);
    };
    // the first blocks and the q slices are waited for here, so that the loop header's wait does not have to cover them (vmcnt(0); expcnt / lgkmcnt untouched)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    {
        int it = wid;
        for (; it + NW < nit; it += NW) block(it, std::true_type{});
        if (it < nit) block(it, std::false_type{});
    }
    // ---- the k-groups of a wave share m; sum their l; then merge the 4 waves through LDS ----
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (i < GQ) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt)
            *reinterpret_cast<f32x4_t*>(&s_acc[wid][i][dt * 16 + g * 4]) = acc[dt];
        if (g == 0) { s_m[wid][i] = m; s_l[wid][i] = l; }
    }
    __syncthreads();
    {
        const size_t wbase = (((size_t)b * nq + kvh * GQ) * nsplit + sp) * (HD + 2);
        // write-through (sc1) stores: visible at agent scope once vmcnt drains, no L2 write-back fence needed
        for (int x = tid; x < GQ * HD; x += NW * 64) {
            const int hq = x >> 7, d = x & 127;
            float M = s_m[0][hq];
#pragma unroll
            for (int w = 1; w < NW; ++w) M = fmaxf(M, s_m[w][hq]);
            float o = 0.f, L = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const float f = __expf(s_m[w][hq] - M);
                o += f * s_acc[w][hq][d];
                L += f * s_l[w][hq];
            }
            if (nsplit == 1) {                        // nothing to merge across workgroups: finish here
                O[(size_t)b * ldo + (kvh * GQ + hq) * HD + d] = f2bf(o / L);
                continue;
            }
            __hip_atomic_store(&ws[wbase + (size_t)hq * nsplit * (HD + 2) + d], o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (d == 0) {
                __hip_atomic_store(&ws[wbase + (size_t)hq * nsplit * (HD + 2) + HD], M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&ws[wbase + (size_t)hq * nsplit * (HD + 2) + HD + 1], L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (nsplit == 1) return;
    // ---- publish + ticket; the last arriver of this (b, kv-head) merges the splits ----
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(&tickets[b * nkv + kvh], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = (t == (unsigned)(nsplit - 1));
        if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    for (int hq = wid; hq < GQ; hq += NW) {   // wave w merges q-head w: lane owns d = 2*lane, 2*lane+1; split loads are independent -> issued in batches
        const float* w = ws + (((size_t)b * nq + kvh * GQ + hq) * nsplit) * (HD + 2);
        float M = -1e30f;
        for (int s2 = lane; s2 < nsplit; s2 += 64) M = fmaxf(M, w[s2 * (HD + 2) + HD]);
        M = wave_max(M);
        float num0 = 0.f, num1 = 0.f, den = 0.f;
        for (int s0 = 0; s0 < nsplit; s0 += 8) {
            float2 o[8];
            float mm[8], ll[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int s2 = min(s0 + u, nsplit - 1);
                const float* ws2 = w + (size_t)s2 * (HD + 2);
                o[u] = *reinterpret_cast<const float2*>(ws2 + 2 * lane);
                mm[u] = ws2[HD];
                ll[u] = ws2[HD + 1];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (s0 + u < nsplit) {
                    const float f = __expf(mm[u] - M);
                    num0 += f * o[u].x; num1 += f * o[u].y; den += f * ll[u];
                }
            }
        }
        const float inv = 1.f / den;
        *reinterpret_cast<uint32_t*>(O + (size_t)b * ldo + (kvh * GQ + hq) * HD + 2 * lane) = pack2bf(num0 * inv, num1 * inv);
    }
    if (tid == 0) __hip_atomic_store(&tickets[b * nkv + kvh], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------
// qkv_finish_kernel (decode.hip) for a kv8 cache: the same sums in chunk order, the same rounding to the element type, the same RoPE; q goes to qout,
// the new k row and v column are quantised by the row rule (amax over the 128 rounded values, reduced over the 8 lanes of the head) and stored with
// their scales at pos[b] of slots[b] — 128 + 128 bytes and two floats per (sequence, kv head), nothing else.
__global__ __launch_bounds__(256) void qkv_finish_kv8_kernel(const float* __restrict__ part, int ks, int ldq, bf16_t* __restrict__ qout,
                                                             uint8_t* __restrict__ k8, uint8_t* __restrict__ v8, float* __restrict__ ksc,
                                                             float* __restrict__ vsc, long slot_stride, long kv_head_stride,
                                                             const int32_t* __restrict__ slots, const int32_t* __restrict__ pos, int B, int nq, int nkv,
                                                             const float* __restrict__ cos_t, const float* __restrict__ sin_t) {
    constexpr int HALF = 64;
    const int nh = nq + 2 * nkv;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * nh * 8) return;                       // whole groups of 8 lanes leave together
    const int c = idx & 7, hh = (idx >> 3) % nh, b = (idx >> 3) / nh;
    const int p_new = pos[b];
    const float* pp = part + (size_t)b * ldq + (size_t)hh * HD + c * 8;
    f32x4_t x[4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};     // d..d+3, d+4..d+7, d+64.., d+68..
    for (int k = 0; k < ks; ++k) {
        const float* pk = pp + (size_t)k * SK_ROWS * ldq;
        x[0] += *reinterpret_cast<const f32x4_t*>(pk);
        x[1] += *reinterpret_cast<const f32x4_t*>(pk + 4);
        x[2] += *reinterpret_cast<const f32x4_t*>(pk + HALF);
        x[3] += *reinterpret_cast<const f32x4_t*>(pk + HALF + 4);
    }
    uint32_t lo[4] = {pack2bf(x[0][0], x[0][1]), pack2bf(x[0][2], x[0][3]), pack2bf(x[1][0], x[1][1]), pack2bf(x[1][2], x[1][3])};
    uint32_t hi[4] = {pack2bf(x[2][0], x[2][1]), pack2bf(x[2][2], x[2][3]), pack2bf(x[3][0], x[3][1]), pack2bf(x[3][2], x[3][3])};
    const bool is_v = hh >= nq + nkv;
    if (!is_v) {
        const float4* cp = reinterpret_cast<const float4*>(cos_t + (size_t)p_new * HALF + c * 8);
        const float4* sq = reinterpret_cast<const float4*>(sin_t + (size_t)p_new * HALF + c * 8);
        const float4 c0 = cp[0], c1 = cp[1], s0 = sq[0], s1 = sq[1];
        const float cs[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x1l = bflo(lo[e]), x1h = bfhi(lo[e]), x2l = bflo(hi[e]), x2h = bfhi(hi[e]);
            lo[e] = pack2bf(x1l * cs[2 * e] - x2l * sn[2 * e], x1h * cs[2 * e + 1] - x2h * sn[2 * e + 1]);
            hi[e] = pack2bf(x2l * cs[2 * e] + x1l * sn[2 * e], x2h * cs[2 * e + 1] + x1h * sn[2 * e + 1]);
        }
    }
    if (hh < nq) {
        bf16_t* dst = qout + (size_t)b * ldq + (size_t)hh * HD;
        *reinterpret_cast<uint4*>(dst + c * 8) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        *reinterpret_cast<uint4*>(dst + HALF + c * 8) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
        return;                                          // a head's 8 lanes leave together: the shuffles below stay inside whole groups
    }
    float f[16];
    unpack_pairs(lo, f);
    unpack_pairs(hi, f + 8);
    uint32_t qb[4];
    const float sc = quant16_of_row(f, qb);
    const size_t base = (size_t)slots[b] * slot_stride + (size_t)(is_v ? hh - nq - nkv : hh - nq) * kv_head_stride;
    if (!is_v) {
        uint8_t* dst = k8 + base + (size_t)p_new * HD;
        *reinterpret_cast<uint2*>(dst + c * 8) = make_uint2(qb[0], qb[1]);
        *reinterpret_cast<uint2*>(dst + HALF + c * 8) = make_uint2(qb[2], qb[3]);
        if (c == 0) ksc[base / HD + p_new] = sc;
        return;
    }
    uint8_t* dst = v8 + base + (size_t)(p_new >> 5) * (HD * 32) + (p_new & 31);       // byte (d, p % 32) of block p / 32
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        dst[(size_t)(c * 8 + e) * 32] = (uint8_t)(qb[e >> 2] >> (8 * (e & 3)));
        dst[(size_t)(HALF + c * 8 + e) * 32] = (uint8_t)(qb[2 + (e >> 2)] >> (8 * (e & 3)));
    }
    if (c == 0) vsc[base / HD + p_new] = sc;
}

// ---------------------------------------------------------------------------------------------------------
// 16-bit rows -> kv8: positions [pos0, pos0 + R) of slot slots[b] from row r = position - pos0 of K (roped) and V, both ROW-major: element d of row r
// of (b, kv head) at src + b * bs + kvh * hs + r * rs + d.  Grid (32-position blocks of the DESTINATION that the rows touch, nkv, B); 8 lanes per
// position (lane c: d = 16c .. 16c + 15), so amax is a contiguous 128-wide reduction for V as well; the V tile goes through LDS to the blocked layout.
// Only the bytes and scales of the R positions are written.
__global__ __launch_bounds__(256) void kv8_pack_kernel(const bf16_t* __restrict__ K, long k_bs, long k_hs, long k_rs, const bf16_t* __restrict__ V,
                                                       long v_bs, long v_hs, long v_rs, uint8_t* __restrict__ k8, uint8_t* __restrict__ v8,
                                                       float* __restrict__ ksc, float* __restrict__ vsc, long slot_stride, long kv_head_stride,
                                                       const int32_t* __restrict__ slots, int pos0, int R) {
    __shared__ __attribute__((aligned(16))) uint8_t s_v[HD][32 + 16];            // [d][position in the block]; rows 48 B apart (16-byte aligned)
    const int tid = threadIdx.x, c = tid & 7, pp = tid >> 3;
    const int kvh = blockIdx.y, b = blockIdx.z;
    const int blk = (pos0 >> 5) + blockIdx.x, p = blk * 32 + pp;
    const bool on = p >= pos0 && p < pos0 + R;
    const size_t base = (size_t)slots[b] * slot_stride + (size_t)kvh * kv_head_stride;
    const int r = on ? p - pos0 : 0;
    uint32_t u[2][8];
    {
        const bf16_t* ksrc = K + (size_t)b * k_bs + (size_t)kvh * k_hs + (size_t)r * k_rs + c * 16;
        const bf16_t* vsrc = V + (size_t)b * v_bs + (size_t)kvh * v_hs + (size_t)r * v_rs + c * 16;
        const uint4 k0 = *reinterpret_cast<const uint4*>(ksrc), k1 = *reinterpret_cast<const uint4*>(ksrc + 8);
        const uint4 v0 = *reinterpret_cast<const uint4*>(vsrc), v1 = *reinterpret_cast<const uint4*>(vsrc + 8);
        const uint32_t kk[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w}, vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) { u[0][e] = kk[e]; u[1][e] = vv[e]; }
    }
    uint32_t qk[4], qv[4];
    float f[16];
#pragma unroll
    for (int e = 0; e < 8; ++e) { f[2 * e] = bflo(u[0][e]); f[2 * e + 1] = bfhi(u[0][e]); }
    const float sk = quant16_of_row(f, qk);
#pragma unroll
    for (int e = 0; e < 8; ++e) { f[2 * e] = bflo(u[1][e]); f[2 * e + 1] = bfhi(u[1][e]); }
    const float sv = quant16_of_row(f, qv);
    if (on) {
        *reinterpret_cast<uint4*>(k8 + base + (size_t)p * HD + c * 16) = make_uint4(qk[0], qk[1], qk[2], qk[3]);
        if (c == 0) { ksc[base / HD + p] = sk; vsc[base / HD + p] = sv; }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) s_v[c * 16 + e][pp] = (uint8_t)(qv[e >> 2] >> (8 * (e & 3)));
    __syncthreads();
    // thread -> (d = tid / 2, 16 positions): a whole 16-byte piece when all its positions belong to the rows, single bytes at the two ends
    const int d = tid >> 1, h0 = (tid & 1) * 16;
    const int lo = max(pos0 - blk * 32, 0), hi = min(pos0 + R - blk * 32, 32);     // the block's positions [lo, hi) belong to the rows
    uint8_t* dst = v8 + base + ((size_t)blk * HD + d) * 32 + h0;
    if (lo <= h0 && h0 + 16 <= hi) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&s_v[d][h0]);
    } else {
        for (int e = max(lo - h0, 0); e < min(hi - h0, 16); ++e) dst[e] = s_v[d][h0 + e];
    }
}

// kv8 -> 16-bit: rows [0, R) of slot slots[b] as round16(scale * e4m3) into row b of a K / V^T pair in the 16-bit cache's layout (K [.][kvh][pos][128],
// V^T [.][kvh][128][ctx_stride]; dst_bs / dst_hs: batch and kv-head strides of both, in elements).  Grid (ceil(R / 32), nkv, B).
__global__ __launch_bounds__(256) void kv8_unpack_kernel(const uint8_t* __restrict__ k8, const uint8_t* __restrict__ v8, const float* __restrict__ ksc,
                                                         const float* __restrict__ vsc, long slot_stride, long kv_head_stride,
                                                         const int32_t* __restrict__ slots, bf16_t* __restrict__ K, bf16_t* __restrict__ Vt, long dst_bs,
                                                         long dst_hs, int ctx_stride, int R) {
    const int tid = threadIdx.x;
    const int kvh = blockIdx.y, b = blockIdx.z, blk = blockIdx.x;
    const size_t base = (size_t)slots[b] * slot_stride + (size_t)kvh * kv_head_stride;
    const size_t dbase = (size_t)b * dst_bs + (size_t)kvh * dst_hs;
    {   // K: 8 lanes per position, lane c: d = 16c .. 16c + 15
        const int c = tid & 7, p = blk * 32 + (tid >> 3);
        if (p < R) {
            const uint4 w = *reinterpret_cast<const uint4*>(k8 + base + (size_t)p * HD + c * 16);
            const float s = ksc[base / HD + p];
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
            uint32_t o[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f[4];
                f32_of_fp8x4(ww[j], f);
                o[2 * j] = pack2bf(s * f[0], s * f[1]);
                o[2 * j + 1] = pack2bf(s * f[2], s * f[3]);
            }
            bf16_t* dst = K + dbase + (size_t)p * HD + c * 16;
            *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<uint4*>(dst + 8) = make_uint4(o[4], o[5], o[6], o[7]);
        }
    }
    {   // V^T: thread -> (d = tid / 2, 16 positions of the block)
        const int d = tid >> 1, p0 = blk * 32 + (tid & 1) * 16;
        if (p0 < R) {
            const uint4 w = *reinterpret_cast<const uint4*>(v8 + base + ((size_t)blk * HD + d) * 32 + (tid & 1) * 16);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
            const float* sp = vsc + base / HD + p0;
            bf16_t* dst = Vt + dbase + (size_t)d * ctx_stride + p0;
            uint32_t o[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f[4];
                f32_of_fp8x4(ww[j], f);
                const f32x4_t s = *reinterpret_cast<const f32x4_t*>(sp + 4 * j);
                o[2 * j] = pack2bf(s[0] * f[0], s[1] * f[1]);
                o[2 * j + 1] = pack2bf(s[2] * f[2], s[3] * f[3]);
            }
            if (p0 + 16 <= R) {
                *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<uint4*>(dst + 8) = make_uint4(o[4], o[5], o[6], o[7]);
            } else {
                for (int e = 0; e < R - p0; ++e) dst[e] = (bf16_t)(o[e >> 1] >> (16 * (e & 1)));
            }
        }
    }
}

// positions [0, n32) (a multiple of 32) of one slot to dst.n others, all four arrays of every (layer, kv head): grid (chunks, layers * kv heads, dst.n),
// 16-byte pieces; per (layer, kv head) K8 and V8 are n32 * 128 contiguous bytes each, ks and vs n32 floats
__global__ __launch_bounds__(256) void kv8_copy_kernel(uint8_t* __restrict__ k8, uint8_t* __restrict__ v8, float* __restrict__ ksc, float* __restrict__ vsc,
                                                       long layer_stride, long slot_stride, long kv_head_stride, int kv_heads, int src, KvCopyDst dst,
                                                       int n32) {
    const int layer = blockIdx.y / kv_heads, kvh = blockIdx.y % kv_heads, to = dst.slot[blockIdx.z];
    const size_t head = (size_t)layer * layer_stride + (size_t)kvh * kv_head_stride;
    const size_t from_b = head + (size_t)src * slot_stride, to_b = head + (size_t)to * slot_stride;
    const int np = n32 * 8, ns = n32 / 4;                // 16-byte pieces of a payload array / of a scale array
    for (int u = blockIdx.x * 256 + threadIdx.x; u < 2 * np + 2 * ns; u += gridDim.x * 256) {
        if (u < np) *reinterpret_cast<uint4*>(k8 + to_b + (size_t)u * 16) = *reinterpret_cast<const uint4*>(k8 + from_b + (size_t)u * 16);
        else if (u < 2 * np) *reinterpret_cast<uint4*>(v8 + to_b + (size_t)(u - np) * 16) = *reinterpret_cast<const uint4*>(v8 + from_b + (size_t)(u - np) * 16);
        else if (u < 2 * np + ns) *reinterpret_cast<uint4*>(ksc + to_b / HD + (size_t)(u - 2 * np) * 4) = *reinterpret_cast<const uint4*>(ksc + from_b / HD + (size_t)(u - 2 * np) * 4);
        else *reinterpret_cast<uint4*>(vsc + to_b / HD + (size_t)(u - 2 * np - ns) * 4) = *reinterpret_cast<const uint4*>(vsc + from_b / HD + (size_t)(u - 2 * np - ns) * 4);
    }
}
}  // namespace

static bool kv8_strides_ok(const Kv8Cache& c) {
    return c.k8 && c.v8 && c.ks && c.vs && c.ctx_pad >= 32 && c.ctx_pad % 32 == 0 && c.kv_head_stride == (long)c.ctx_pad * HD && c.slot_stride > 0 &&
           c.slot_stride % c.kv_head_stride == 0;
}

int launch_attn_decode_kv8(const bf16_t* q, int ldq, const Kv8Cache& c, const int32_t* slots, const int32_t* pos, bf16_t* O, int ldo, float* ws,
                           unsigned int* tickets, int B, int nq, int nkv, int hd, int nsplit, float scale, hipStream_t s) {
    if (hd != HD || nq != 4 * nkv || nsplit < 1 || B < 1 || !tickets || !kv8_strides_ok(c) || (ldq % 8) || (nsplit > 1 && !ws)) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(attn_decode_kv8_kernel, dim3(nsplit, nkv, B), dim3(NW * 64), 0, s, q, ldq, c.k8, c.v8, c.ks, c.vs, c.slot_stride, c.kv_head_stride,
                       slots, pos, ws, tickets, O, ldo, nq, nkv, nsplit, scale);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_qkv_finish_kv8(const float* part, int ks, int ldq, bf16_t* qout, const Kv8Cache& c, const int32_t* slots, const int32_t* pos, int B, int nq,
                          int nkv, const float* cos_t, const float* sin_t, hipStream_t s) {
    if (B < 1 || ks < 1 || (ldq % 8) || !kv8_strides_ok(c)) return TRACE_ERR_ARG;
    const int total = B * (nq + 2 * nkv) * 8;
    hipLaunchKernelGGL(qkv_finish_kv8_kernel, dim3((total + 255) / 256), dim3(256), 0, s, part, ks, ldq, qout, c.k8, c.v8, c.ks, c.vs, c.slot_stride,
                       c.kv_head_stride, slots, pos, B, nq, nkv, cos_t, sin_t);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_kv8_pack(const bf16_t* K, long k_bs, long k_hs, long k_rs, const bf16_t* V, long v_bs, long v_hs, long v_rs, const Kv8Cache& c,
                    const int32_t* slots, int pos0, int R, int B, int nkv, hipStream_t s) {
    if (B < 1 || nkv < 1 || R < 1 || pos0 < 0 || pos0 + R > c.ctx_pad || !kv8_strides_ok(c) || !K || !V) return TRACE_ERR_ARG;
    if ((k_bs | k_hs | k_rs | v_bs | v_hs | v_rs) % 8) return TRACE_ERR_ARG;           // 16-byte loads
    const int nblk = ((pos0 + R - 1) >> 5) - (pos0 >> 5) + 1;
    hipLaunchKernelGGL(kv8_pack_kernel, dim3(nblk, nkv, B), dim3(256), 0, s, K, k_bs, k_hs, k_rs, V, v_bs, v_hs, v_rs, c.k8, c.v8, c.ks, c.vs, c.slot_stride,
                       c.kv_head_stride, slots, pos0, R);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_kv8_unpack(const Kv8Cache& c, const int32_t* slots, bf16_t* K, bf16_t* Vt, long dst_bs, long dst_hs, int ctx_stride, int R, int B, int nkv,
                      hipStream_t s) {
    if (B < 1 || nkv < 1 || R < 1 || R > c.ctx_pad || R > ctx_stride || !kv8_strides_ok(c) || !K || !Vt || (ctx_stride % 8) || (dst_bs % 8) || (dst_hs % 8))
        return TRACE_ERR_ARG;
    hipLaunchKernelGGL(kv8_unpack_kernel, dim3((R + 31) / 32, nkv, B), dim3(256), 0, s, c.k8, c.v8, c.ks, c.vs, c.slot_stride, c.kv_head_stride, slots, K, Vt,
                       dst_bs, dst_hs, ctx_stride, R);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_kv8_copy(const Kv8Cache& c, long layer_stride, int layers, int kv_heads, int src, const KvCopyDst& dst, int rows, hipStream_t s) {
    if (!kv8_strides_ok(c) || layers < 1 || kv_heads < 1 || dst.n < 1 || dst.n > KV_COPY_MAX || rows < 1 || rows > c.ctx_pad || layer_stride % c.slot_stride)
        return TRACE_ERR_ARG;
    const int n32 = (rows + 31) / 32 * 32;
    const int units = 2 * n32 * 8 + 2 * (n32 / 4);
    hipLaunchKernelGGL(kv8_copy_kernel, dim3(std::min((units + 255) / 256, 64), layers * kv_heads, dst.n), dim3(256), 0, s, c.k8, c.v8, c.ks, c.vs, layer_stride,
                       c.slot_stride, c.kv_head_stride, kv_heads, src, dst, n32);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
