// w4 weight path of the Mistral decoder: the four projections of every layer as OCP e2m1 codes with one power-of-two scale (an e8m0 byte) per 32
// consecutive k of an output row — the format include/trace_hip.h states at its end and trace_amd/w4.py restates in torch.  The effective weight
// W~[n][k] = e2m1(code) * 2^e is exactly a bf16 value, so the prefill (dequant_w4 into a row-major scratch, then the bf16 GEMMs) and the decode GEMV
// (codes widened to bf16 in registers by v_cvt_scalef32_pk_bf16_fp4 with the block's scale, bf16 MFMA) multiply by the same matrix, and a bf16 engine
// loaded with W~ is the exact reference of both.  bf16 library only: the element bits are read as bf16 here, whatever the build's element type.
// This file: row quantiser, the decode tile layout and its inverse (the dequantiser), and the decode GEMV, which has the structure of fp8.hip's
// weight-only kernel with 256-k units: a lane's 32 contiguous weight bytes are EIGHT 8-k fragments in two scale blocks.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// exponent byte of a block from the largest bf16 magnitude bits in it (positive floats order as their bits): the smallest e with amax <= 6 * 2^e =
// 1.5 * 2^(e + 2), i.e. E - 2 for a mantissa <= 1.5 and E - 1 above, kept >= -120 so that 2^-e and every quotient below stay normal fp32 numbers
// (a bf16 denormal then rounds to code 0 whether or not the hardware flushes it).  An all-zero block: byte 0.
__device__ __forceinline__ int w4_exp_byte(unsigned int amax_bits) {
    if (amax_bits == 0) return 0;
    const int e = (int)(amax_bits >> 7) - 127 - 2 + ((amax_bits & 0x7f) > 0x40 ? 1 : 0);
    return max(e, -120) + 127;
}
// e2m1 code of bf16 bits v under the scale 2^(eb - 127): round to nearest, ties to the even code, on |v| / 2^e (exact: a power-of-two quotient);
// the sign bit is set only beside a non-zero magnitude
__device__ __forceinline__ unsigned int w4_code(unsigned int v, int eb) {
    const float a = __uint_as_float((v & 0x7fffu) << 16) * __uint_as_float((unsigned int)(254 - eb) << 23);
    const unsigned int m = a <= 0.25f ? 0u : a < 0.75f ? 1u : a <= 1.25f ? 2u : a < 1.75f ? 3u : a <= 2.5f ? 4u : a < 3.5f ? 5u : a <= 5.0f ? 6u : 7u;
    return m ? m | ((v >> 12) & 8u) : 0u;
}

// W [N][K] bf16 -> codes [N][K/2] (k = 2j in the low nibble of byte j, k = 2j + 1 in the high one) + exps [N][K/32].  One thread per 32-k block.
__global__ __launch_bounds__(256) void quant_rows_w4_kernel(const bf16_t* __restrict__ W, long ldw, uint8_t* __restrict__ codes, uint8_t* __restrict__ exps,
                                                            int N, int K) {
    const int KB = K >> 5;
    const long total = (long)N * KB;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const int n = (int)(p / KB), kb = (int)(p - (long)n * KB);
        const uint4* src = reinterpret_cast<const uint4*>(W + (size_t)n * ldw + (size_t)kb * 32);
        uint32_t w[16];
        unsigned int amax = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = src[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) amax = max(amax, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
        const int eb = w4_exp_byte(amax);
        uint32_t q[4] = {0, 0, 0, 0};
        if (eb) {
#pragma unroll
            for (int i = 0; i < 16; ++i) q[i >> 2] |= (w4_code(w[i] & 0xffffu, eb) | w4_code(w[i] >> 16, eb) << 4) << (8 * (i & 3));
        }
        *reinterpret_cast<uint4*>(codes + (size_t)n * (K >> 1) + (size_t)kb * 16) = make_uint4(q[0], q[1], q[2], q[3]);
        exps[(size_t)n * KB + kb] = (uint8_t)eb;
    }
}

// Logical codes / exps -> the decode copy.  Source row n goes to tile tile0 + (n / 16) * tile_step, row n % 16; block kb of it to unit kb / 8,
// lane g * 16 + r with g = (kb % 8) / 2, half h = kb % 2: 16 code bytes at (tile, unit, lane) * 32 + h * 16 and the exponent byte at (tile, unit, lane) * 2 + h.
// The nibble order inside a byte is the logical one (the conversion instruction takes the low nibble to the low half: tests/test_gpu_w4.py pointer probe).
__global__ __launch_bounds__(256) void tile_pack_w4_kernel(const uint8_t* __restrict__ codes, const uint8_t* __restrict__ exps, uint8_t* __restrict__ tc,
                                                           uint8_t* __restrict__ te, int N, int K, int tile0, int tile_step) {
    const int KB = K >> 5, U = K >> 8;
    const long total = (long)N * KB;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const int n = (int)(p / KB), kb = (int)(p - (long)n * KB);
        const int tile = tile0 + (n >> 4) * tile_step, r = n & 15, u = kb >> 3, g = (kb & 7) >> 1, h = kb & 1;
        const size_t slot = ((size_t)tile * U + u) * 64 + g * 16 + r;
        *reinterpret_cast<u32x4_t*>(tc + slot * 32 + h * 16) = *reinterpret_cast<const u32x4_t*>(codes + (size_t)n * (K >> 1) + (size_t)kb * 16);
        te[slot * 2 + h] = exps[(size_t)n * KB + kb];
    }
}

// value of a code under exponent byte eb as bf16 bits: {0, .5, 1, 1.5, 2, 3, 4, 6} * 2^(eb - 127), exact (one mantissa bit, exponent in range); byte 0
// (all-zero block) and code 0 give 0
__device__ __forceinline__ uint32_t w4_value_bits(unsigned int c, int eb) {
    const unsigned int m = c & 7u;
    if (!m || !eb) return 0;
    const float base = m == 1 ? 0.5f : m == 2 ? 1.0f : m == 3 ? 1.5f : m == 4 ? 2.0f : m == 5 ? 3.0f : m == 6 ? 4.0f : 6.0f;
    const float v = base * __uint_as_float((unsigned int)eb << 23);
    return (__float_as_uint(v) >> 16) | ((c & 8u) << 12);
}
// the decode copy -> row-major bf16 [N][ldo].  One thread per 32-k block (the inverse walk of tile_pack_w4).
__global__ __launch_bounds__(256) void dequant_w4_kernel(const uint8_t* __restrict__ tc, const uint8_t* __restrict__ te, bf16_t* __restrict__ out, long ldo,
                                                         int N, int K) {
    const int KB = K >> 5, U = K >> 8;
    const long total = (long)N * KB;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const int n = (int)(p / KB), kb = (int)(p - (long)n * KB);
        const int tile = n >> 4, r = n & 15, u = kb >> 3, g = (kb & 7) >> 1, h = kb & 1;
        const size_t slot = ((size_t)tile * U + u) * 64 + g * 16 + r;
        const u32x4_t c = *reinterpret_cast<const u32x4_t*>(tc + slot * 32 + h * 16);
        const int eb = te[slot * 2 + h];
        uint4* dst = reinterpret_cast<uint4*>(out + (size_t)n * ldo + (size_t)kb * 32);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t d = c[i];
            uint32_t o[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned int by = (d >> (8 * b)) & 0xffu;
                o[b] = w4_value_bits(by & 15u, eb) | w4_value_bits(by >> 4, eb) << 16;
            }
            dst[i] = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
}

__device__ __forceinline__ uint4 ldg_nt16(const uint8_t* p) {
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    return make_uint4(v[0], v[1], v[2], v[3]);
}
// eight codes (one dword = one 8-k MFMA fragment) -> bf16 under the block's scale: four conversions, one per byte
__device__ __forceinline__ bf16x8_t widen8_w4(unsigned int d, float scale) {
    union { bf16x8_t v; bf16x2_t p[4]; } u;
    u.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 0);
    u.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 1);
    u.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 2);
    u.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, scale, 3);
    return u.v;
}
// 2^(eb - 127) as the conversion's scale operand; byte 0 (all codes zero) takes 2^-126, a normal number, so the product is a plain zero
__device__ __forceinline__ float w4_scale(unsigned int eb) { return __uint_as_float(max(eb, 1u) << 23); }

// Decode GEMV on w4 weights: fp8.hip's weight-only kernel with 256-k units.  Lane (r, g) of (tile, unit) holds the 64 codes of row tile*16 + r,
// k = unit*256 + g*64 .. +64: dword q (0..7) of its 32 bytes is MFMA fragment q, dwords 0-3 under the lane's first exponent byte, 4-7 under its second.
// A unit parks EIGHT 1 KB activation images per row group: image q, lane (r, g) = X[16 nb + r][unit*256 + g*64 + q*8 .. +8].  No scale multiply in the
// epilogue: the scales are inside the widened weights.  partial[ks][m][n] = sum over the chunk of X[m][k] W~[n][k].
template <int NB, int NT>
__global__ __launch_bounds__(512) void skinny_w4_kernel(const bf16_t* __restrict__ X, long ldx, const uint8_t* __restrict__ W, const uint8_t* __restrict__ E,
                                                        int B, int K, int chunk_units, int KS, int T, int WPT, int ntiles, float* __restrict__ ws, int N) {
    constexpr int UN = 2;                                // 256-k units per load batch: 4 KB (NT = 1) / 8 KB (NT = 2) of codes per wave
    constexpr int NF = NT * NB;
    constexpr int IPU = 8;                               // 1 KB activation images per unit and row group
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u32x4_t* xs = reinterpret_cast<u32x4_t*>(smem);                                           // [unit][fragment][nb][lane]
    f32x4_t* red = reinterpret_cast<f32x4_t*>(smem + (size_t)chunk_units * IPU * NB * 1024);   // [task][wsub][NF][lane]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nwaves = blockDim.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int ks = blockIdx.x % KS, rg = blockIdx.x / KS;
    const int U = K >> 8;
    const int u_beg = ks * chunk_units, nu = min(U - u_beg, chunk_units);
    const int team = wid / WPT, wsub = wid - team * WPT, nteams = nwaves / WPT;
    const int ua = (wsub * nu) / WPT, ub = ((wsub + 1) * nu) / WPT;
    const uint8_t* wp[NT];
    const uint8_t* ep[NT];
    uint4 wa[UN][NT][2], wb[UN][NT][2];
    unsigned int ea[UN][NT], eb[UN][NT];
    auto loadw = [&](uint4 (&wf)[UN][NT][2], unsigned int (&ef)[UN][NT], int u) {
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            const bool ok = u + j < ub;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                wf[j][t][0] = ok ? ldg_nt16(wp[t] + (size_t)(u + j) * 2048) : make_uint4(0, 0, 0, 0);
                wf[j][t][1] = ok ? ldg_nt16(wp[t] + (size_t)(u + j) * 2048 + 16) : make_uint4(0, 0, 0, 0);
                ef[j][t] = ok ? (unsigned int)__builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(ep[t] + (size_t)(u + j) * 128)) : 0u;
            }
        }
    };
    f32x4_t acc[NT][NB];
    bool parked = false;
    for (int task = team; task < T; task += nteams) {
    const int tile = rg * T + task;
    const bool active = tile < ntiles;
    const int n0 = tile * 16 * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const size_t blk = (size_t)(active ? tile * NT + t : 0) * U + u_beg;
        wp[t] = W + blk * 2048 + lane * 32;
        ep[t] = E + blk * 128 + lane * 2;
    }
    const bool work = active && ua < ub;
    if (work) loadw(wa, ea, ua);
    // park X[:, chunk]: combo c = (unit*8 + q)*NB + nb, one lane-linear 1 KB image per combo by LDS-DMA; rows >= B read row B-1
    if (!parked) {
        const int combos = nu * IPU * NB;
        for (int c = wid; c < combos; c += nwaves) {
            const int nb = c % NB, uq = c / NB, q = uq % IPU, u = uq / IPU;
            const int m = min(16 * nb + r, B - 1);
            const bf16_t* src = X + (size_t)m * ldx + (size_t)(u_beg + u) * 256 + g * 64 + q * 8;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(smem + (size_t)c * 1024), 16, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        parked = true;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[t][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto mma = [&](uint4 (&wf)[UN][NT][2], unsigned int (&ef)[UN][NT], int u) {
#pragma unroll
        for (int j = 0; j < UN; ++j) {
            if (u + j < ub) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float sc[NT];
#pragma unroll
                    for (int t = 0; t < NT; ++t) sc[t] = w4_scale((ef[j][t] >> (8 * h)) & 0xffu);
#pragma unroll
                    for (int d = 0; d < 4; ++d) {
                        bf16x8_t wq[NT];                 // fragment q = 4 h + d of every tile, widened once, used by every row group
#pragma unroll
                        for (int t = 0; t < NT; ++t) {
                            const uint4& w = wf[j][t][h];
                            wq[t] = widen8_w4(d == 0 ? w.x : d == 1 ? w.y : d == 2 ? w.z : w.w, sc[t]);
                        }
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) {
                            const bf16x8_t xq = __builtin_bit_cast(bf16x8_t, xs[(((u + j) * IPU + 4 * h + d) * NB + nb) * 64 + lane]);
#pragma unroll
                            for (int t = 0; t < NT; ++t) acc[t][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wq[t], xq, acc[t][nb], 0, 0, 0);
                        }
                    }
                }
            }
        }
    };
    if (work) {
        for (int u = ua; u < ub; u += 2 * UN) {
            if (u + UN < ub) loadw(wb, eb, u + UN);
            mma(wa, ea, u);
            if (u + UN < ub) {
                if (u + 2 * UN < ub) loadw(wa, ea, u + 2 * UN);
                mma(wb, eb, u + UN);
            }
        }
    }
    if (WPT > 1) {                                       // the WPT waves of a task: fixed-order sum through LDS (workgroup-uniform branch)
        if (active) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) red[((team * WPT + wsub) * NF + t * NB + nb) * 64 + lane] = acc[t][nb];
        }
        __syncthreads();
        if (active && wsub == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    f32x4_t sacc = red[((team * WPT) * NF + t * NB + nb) * 64 + lane];
                    for (int w = 1; w < WPT; ++w) sacc += red[((team * WPT + w) * NF + t * NB + nb) * 64 + lane];
                    acc[t][nb] = sacc;
                }
        }
    }
    if (!active || wsub != 0) continue;
    float* pr = ws + (size_t)ks * SK_ROWS * N;           // lane (r, g): out[m = 16 nb + r][n0 + t*16 + g*4 + 0..3]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int m = 16 * nb + r;
            if (m < B) *reinterpret_cast<f32x4_t*>(pr + (size_t)m * N + n0 + t * 16 + g * 4) = acc[t][nb];
        }
    }   // task loop
}

template <int NB, int NT>
int w4_launch(const SkinnyPlan& p, const bf16_t* X, long ldx, const uint8_t* W, const uint8_t* E, int B, int N, int K, float* ws, hipStream_t s) {
    static LdsGrantSized grant;
    if (!grant_dynamic_lds(grant, reinterpret_cast<const void*>(skinny_w4_kernel<NB, NT>), p.lds_bytes)) return TRACE_ERR_HIP;
    hipLaunchKernelGGL((skinny_w4_kernel<NB, NT>), dim3(p.grid), dim3(p.threads), p.lds_bytes, s, X, ldx, W, E, B, K, p.chunk_units, p.KS, p.T, p.WPT,
                       p.ntiles, ws, N);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}
int blocks_for(long total) { return (int)std::min<long>((total + 255) / 256, 65536); }
}  // namespace

int launch_quant_rows_w4(const bf16_t* W, long ldw, uint8_t* codes, uint8_t* exps, int N, int K, hipStream_t s) {
    if (N < 1 || K < 32 || K % 32 || ldw % 8 || ldw < K) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(quant_rows_w4_kernel, dim3(blocks_for((long)N * (K / 32))), dim3(256), 0, s, W, ldw, codes, exps, N, K);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_tile_pack_w4(const uint8_t* codes, const uint8_t* exps, uint8_t* tcodes, uint8_t* texps, int N, int K, int tile0, int tile_step, hipStream_t s) {
    if (N < 16 || N % 16 || K < 256 || K % 256 || tile0 < 0 || tile_step < 1) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(tile_pack_w4_kernel, dim3(blocks_for((long)N * (K / 32))), dim3(256), 0, s, codes, exps, tcodes, texps, N, K, tile0, tile_step);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_dequant_w4(const uint8_t* tcodes, const uint8_t* texps, bf16_t* out, long ldo, int N, int K, hipStream_t s) {
    if (N < 16 || N % 16 || K < 256 || K % 256 || ldo % 8 || ldo < K) return TRACE_ERR_ARG;
    hipLaunchKernelGGL(dequant_w4_kernel, dim3(blocks_for((long)N * (K / 32))), dim3(256), 0, s, tcodes, texps, out, ldo, N, K);
    return hipGetLastError() == hipSuccess ? TRACE_OK : TRACE_ERR_HIP;
}

int launch_skinny_w4(const bf16_t* X, long ldx, const uint8_t* tcodes, const uint8_t* texps, int B, int N, int K, float* ws, size_t ws_floats, hipStream_t s) {
    if (!skinny_shape_ok(SK_W4A16, N, K, EPI_PARTIAL, B) || ldx % 8 || ldx < K) return TRACE_ERR_ARG;
    const SkinnyPlan p = skinny_plan(SK_W4A16, N, K, EPI_PARTIAL, B);
    if (!ws || ws_floats < (size_t)p.KS * SK_ROWS * N) return TRACE_ERR_ARG;
    return skinny_by_nb(p.NB, [&](auto nb) {
        return p.NT == 2 ? w4_launch<decltype(nb)::value, 2>(p, X, ldx, tcodes, texps, B, N, K, ws, s)
                         : w4_launch<decltype(nb)::value, 1>(p, X, ldx, tcodes, texps, B, N, K, ws, s);
    });
}
