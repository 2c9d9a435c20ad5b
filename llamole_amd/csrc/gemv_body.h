// The body of the f32-FMA weight-streaming GEMV (ll_gemv_fused_bf16), shared by the dense kernel (llm_layer.hip) and the expert-indexed
// kernels of the sparse-MoE block (llm_moe.hip): one device function, so that a token row that is alone on its expert is rounded bit for
// bit like the dense GEMV on that expert's matrix -- the reasoning of head_pair for the q/k norm.  The token rows are given as pointers
// (the dense kernel's rows are X + m * ldx, the MoE kernels gather the rows of one expert), everything else is the dense kernel's.
#pragma once
#include "common.h"

namespace ll {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bfr2(float v) { return bf16_to_f32(f32_to_bf16(v)); }   // round through bf16

// GEMV_SCALE (MoE down projection only): bf16( bf16(acc) * row_scale[m] ) -- the routing weight applied to the rounded expert output
// GEMV_RESIDUAL_SCALED (Granite layout, ll_gemv_fused_rs_bf16): bf16( residual + bf16( bf16(acc + bias) * row_scale[m] ) ) -- the layer's
//     residual_multiplier (the same float in every row) applied to the rounded Linear output, as HF's `residual + hidden_states * m`
enum { GEMV_PLAIN = 0, GEMV_RESIDUAL = 1, GEMV_SILU_MUL = 2, GEMV_SCALE = 3, GEMV_RESIDUAL_SCALED = 4 };
// 16-byte weight loads per row in flight per lane at one token row (x 2 rows per wave).  Re-swept once the kernels were built with
// kernel-argument preloading: 4 beats the earlier 8 (q|k|v 9.2 -> 8.2 us, LLM part of a molecule 353.6 -> 347.1 ms with the
// plain GEMV of lm_head at 4 as well); the FMA order per output row does not depend on it.
#ifndef LL_GEMV_UNR
#define LL_GEMV_UNR 4
#endif
#ifndef LL_GEMV_STAGE_UNR
#define LL_GEMV_STAGE_UNR 4
#endif

template <bool NT> __device__ __forceinline__ u32x4 ldw16(const bf16_t *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return *reinterpret_cast<const u32x4 *>(p);
}

template <int UNR, bool NT>
__device__ __forceinline__ void gemv_load_w(u32x4 (&wv)[UNR][2], const bf16_t *const (&wr)[2], int c0, int nchunk, bool active) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
        const int c = c0 + u * 64;
#pragma unroll
        for (int r = 0; r < 2; ++r) wv[u][r] = (active && c < nchunk) ? ldw16<NT>(wr[r] + c * 8) : (u32x4)(0);
    }
}

// acc += w . x over UNR 16-byte chunks per lane; x rows at xp + m*ldx (LDS when XLDS)
template <int MROWS, int UNR, bool XLDS>
__device__ __forceinline__ void gemv_fma(float (&acc)[MROWS][2], const u32x4 (&wv)[UNR][2], const bf16_t *xp, int64_t ldx, int c0,
                                         int nchunk) {
    u32x4 xv[UNR][MROWS];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
        const int c = c0 + u * 64;
#pragma unroll
        for (int m = 0; m < MROWS; ++m) xv[u][m] = c < nchunk ? *reinterpret_cast<const u32x4 *>(xp + (int64_t)m * ldx + c * 8) : (u32x4)(0);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
        for (int m = 0; m < MROWS; ++m) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float a = acc[m][r];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    a = fmaf(__uint_as_float(wv[u][r][t] << 16), __uint_as_float(xv[u][m][t] << 16), a);
                    a = fmaf(__uint_as_float(wv[u][r][t] & 0xffff0000u), __uint_as_float(xv[u][m][t] & 0xffff0000u), a);
                }
                acc[m][r] = a;
            }
        }
    }
}

// One workgroup of 256 threads = 4 waves; ``wave`` is the wave's index over the whole matrix.  Each wave owns two weight rows
// (GEMV_SILU_MUL: gate row n and up row n + N; otherwise rows 2w, 2w+1); a lane reads 16 B of each row per step with UNR steps in flight,
// x comes from LDS (NORM: the workgroup normalises its MROWS rows once into xs [MROWS][K], with the first weight loads already in flight;
// red [MROWS][4] is its reduction scratch) or from L1/L2.  f32 FMA chains in the lane/chunk order of gemv_bf16_kernel.
// Token row m: x at xr[m], residual at rr[m] (GEMV_RESIDUAL, GEMV_RESIDUAL_SCALED), output at cr[m], routing weight / residual multiplier
// rs[m] (GEMV_SCALE / GEMV_RESIDUAL_SCALED).
// Every thread of the workgroup must call it (NORM has two barriers); a caller that calls it again puts a barrier in between (xs, red).
template <int MROWS, bool NORM, int EPI, bool NT, int XC>
__device__ __forceinline__ void gemv_fused_body(const bf16_t *const (&xr)[MROWS], const bf16_t *__restrict__ W, int ldw,
                                                const float *__restrict__ bias, const bf16_t *__restrict__ normw, float eps,
                                                const bf16_t *const (&rr)[MROWS], bf16_t *const (&cr)[MROWS], const float (&rs)[MROWS],
                                                int N, int K, int wave, bf16_t *xs, float (*red)[4]) {
    constexpr int R = 2, UNR = MROWS == 1 ? LL_GEMV_UNR : 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n0 = EPI == GEMV_SILU_MUL ? wave : wave * R;
    const bool active = n0 < N;     // whole waves; inactive waves still take part in the NORM barriers
    const bf16_t *wr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = EPI == GEMV_SILU_MUL ? (int64_t)(n0 < N ? n0 : N - 1) + (int64_t)r * N : (n0 + r < N ? n0 + r : N - 1);
        wr[r] = W + row * ldw;
    }
    const int nchunk = K / 8;
    // XC 16-byte chunks of x per thread (K <= 2048 XC): keeping it at 2 for hidden sizes <= 4096 holds the kernel at
    // <= 128 VGPRs = 4 waves per SIMD
    u32x4 xv0[MROWS][XC], nw0[XC];
    if (NORM) {   // x (and the norm weight) first: vmcnt retires in order, the weight loads below stay in flight
#pragma unroll
        for (int c = 0; c < XC; ++c) {
            const int ch = tid + c * 256;
            const bool ok = ch < nchunk;
#pragma unroll
            for (int m = 0; m < MROWS; ++m) xv0[m][c] = ok ? *reinterpret_cast<const u32x4 *>(xr[m] + ch * 8) : (u32x4)(0);
            nw0[c] = ok ? *reinterpret_cast<const u32x4 *>(normw + ch * 8) : (u32x4)(0);
        }
    }
    u32x4 wv[UNR][R];
    if (NORM) gemv_load_w<UNR, NT>(wv, wr, lane, nchunk, active);
    if (NORM) {
        // same summation order as rmsnorm_bf16_kernel: per-thread fmaf chain over its chunks, wave_sum, 4 partials
#pragma unroll
        for (int m = 0; m < MROWS; ++m) {
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < XC; ++c)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float a = __uint_as_float(xv0[m][c][t] << 16), b = __uint_as_float(xv0[m][c][t] & 0xffff0000u);
                    ss = fmaf(a, a, ss);
                    ss = fmaf(b, b, ss);
                }
            ss = wave_sum(ss);
            if (lane == 0) red[m][tid >> 6] = ss;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MROWS; ++m) {
            const float var = (red[m][0] + red[m][1] + red[m][2] + red[m][3]) / (float)K;
            const float rstd = rsqrtf(var + eps);
#pragma unroll
            for (int c = 0; c < XC; ++c) {
                const int ch = tid + c * 256;
                if (ch < nchunk) {
                    u32x4 o;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float a = bfr2(__uint_as_float(xv0[m][c][t] << 16) * rstd) * __uint_as_float(nw0[c][t] << 16);
                        const float b = bfr2(__uint_as_float(xv0[m][c][t] & 0xffff0000u) * rstd) * __uint_as_float(nw0[c][t] & 0xffff0000u);
                        o[t] = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
                    }
                    *reinterpret_cast<u32x4 *>(xs + (int64_t)m * K + ch * 8) = o;
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float acc[MROWS][R];
#pragma unroll
    for (int m = 0; m < MROWS; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
    int cbeg = lane;
    if (NORM) {   // first block: its weights were requested before the normalisation
        gemv_fma<MROWS, UNR, true>(acc, wv, xs, K, lane, nchunk);
        cbeg += 64 * UNR;
    }
    for (int c0 = cbeg; c0 < nchunk; c0 += 64 * UNR) {
        if (NORM) {
            gemv_load_w<UNR, NT>(wv, wr, c0, nchunk, true);
            gemv_fma<MROWS, UNR, true>(acc, wv, xs, K, c0, nchunk);
        } else {
            // x chunk u right behind weight chunk u (loads retire in order: the first FMAs need not wait for all of W)
            u32x4 xv[UNR][MROWS];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int c = c0 + u * 64;
                const bool ok = c < nchunk;
#pragma unroll
                for (int r = 0; r < R; ++r) wv[u][r] = ok ? ldw16<NT>(wr[r] + c * 8) : (u32x4)(0);
#pragma unroll
                for (int m = 0; m < MROWS; ++m) xv[u][m] = ok ? *reinterpret_cast<const u32x4 *>(xr[m] + c * 8) : (u32x4)(0);
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
#pragma unroll
                for (int m = 0; m < MROWS; ++m) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        float a = acc[m][r];
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            a = fmaf(__uint_as_float(wv[u][r][t] << 16), __uint_as_float(xv[u][m][t] << 16), a);
                            a = fmaf(__uint_as_float(wv[u][r][t] & 0xffff0000u), __uint_as_float(xv[u][m][t] & 0xffff0000u), a);
                        }
                        acc[m][r] = a;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MROWS; ++m) {
        float v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = wave_sum(acc[m][r]);
        if (lane == 0) {
            if (EPI == GEMV_SILU_MUL) {
                const float g = bfr2(v[0] + (bias ? bias[n0] : 0.f)), up = bfr2(v[1] + (bias ? bias[n0 + N] : 0.f));
                cr[m][n0] = f32_to_bf16(bfr2(silu(g)) * up);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (n0 + r < N) {
                        float o = v[r] + (bias ? bias[n0 + r] : 0.f);
                        if (EPI == GEMV_RESIDUAL) o = bf16_to_f32(rr[m][n0 + r]) + bfr2(o);
                        if (EPI == GEMV_SCALE) o = bfr2(o) * rs[m];
                        if (EPI == GEMV_RESIDUAL_SCALED) o = bf16_to_f32(rr[m][n0 + r]) + bfr2(bfr2(o) * rs[m]);
                        cr[m][n0 + r] = f32_to_bf16(o);
                    }
                }
            }
        }
    }
}

}  // namespace ll
