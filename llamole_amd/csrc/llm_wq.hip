// Weight-only MX quantisation of the decode step's Linear weights (quantization_bit: 8 | 4): the decode token is bound by the weight
// stream, so the seven Linears of a decoder layer are rounded ONCE onto an OCP microscaling grid and decode calls of 1..16 token rows
// stream the packed codes instead of the bf16 matrices.
//
// Format (both widths): blocks of 32 consecutive elements along K share one E8M0 scale 2^e stored as the byte e + 127; elements are
// FP8 E4M3 (OCP e4m3fn, max 448) at 8 bits and FP4 E2M1 (0, 0.5, 1, 1.5, 2, 3, 4, 6) at 4 bits.  Quantiser: amax = max |w| of the block
// (bf16 values); e = the smallest integer with amax * 2^-e <= elem_max, from the exponent and mantissa bits of amax, clamped so that
// every dequantised value is a normal bf16 number (8 bits: [-117, 119], 4 bits: [-125, 125]); e = 0 for an all-zero block; element =
// w * 2^-e rounded to the nearest grid value, ties to even.  Rounding e UP means no element saturates (the OCP floor rule would clip
// the block maximum).  E4M3 has 3 mantissa bits, E2M1 one, the scale is a power of two: code * 2^e is EXACTLY a bf16 number, so the
// dequantised matrix is an ordinary bf16 weight and every bf16 path computes the same model as the packed-code kernels.
//
// Layout of `packed` for an [N, K] matrix (ll_wq_bytes(N, K, bits) bytes; tests reach it only through the entry points):
//   bytes [0, N * K * bits / 8)   codes, row-major, row pitch K * bits / 8 (a multiple of 16: K % 32 == 0); at 4 bits element 2i sits in
//                                 the LOW nibble of byte i and element 2i + 1 in the high nibble;
//   then N * K / 32 bytes         scale bytes, row-major, row pitch K / 32.
// Rows stay contiguous, so adjacent lanes read contiguous 16-byte pieces of one row (>= 128 B per row segment: what a CU needs to
// pull its share of HBM, tools/ingest_probe.hip) and the scale bytes of those lanes are contiguous as well.
//
// Kernels: codes are expanded in registers by v_cvt_scalef32_pk_{f32,bf16}_{fp8,fp4} with the block's scale as the f32 scale operand.
//   gemv_wq_kernel    1..4 token rows, f32 FMA (the ll_gemv_fused_bf16 counterpart): a lane reads 16 B of codes per row and step
//                     (16 elements at 8 bits, 32 at 4) with UNR steps in flight; x sits in LDS, stored so that the 16-byte pieces
//                     the 64 lanes read together are contiguous (no bank conflicts although a lane's elements span 32 / 64 B of x).
//   rows16_wq_kernel  1..16 token rows on v_mfma_f32_16x16x32_bf16 (the ll_linear_rows16_bf16 counterpart): every wave streams the
//                     codes of its 16 weight rows and expands them to bf16 on the way from registers into its private LDS image.
//                     The image keeps the k order of the CODE lanes -- piece j of all lanes of a row is contiguous -- and the x image
//                     uses the same order, which a dot product does not see; writes and fragment reads stay conflict-free.
#include "common.h"
#include "mx_quant.h"

namespace ll {

typedef uint32_t wq_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wq_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(2))) float wq_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 wq_bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 wq_bf16x8;
typedef __attribute__((ext_vector_type(4))) float wq_f32x4;

enum { WQ_PLAIN = 0, WQ_RESIDUAL = 1, WQ_SILU_MUL = 2 };

__device__ __forceinline__ float wq_bfr(float v) { return bf16_to_f32(f32_to_bf16(v)); }
__device__ __forceinline__ float wq_scale_f32(uint32_t byte) { return __uint_as_float(byte << 23); }     // E8M0 byte -> 2^(byte - 127)
__device__ __forceinline__ float wq_lo(uint32_t v) { return __uint_as_float(v << 16); }
__device__ __forceinline__ float wq_hi(uint32_t v) { return __uint_as_float(v & 0xffff0000u); }

// ---------------------------------------------------------------------------------------------------------------- quantiser
// (wq_block_exp and wq_encode: mx_quant.h)
// four lanes per block of 32 elements (16 B of bf16 each): coalesced reads and writes; Wdq may alias W (a lane writes what it alone read;
// neither pointer is __restrict__)
template <int BITS>
__global__ __launch_bounds__(256) void wq_quantize_kernel(const bf16_t *W, int64_t ldw, int N, int K, unsigned char *codes,
                                                          unsigned char *scales, bf16_t *Wdq, int64_t lddq) {
    const int k8 = K / 8;
    const int64_t total = (int64_t)N * k8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {     // total % 4 == 0: quads stay whole
        const int row = (int)(i / k8), c = (int)(i - (int64_t)row * k8);
        const wq_u32x4 v = *reinterpret_cast<const wq_u32x4 *>(W + row * ldw + c * 8);
        uint32_t am = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t a = v[t] & 0x7fffu, b = (v[t] >> 16) & 0x7fffu;
            am = am > a ? am : a;
            am = am > b ? am : b;
        }
        const uint32_t o1 = (uint32_t)__shfl_xor((int)am, 1, 64);
        am = am > o1 ? am : o1;
        const uint32_t o2 = (uint32_t)__shfl_xor((int)am, 2, 64);
        am = am > o2 ? am : o2;
        const int e = wq_block_exp<BITS>(am);
        const float inv = __uint_as_float((uint32_t)(127 - e) << 23), sc = __uint_as_float((uint32_t)(127 + e) << 23);
        uint32_t code[8];
        wq_u32x4 dq;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint32_t o = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t bits = h ? (v[t] >> 16) : (v[t] & 0xffffu);
                float g;
                const uint32_t cd = wq_encode<BITS>(fabsf(bf16_to_f32((bf16_t)bits)) * inv, &g);
                const uint32_t sign = bits >> 15;
                code[t * 2 + h] = cd | (sign << (BITS - 1));
                o |= (((uint32_t)f32_to_bf16(g * sc)) | (sign << 15)) << (16 * h);
            }
            dq[t] = o;
        }
        if (codes) {
            if (BITS == 8) {
                wq_u32x2 o;
                o[0] = code[0] | code[1] << 8 | code[2] << 16 | code[3] << 24;
                o[1] = code[4] | code[5] << 8 | code[6] << 16 | code[7] << 24;
                *reinterpret_cast<wq_u32x2 *>(codes + (int64_t)row * K + c * 8) = o;
            } else {
                uint32_t o = 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) o |= code[t] << (4 * t);
                *reinterpret_cast<uint32_t *>(codes + (int64_t)row * (K / 2) + c * 4) = o;
            }
            if ((c & 3) == 0) scales[(int64_t)row * (K / 32) + (c >> 2)] = (unsigned char)(e + 127);
        }
        if (Wdq) *reinterpret_cast<wq_u32x4 *>(Wdq + row * lddq + c * 8) = dq;
    }
}

// 8 codes (two dwords at 8 bits, one at 4) -> 8 bf16 through the hardware conversion
template <int BITS> __device__ __forceinline__ wq_u32x4 wq_expand8(uint32_t c0, uint32_t c1, float s) {
    wq_u32x4 o;
    if (BITS == 8) {
        o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, s, false));
        o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c0, s, true));
        o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, s, false));
        o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c1, s, true));
    } else {
        o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c0, s, 0));
        o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c0, s, 1));
        o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c0, s, 2));
        o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c0, s, 3));
    }
    return o;
}

template <int BITS>
__global__ __launch_bounds__(256) void wq_dequantize_kernel(const unsigned char *__restrict__ codes, const unsigned char *__restrict__ scales,
                                                            int N, int K, bf16_t *__restrict__ W, int64_t ldw) {
    const int k8 = K / 8;
    const int64_t total = (int64_t)N * k8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int row = (int)(i / k8), c = (int)(i - (int64_t)row * k8);
        const float s = wq_scale_f32(scales[(int64_t)row * (K / 32) + (c >> 2)]);
        uint32_t c0, c1 = 0;
        if (BITS == 8) {
            const wq_u32x2 v = *reinterpret_cast<const wq_u32x2 *>(codes + (int64_t)row * K + c * 8);
            c0 = v[0], c1 = v[1];
        } else {
            c0 = *reinterpret_cast<const uint32_t *>(codes + (int64_t)row * (K / 2) + c * 4);
        }
        *reinterpret_cast<wq_u32x4 *>(W + row * ldw + c * 8) = wq_expand8<BITS>(c0, c1, s);
    }
}

// ---------------------------------------------------------------------------------------------------------------- GEMV, 1..4 rows
// acc[m][r] += sum over the 16 B of codes `w` (scale s) of row r times the matching x pieces xv[m][P] (P pieces of 8 bf16)
template <int BITS, int MROWS, int P>
__device__ __forceinline__ void wq_fma_chunk(float (&acc)[MROWS][2], int r, const wq_u32x4 w, float s, const wq_u32x4 (&xv)[MROWS][P]) {
#define LL_WQ_FMA2(V, XD)                                         \
    _Pragma("unroll") for (int m = 0; m < MROWS; ++m) {           \
        const uint32_t xd = (XD);                                 \
        acc[m][r] = fmaf((V).x, wq_lo(xd), acc[m][r]);            \
        acc[m][r] = fmaf((V).y, wq_hi(xd), acc[m][r]);            \
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (BITS == 8) {       // dword t = elements 4t .. 4t+3 = piece t / 2, dwords 2 (t & 1), 2 (t & 1) + 1
            const wq_f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[t], s, false);
            const wq_f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[t], s, true);
            LL_WQ_FMA2(lo, xv[m][(t >> 1) % P][(t & 1) * 2])
            LL_WQ_FMA2(hi, xv[m][(t >> 1) % P][(t & 1) * 2 + 1])
        } else {               // dword t = elements 8t .. 8t+7 = piece t, byte b = dword b of the piece
            const wq_f32x2 v0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[t], s, 0);
            const wq_f32x2 v1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[t], s, 1);
            const wq_f32x2 v2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[t], s, 2);
            const wq_f32x2 v3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[t], s, 3);
            LL_WQ_FMA2(v0, xv[m][t % P][0])
            LL_WQ_FMA2(v1, xv[m][t % P][1])
            LL_WQ_FMA2(v2, xv[m][t % P][2])
            LL_WQ_FMA2(v3, xv[m][t % P][3])
        }
    }
#undef LL_WQ_FMA2
}

// Each wave owns two weight rows (WQ_SILU_MUL: gate row n and up row n + N; otherwise rows 2w, 2w + 1).  A "chunk" is 16 B of codes
// (EPC = 16 | 32 elements); chunk c of a row belongs to lane c % 64.  x lives in LDS as 16-byte pieces (8 bf16): piece j of chunk c at
// index ((c / 64) * P + j) * 64 + c % 64, so the 64 lanes of a wave read 1 KB contiguous per piece.  XC = 16-byte pieces of x per
// thread held in registers by the RMSNorm prologue (K <= 2048 XC); without the prologue (XC = 0) x is copied by a loop.
template <int BITS, int MROWS, bool NORM, int EPI, int XC>
__global__ __launch_bounds__(256) void gemv_wq_kernel(const bf16_t *__restrict__ X, int ldx, const unsigned char *__restrict__ codes,
                                                      const unsigned char *__restrict__ scales, const float *__restrict__ bias,
                                                      const bf16_t *__restrict__ normw, float eps, const bf16_t *__restrict__ res, int ldr,
                                                      bf16_t *__restrict__ C, int ldc, int N, int K) {
    // 16-byte code loads per row in flight per lane: 4 at one token row (64 / 128 elements per row), 2 at two, 1 at three and four (the x
    // pieces of a step are MROWS * P registers of 16 B: more steps in flight at 3..4 rows of 4-bit codes overflow the register file)
    constexpr int R = 2, UNR = MROWS == 1 ? 4 : (MROWS == 2 ? 2 : 1), EPC = 128 / BITS, P = EPC / 8;
    constexpr int XCR = XC > 0 ? XC : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_wq[];
    wq_u32x4 *xs = reinterpret_cast<wq_u32x4 *>(sm_wq);     // [MROWS][kp16] pieces
    __shared__ float red[MROWS][4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = blockIdx.x * 4 + (tid >> 6);
    const int n0 = EPI == WQ_SILU_MUL ? wave : wave * R;
    const bool active = n0 < N;     // whole waves; inactive waves still take part in the barriers
    const int nchunk = K / EPC, nch8 = K / 8, kp16 = ((nchunk + 63) / 64) * 64 * P;
    const unsigned char *wr[R], *sr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = EPI == WQ_SILU_MUL ? (int64_t)(n0 < N ? n0 : N - 1) + (int64_t)r * N : (n0 + r < N ? n0 + r : N - 1);
        wr[r] = codes + row * (K / 8 * BITS);
        sr[r] = scales + row * (K / 32);
    }
    auto dest16 = [&](int ch) {
        const int c = ch / P, j = ch % P;
        return ((c >> 6) * P + j) * 64 + (c & 63);
    };
    wq_u32x4 xv0[MROWS][XCR], nw0[XCR];
    if (NORM) {   // x (and the norm weight) first: vmcnt retires in order, the weight loads below stay in flight
#pragma unroll
        for (int c = 0; c < XCR; ++c) {
            const int ch = tid + c * 256;
            const bool ok = ch < nch8;
#pragma unroll
            for (int m = 0; m < MROWS; ++m) xv0[m][c] = ok ? *reinterpret_cast<const wq_u32x4 *>(X + (int64_t)m * ldx + ch * 8) : (wq_u32x4)(0);
            nw0[c] = ok ? *reinterpret_cast<const wq_u32x4 *>(normw + ch * 8) : (wq_u32x4)(0);
        }
    }
    wq_u32x4 wv[UNR][R];
    uint32_t sb[UNR][R];
    auto load_w = [&](int c0, bool on) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int c = c0 + u * 64;
            const bool ok = on && c < nchunk;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                wv[u][r] = ok ? __builtin_nontemporal_load(reinterpret_cast<const wq_u32x4 *>(wr[r] + (int64_t)c * 16)) : (wq_u32x4)(0);
                sb[u][r] = ok ? (uint32_t)__builtin_nontemporal_load(sr[r] + (c * EPC) / 32) : 127u;
            }
        }
    };
    load_w(lane, active);
    if (NORM) {
        // same summation order as rmsnorm_bf16_kernel: per-thread fmaf chain over its pieces, wave_sum, 4 partials
#pragma unroll
        for (int m = 0; m < MROWS; ++m) {
            float ss = 0.f;
#pragma unroll
            for (int c = 0; c < XCR; ++c)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float a = wq_lo(xv0[m][c][t]), b = wq_hi(xv0[m][c][t]);
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
            for (int c = 0; c < XCR; ++c) {
                const int ch = tid + c * 256;
                if (ch < nch8) {
                    wq_u32x4 o;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float a = wq_bfr(wq_lo(xv0[m][c][t]) * rstd) * wq_lo(nw0[c][t]);
                        const float b = wq_bfr(wq_hi(xv0[m][c][t]) * rstd) * wq_hi(nw0[c][t]);
                        o[t] = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
                    }
                    xs[m * kp16 + dest16(ch)] = o;
                }
            }
        }
    } else {
        for (int i = tid; i < MROWS * nch8; i += 256) {
            const int m = i / nch8, ch = i - m * nch8;
            xs[m * kp16 + dest16(ch)] = *reinterpret_cast<const wq_u32x4 *>(X + (int64_t)m * ldx + ch * 8);
        }
    }
    __syncthreads();
    if (!active) return;
    float acc[MROWS][R];
#pragma unroll
    for (int m = 0; m < MROWS; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
    for (int c0 = lane; c0 < nchunk; c0 += 64 * UNR) {
        if (c0 != lane) load_w(c0, true);       // the first block was requested before x was staged
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int c = c0 + u * 64;
            const bool ok = c < nchunk;
            const int base = (c >> 6) * P * 64 + lane;
            wq_u32x4 xv[MROWS][P];
#pragma unroll
            for (int m = 0; m < MROWS; ++m)
#pragma unroll
                for (int j = 0; j < P; ++j) xv[m][j] = ok ? xs[m * kp16 + base + j * 64] : (wq_u32x4)(0);
#pragma unroll
            for (int r = 0; r < R; ++r) wq_fma_chunk<BITS, MROWS, P>(acc, r, wv[u][r], wq_scale_f32(sb[u][r]), xv);
        }
    }
#pragma unroll
    for (int m = 0; m < MROWS; ++m) {
        float v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = wave_sum(acc[m][r]);
        if (lane == 0) {
            if (EPI == WQ_SILU_MUL) {
                const float g = wq_bfr(v[0] + (bias ? bias[n0] : 0.f)), up = wq_bfr(v[1] + (bias ? bias[n0 + N] : 0.f));
                C[(int64_t)m * ldc + n0] = f32_to_bf16(wq_bfr(silu(g)) * up);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (n0 + r < N) {
                        float o = v[r] + (bias ? bias[n0 + r] : 0.f);
                        if (EPI == WQ_RESIDUAL) o = bf16_to_f32(res[(int64_t)m * ldr + n0 + r]) + wq_bfr(o);
                        C[(int64_t)m * ldc + n0 + r] = f32_to_bf16(o);
                    }
                }
            }
        }
    }
}

template <int BITS, int MROWS, bool NORM, int EPI, int XC>
static int launch_gemv_wq(hipStream_t s, const bf16_t *X, int ldx, const unsigned char *codes, const unsigned char *scales, const float *bias,
                          const bf16_t *normw, float eps, const bf16_t *res, int ldr, bf16_t *C, int ldc, int N, int K) {
    constexpr int EPC = 128 / BITS, P = EPC / 8;
    const size_t lds = (size_t)MROWS * ((K / EPC + 63) / 64) * 64 * P * 16;
    LL_TRY((allow_dynamic_lds<gemv_wq_kernel<BITS, MROWS, NORM, EPI, XC>>(lds)));
    const dim3 grid(EPI == WQ_SILU_MUL ? cdiv(N, 4) : cdiv(N, 8));
    hipLaunchKernelGGL((gemv_wq_kernel<BITS, MROWS, NORM, EPI, XC>), grid, dim3(256), lds, s, X, ldx, codes, scales, bias, normw, eps, res, ldr, C,
                       ldc, N, K);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

template <int BITS, int MROWS>
static int dispatch_gemv_wq(hipStream_t s, const bf16_t *X, int ldx, const unsigned char *codes, const unsigned char *scales, const float *bias,
                            const bf16_t *normw, float eps, const bf16_t *res, int ldr, bf16_t *C, int ldc, int N, int K, int epi) {
#define LL_WQ_CASE(NORM_, EPI_, XC_) return launch_gemv_wq<BITS, MROWS, NORM_, EPI_, XC_>(s, X, ldx, codes, scales, bias, normw, eps, res, ldr, C, ldc, N, K)
    if (normw) {
        if (K <= 4096) {
            if (epi == WQ_PLAIN) LL_WQ_CASE(true, WQ_PLAIN, 2);
            if (epi == WQ_RESIDUAL) LL_WQ_CASE(true, WQ_RESIDUAL, 2);
            LL_WQ_CASE(true, WQ_SILU_MUL, 2);
        }
        if (epi == WQ_PLAIN) LL_WQ_CASE(true, WQ_PLAIN, 4);
        if (epi == WQ_RESIDUAL) LL_WQ_CASE(true, WQ_RESIDUAL, 4);
        LL_WQ_CASE(true, WQ_SILU_MUL, 4);
    }
    if (epi == WQ_PLAIN) LL_WQ_CASE(false, WQ_PLAIN, 0);
    if (epi == WQ_RESIDUAL) LL_WQ_CASE(false, WQ_RESIDUAL, 0);
    LL_WQ_CASE(false, WQ_SILU_MUL, 0);
#undef LL_WQ_CASE
}

static int wq_check_packed(const char *who, const void *packed, int bits, int rows, int K) {
    LL_CHECK(bits == 4 || bits == 8, "%s: bits=%d (4 or 8)", who, bits);
    LL_CHECK(rows >= 1 && K >= 32 && K % 32 == 0, "%s: K=%d must be a multiple of 32 (one scale per 32 elements)", who, K);
    LL_CHECK(packed && ((uintptr_t)packed & 15) == 0, "%s: the packed buffer must be 16-byte aligned", who);
    return LL_OK;
}

static int gemv_fused_wq(const void *x, int ldx, const void *packed, int bits, const float *bias, const void *norm_w, float eps,
                         const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, hipStream_t s) {
    LL_CHECK(x && out, "ll_gemv_fused_wq: null argument");
    LL_CHECK(M >= 1 && M <= 4, "ll_gemv_fused_wq: M=%d rows (decode shapes only, 1..4)", M);
    LL_CHECK(epi >= WQ_PLAIN && epi <= WQ_SILU_MUL, "ll_gemv_fused_wq: epilogue %d", epi);
    const int rows = epi == WQ_SILU_MUL ? 2 * N : N;
    LL_TRY(wq_check_packed("ll_gemv_fused_wq", packed, bits, rows, K));
    LL_CHECK(N >= 1 && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0, "ll_gemv_fused_wq: ldx must be a multiple of 8 and x 16-byte aligned");
    LL_CHECK(epi != WQ_RESIDUAL || residual, "ll_gemv_fused_wq: residual epilogue without a residual");
    LL_CHECK(!norm_w || K <= 8192, "ll_gemv_fused_wq: RMSNorm prologue needs K <= 8192");
    const int epc = 128 / bits;
    // the x image (rows padded to 64 chunks) + the kernel's static 16 M bytes of row sums
    LL_CHECK((size_t)M * ((K / epc + 63) / 64) * 64 * epc * 2 + 16 * (size_t)M <= 160 * 1024, "ll_gemv_fused_wq: M=%d rows of K=%d do not fit the 160 KB of LDS", M, K);
    const unsigned char *codes = (const unsigned char *)packed, *scales = codes + (size_t)rows * K / 8 * bits;
    const bf16_t *X = (const bf16_t *)x, *nw = (const bf16_t *)norm_w, *rs = (const bf16_t *)residual;
    bf16_t *C = (bf16_t *)out;
#define LL_WQ_M(B_, M_) return dispatch_gemv_wq<B_, M_>(s, X, ldx, codes, scales, bias, nw, eps, rs, ldr, C, ldc, N, K, epi)
    if (bits == 8) {
        switch (M) {
            case 1: LL_WQ_M(8, 1);
            case 2: LL_WQ_M(8, 2);
            case 3: LL_WQ_M(8, 3);
            default: LL_WQ_M(8, 4);
        }
    }
    switch (M) {
        case 1: LL_WQ_M(4, 1);
        case 2: LL_WQ_M(4, 2);
        case 3: LL_WQ_M(4, 3);
        default: LL_WQ_M(4, 4);
    }
#undef LL_WQ_M
}

// ---------------------------------------------------------------------------------------------------------------- MFMA Linear, 1..16 rows
// CSEG = bytes of CODES of a row per block (128, at 8 bits also 256) = CSEG / 16 lanes per row; its bf16 image is SEGIMG = CSEG * 16 / BITS
// bytes (256 | 512) per row -- the image sizes of rows16_kernel; 256-byte segments of 4-bit codes would be a 1 KB image row and 16 x loads
// per lane and block, which no longer fits the register file.  A code lane holds EPC = 128 / BITS elements = P pieces of 16 B of bf16; piece j of code lane l goes to image
// column j * CSEG + l * 16 (adjacent lanes contiguous: conflict-free ds_write_b128 with the padded pitch), and the x loader (16 B of
// bf16 per lane, adjacent lanes contiguous in memory) writes its piece to the same column.  The fragment reads and the MFMA loop are
// those of rows16_kernel; which k sits in which column does not matter to a dot product as long as both images agree.
template <int EPI, int BITS, int CSEG, bool NORM>
__global__ __launch_bounds__(512) void rows16_wq_kernel(const bf16_t *__restrict__ X, int ldx, const unsigned char *__restrict__ codes,
                                                        const unsigned char *__restrict__ scales, const float *__restrict__ bias,
                                                        const bf16_t *__restrict__ normw, float eps, const bf16_t *__restrict__ res, int ldr,
                                                        bf16_t *__restrict__ C, int ldc, int M, int N, int K, int ksplit) {
    constexpr int NT = EPI == WQ_SILU_MUL ? 2 : 1;      // weight sub-tiles per wave (gate rows + the matching up rows)
    constexpr int EPC = 128 / BITS, P = EPC / 8;        // elements per code lane, 16-byte bf16 pieces per code lane
    constexpr int SEGIMG = CSEG * P, PITCH = SEGIMG + 16;       // (PITCH / 4) % 64 == 4: 16 rows cover the 64 banks once
    constexpr int BLK = SEGIMG / 2;                     // elements of K per block
    constexpr int LPR = CSEG / 16, RPI = 64 / LPR, IPT = 16 / RPI;          // code loads: lanes per row, rows per instruction, instructions per tile
    constexpr int XLPR = SEGIMG / 16, XRPI = 64 / XLPR, XIPT = 16 / XRPI;   // x loads
    constexpr int KSTEPS = SEGIMG / 64;
    constexpr int WAVE_LDS = (NT + 1) * 16 * PITCH;
    static_assert(SEGIMG == 256 || SEGIMG == 512, "image segment");
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_r16q[];
    const int tid = threadIdx.x, lane = tid & 63, waves = blockDim.x >> 6;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char *wl = sm_r16q + wid * WAVE_LDS;       // [NT*16 weight rows | 16 x rows][PITCH]
    unsigned char *xl = wl + NT * 16 * PITCH;
    const int tpw = waves / ksplit;
    const int tile = blockIdx.x * tpw + wid / ksplit, slice = wid % ksplit;
    const int ntiles = (N + 15) / 16;
    const bool tile_ok = tile < ntiles;
    // K range of this wave in elements (multiples of 32 = one scale block = one MFMA k-step)
    const int steps = K / 32, per = (steps + ksplit - 1) / ksplit;
    const int kb = min(slice * per, steps) * 32, ke = min((slice + 1) * per, steps) * 32;
    const int lrow = lane / LPR, lc = lane % LPR;       // code loads: row within an instruction, code lane within the segment
    const int xrow = lane / XLPR, xc = lane % XLPR;     // x loads: row within an instruction, 8-element piece within the segment
    const int xcol = (xc % P) * CSEG + (xc / P) * 16;   // image column of this lane's x piece
    const int n0 = tile * 16;
    const int64_t cpitch = (int64_t)K / 8 * BITS, spitch = K / 32;
    wq_f32x4 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = (wq_f32x4)(0.f);
    wq_u32x4 wr[NT][IPT], xr[XIPT], nwr = (wq_u32x4)(0);
    uint32_t sb[NT][IPT];
    float ssq[XIPT];                                    // NORM: sum of squares of this lane's x elements, per row of its instructions
#pragma unroll
    for (int q = 0; q < XIPT; ++q) ssq[q] = 0.f;
    auto load_block = [&](int k0) {
        const int kw = k0 + lc * EPC, kx = k0 + xc * 8;
        const bool win = kw < ke && tile_ok, xin = kx < ke && tile_ok;
        if (NORM) nwr = xin ? *reinterpret_cast<const wq_u32x4 *>(normw + kx) : (wq_u32x4)(0);
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                int row = n0 + q * RPI + lrow;
                row = row < N ? row : N - 1;
                const int64_t rr = (int64_t)row + (int64_t)s * N;
                wr[s][q] = win ? __builtin_nontemporal_load(reinterpret_cast<const wq_u32x4 *>(codes + rr * cpitch + kw / 8 * BITS)) : (wq_u32x4)(0);
                sb[s][q] = win ? (uint32_t)__builtin_nontemporal_load(scales + rr * spitch + kw / 32) : 127u;
            }
        }
#pragma unroll
        for (int q = 0; q < XIPT; ++q) {
            const int r = q * XRPI + xrow;
            xr[q] = (xin && r < M) ? *reinterpret_cast<const wq_u32x4 *>(X + (int64_t)r * ldx + kx) : (wq_u32x4)(0);
        }
    };
    const int fr = lane & 15, fq = lane >> 4;
    if (kb < ke) load_block(kb);
    for (int k0 = kb; k0 < ke; k0 += BLK) {
        // registers -> the wave's LDS image (the previous block's fragment reads have retired: same wave, in order)
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            const int r = q * RPI + lrow;
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                const float sc = wq_scale_f32(sb[s][q]);
                unsigned char *dst = wl + (s * 16 + r) * PITCH + lc * 16;
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const wq_u32x4 w = wr[s][q];
                    const wq_u32x4 e = BITS == 8 ? wq_expand8<BITS>(w[(2 * j) % 4], w[(2 * j + 1) % 4], sc) : wq_expand8<BITS>(w[j % 4], 0u, sc);
                    *reinterpret_cast<wq_u32x4 *>(dst + j * CSEG) = e;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < XIPT; ++q) {
            wq_u32x4 xv = xr[q];
            if (NORM) {     // x' = bf16(x * w_norm); the row's rsqrt(mean(x^2) + eps) multiplies the accumulator in the epilogue
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float a = wq_lo(xv[t]), b = wq_hi(xv[t]);
                    ssq[q] = fmaf(a, a, ssq[q]);
                    ssq[q] = fmaf(b, b, ssq[q]);
                    xv[t] = (uint32_t)f32_to_bf16(a * wq_lo(nwr[t])) | ((uint32_t)f32_to_bf16(b * wq_hi(nwr[t])) << 16);
                }
            }
            *reinterpret_cast<wq_u32x4 *>(xl + (q * XRPI + xrow) * PITCH + xcol) = xv;
        }
        if (k0 + BLK < ke) load_block(k0 + BLK);        // next block in flight while this one is multiplied
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) {
            const wq_bf16x8 b = *reinterpret_cast<const wq_bf16x8 *>(xl + fr * PITCH + (ks * 4 + fq) * 16);
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                const wq_bf16x8 a = *reinterpret_cast<const wq_bf16x8 *>(wl + (s * 16 + fr) * PITCH + (ks * 4 + fq) * 16);
                acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[s], 0, 0, 0);
            }
        }
    }
    // acc[s][j] = C[weight row n0 + (lane>>4)*4 + j][token row lane & 15]
    if (NORM) {             // lanes of one row segment -> one sum per row of this wave's K slice
#pragma unroll
        for (int q = 0; q < XIPT; ++q)
#pragma unroll
            for (int off = 1; off < XLPR; off <<= 1) ssq[q] += __shfl_xor(ssq[q], off, 64);
    }
    float rstd = 1.f;
    if (ksplit > 1) {
        __syncthreads();                                // every wave is done with its LDS image
        float *part = reinterpret_cast<float *>(sm_r16q);              // [waves][NT][64 lanes][4] | [waves][16] sums of squares
        float *psq = part + waves * NT * 256;
#pragma unroll
        for (int s = 0; s < NT; ++s) *reinterpret_cast<wq_f32x4 *>(part + ((wid * NT + s) * 64 + lane) * 4) = acc[s];
        if (NORM && xc == 0) {
#pragma unroll
            for (int q = 0; q < XIPT; ++q) psq[wid * 16 + q * XRPI + xrow] = ssq[q];
        }
        __syncthreads();
        if (slice != 0) return;
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            wq_f32x4 t = acc[s];
            for (int w = 1; w < ksplit; ++w) t += *reinterpret_cast<const wq_f32x4 *>(part + (((wid + w) * NT + s) * 64 + lane) * 4);
            acc[s] = t;
        }
        if (NORM) {
            float t = psq[wid * 16 + (lane & 15)];
            for (int w = 1; w < ksplit; ++w) t += psq[(wid + w) * 16 + (lane & 15)];
            rstd = rsqrtf(t / (float)K + eps);
        }
    } else if (NORM) {      // the wave owns the whole K: row sums through its own LDS image (same wave: in order)
        float *psq = reinterpret_cast<float *>(wl);
        if (xc == 0) {
#pragma unroll
            for (int q = 0; q < XIPT; ++q) psq[q * XRPI + xrow] = ssq[q];
        }
        rstd = rsqrtf(psq[lane & 15] / (float)K + eps);
    }
    if (NORM) {
#pragma unroll
        for (int s = 0; s < NT; ++s) acc[s] *= rstd;
    }
    if (!tile_ok) return;
    const int m = lane & 15, nb = n0 + (lane >> 4) * 4;
    if (m >= M) return;
    uint16_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = nb + j;
        const bool ok = n < N;
        if (EPI == WQ_SILU_MUL) {
            const float g = wq_bfr(acc[0][j] + ((bias && ok) ? bias[n] : 0.f));
            const float u = wq_bfr(acc[NT - 1][j] + ((bias && ok) ? bias[n + N] : 0.f));
            o[j] = f32_to_bf16(wq_bfr(silu(g)) * u);
        } else {
            float v = acc[0][j] + ((bias && ok) ? bias[n] : 0.f);
            if (EPI == WQ_RESIDUAL) v = (ok ? bf16_to_f32(res[(int64_t)m * ldr + n]) : 0.f) + wq_bfr(v);
            o[j] = f32_to_bf16(v);
        }
    }
    bf16_t *dst = C + (int64_t)m * ldc + nb;
    if (nb + 3 < N && ((reinterpret_cast<uintptr_t>(dst) & 7) == 0)) {
        *reinterpret_cast<uint2 *>(dst) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (nb + j < N) dst[j] = o[j];
    }
}

static int g_wq_geom = 0;     // 0: by shape; else cseg << 16 | waves << 8 | ksplit (tuning)

static size_t rows16_wq_lds(int bits, int cseg, int waves, int nt) { return (size_t)waves * (nt + 1) * 16 * (cseg * (16 / bits) + 16); }

template <int EPI, int BITS, int CSEG, bool NORM>
static int launch_rows16_wq_seg(int waves, int ksplit, hipStream_t s, const bf16_t *X, int ldx, const unsigned char *codes,
                                const unsigned char *scales, const float *bias, const bf16_t *normw, float eps, const bf16_t *res, int ldr,
                                bf16_t *C, int ldc, int M, int N, int K) {
    constexpr int NT = EPI == WQ_SILU_MUL ? 2 : 1;
    const int ntiles = (N + 15) / 16;
    const size_t lds = rows16_wq_lds(BITS, CSEG, waves, NT);
    LL_CHECK(lds <= 160 * 1024, "ll_linear_rows16_wq: %d waves x %d-byte code segments at %d bits need %zu bytes of LDS", waves, CSEG, BITS, lds);
    LL_TRY((allow_dynamic_lds<rows16_wq_kernel<EPI, BITS, CSEG, NORM>>(lds)));
    const int tpw = waves / ksplit;
    hipLaunchKernelGGL((rows16_wq_kernel<EPI, BITS, CSEG, NORM>), dim3((ntiles + tpw - 1) / tpw), dim3(waves * 64), lds, s, X, ldx, codes, scales,
                       bias, normw, eps, res, ldr, C, ldc, M, N, K, ksplit);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

// Geometry, derived for the narrower rows (a row of K elements is K * bits / 8 bytes of codes, a block covers CSEG * 8 / bits elements):
// K is split until there are ~14 waves per CU as for the bf16 kernel (what limits a wave is its own load -> expand -> LDS -> MFMA
// chain), but never so far that a wave is left with fewer than two blocks.  256-byte code segments (16 lanes per row: conflict-free image
// writes) for 8-bit matrices without the RMSNorm prologue whose K is split eight ways (o_proj 7.4 vs 7.9 us, down_proj 22.5 vs 25.0 us at six
// rows; with the prologue the variant needs 186 VGPRs and loses: q|k|v 17.8 vs 13.0 us), 128-byte ones otherwise (tools/wq_sweep.py --sweep).
static void rows16_wq_geometry(int bits, int nt, bool norm, int N, int K, int *cseg, int *waves, int *ksplit) {
    if (g_wq_geom) {
        *cseg = g_wq_geom >> 16, *waves = (g_wq_geom >> 8) & 255, *ksplit = g_wq_geom & 255;
        return;
    }
    const int ntiles = (N + 15) / 16, blk128 = 128 * 8 / bits;
    int ks = 1;
    while (ks < 8 && ntiles * ks < 3500 && K / (ks * 2) >= 2 * blk128) ks *= 2;
    int w = ks <= 4 ? 4 : 8;
    if (rows16_wq_lds(bits, 128, w, nt) > 160 * 1024) w = 4, ks = 4;      // gate|up at 4 bits: three 512-byte images per wave
    int cs = 128;
    if (bits == 8 && nt == 1 && !norm && ks == 8 && rows16_wq_lds(bits, 256, w, nt) <= 160 * 1024) cs = 256;
    *cseg = cs, *waves = w, *ksplit = ks;
}

template <int EPI, int BITS, bool NORM>
static int launch_rows16_wq(hipStream_t s, const bf16_t *X, int ldx, const unsigned char *codes, const unsigned char *scales, const float *bias,
                            const bf16_t *normw, float eps, const bf16_t *res, int ldr, bf16_t *C, int ldc, int M, int N, int K) {
    int cseg, waves, ksplit;
    rows16_wq_geometry(BITS, EPI == WQ_SILU_MUL ? 2 : 1, NORM, N, K, &cseg, &waves, &ksplit);
    if (BITS == 8 && cseg == 256)
        return launch_rows16_wq_seg<EPI, 8, 256, NORM>(waves, ksplit, s, X, ldx, codes, scales, bias, normw, eps, res, ldr, C, ldc, M, N, K);
    return launch_rows16_wq_seg<EPI, BITS, 128, NORM>(waves, ksplit, s, X, ldx, codes, scales, bias, normw, eps, res, ldr, C, ldc, M, N, K);
}

static int linear_rows16_wq(const void *x, int ldx, const void *packed, int bits, const float *bias, const void *norm_w, float eps,
                            const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, hipStream_t s) {
    LL_CHECK(x && out, "ll_linear_rows16_wq: null argument");
    LL_CHECK(M >= 1 && M <= 16, "ll_linear_rows16_wq: M=%d rows (1..16)", M);
    LL_CHECK(epi >= WQ_PLAIN && epi <= WQ_SILU_MUL, "ll_linear_rows16_wq: epilogue %d", epi);
    const int rows = epi == WQ_SILU_MUL ? 2 * N : N;
    LL_TRY(wq_check_packed("ll_linear_rows16_wq", packed, bits, rows, K));
    LL_CHECK(N >= 1 && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0, "ll_linear_rows16_wq: ldx must be a multiple of 8 and x 16-byte aligned");
    LL_CHECK(epi != WQ_RESIDUAL || residual, "ll_linear_rows16_wq: residual epilogue without a residual");
    LL_CHECK(!norm_w || ((uintptr_t)norm_w & 15) == 0, "ll_linear_rows16_wq: norm weight must be 16-byte aligned");
    const unsigned char *codes = (const unsigned char *)packed, *scales = codes + (size_t)rows * K / 8 * bits;
    const bf16_t *X = (const bf16_t *)x, *nw = (const bf16_t *)norm_w, *rs = (const bf16_t *)residual;
    bf16_t *C = (bf16_t *)out;
#define LL_WQ_R16(EPI_, B_, NORM_) return launch_rows16_wq<EPI_, B_, NORM_>(s, X, ldx, codes, scales, bias, nw, eps, rs, ldr, C, ldc, M, N, K)
#define LL_WQ_R16_EPI(B_, NORM_)                           \
    do {                                                   \
        if (epi == WQ_PLAIN) LL_WQ_R16(WQ_PLAIN, B_, NORM_);       \
        if (epi == WQ_RESIDUAL) LL_WQ_R16(WQ_RESIDUAL, B_, NORM_); \
        LL_WQ_R16(WQ_SILU_MUL, B_, NORM_);                 \
    } while (0)
    if (bits == 8) {
        if (nw) LL_WQ_R16_EPI(8, true);
        LL_WQ_R16_EPI(8, false);
    }
    if (nw) LL_WQ_R16_EPI(4, true);
    LL_WQ_R16_EPI(4, false);
#undef LL_WQ_R16_EPI
#undef LL_WQ_R16
}

}  // namespace ll

using namespace ll;

extern "C" {

int64_t ll_wq_bytes(int N, int K, int bits) {
    if ((bits != 4 && bits != 8) || N < 1 || K < 32 || K % 32 != 0) return -1;
    return (int64_t)N * K / 8 * bits + (int64_t)N * (K / 32);
}

int ll_wq_quantize_bf16(const void *W, int ldw, int N, int K, int bits, void *packed, void *Wdq, int lddq, void *stream) {
    LL_CHECK(W && (packed || Wdq), "ll_wq_quantize_bf16: null argument");
    LL_CHECK(bits == 4 || bits == 8, "ll_wq_quantize_bf16: bits=%d (4 or 8)", bits);
    LL_CHECK(N >= 1 && K >= 32 && K % 32 == 0, "ll_wq_quantize_bf16: K=%d must be a multiple of 32 (one scale per 32 elements)", K);
    LL_CHECK(ldw % 8 == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)packed & 15) == 0, "ll_wq_quantize_bf16: ldw must be a multiple of 8, W and packed 16-byte aligned");
    LL_CHECK(!Wdq || (lddq % 8 == 0 && ((uintptr_t)Wdq & 15) == 0), "ll_wq_quantize_bf16: lddq must be a multiple of 8, Wdq 16-byte aligned");
    unsigned char *codes = (unsigned char *)packed, *scales = codes ? codes + (size_t)N * K / 8 * bits : nullptr;
    const int64_t total = (int64_t)N * (K / 8);
    const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (bits == 8)
        hipLaunchKernelGGL((wq_quantize_kernel<8>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)W, (int64_t)ldw, N, K, codes, scales,
                           (bf16_t *)Wdq, (int64_t)lddq);
    else
        hipLaunchKernelGGL((wq_quantize_kernel<4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)W, (int64_t)ldw, N, K, codes, scales,
                           (bf16_t *)Wdq, (int64_t)lddq);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_wq_dequantize_bf16(const void *packed, int N, int K, int bits, void *W, int ldw, void *stream) {
    LL_CHECK(W, "ll_wq_dequantize_bf16: null argument");
    LL_TRY(wq_check_packed("ll_wq_dequantize_bf16", packed, bits, N, K));
    LL_CHECK(ldw % 8 == 0 && ((uintptr_t)W & 15) == 0, "ll_wq_dequantize_bf16: ldw must be a multiple of 8, W 16-byte aligned");
    const unsigned char *codes = (const unsigned char *)packed, *scales = codes + (size_t)N * K / 8 * bits;
    const int64_t total = (int64_t)N * (K / 8);
    const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (bits == 8)
        hipLaunchKernelGGL((wq_dequantize_kernel<8>), dim3(grid), dim3(256), 0, (hipStream_t)stream, codes, scales, N, K, (bf16_t *)W, (int64_t)ldw);
    else
        hipLaunchKernelGGL((wq_dequantize_kernel<4>), dim3(grid), dim3(256), 0, (hipStream_t)stream, codes, scales, N, K, (bf16_t *)W, (int64_t)ldw);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_gemv_fused_wq(const void *x, int ldx, const void *packed, int bits, const float *bias, const void *norm_w, float eps,
                     const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream) {
    return gemv_fused_wq(x, ldx, packed, bits, bias, norm_w, eps, residual, ldr, out, ldc, M, N, K, epi, (hipStream_t)stream);
}

int ll_linear_rows16_wq(const void *x, int ldx, const void *packed, int bits, const float *bias, const void *norm_w, float eps,
                        const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream) {
    return linear_rows16_wq(x, ldx, packed, bits, bias, norm_w, eps, residual, ldr, out, ldc, M, N, K, epi, (hipStream_t)stream);
}

#if LL_TUNING
int ll_set_wq_geometry(int cseg, int waves, int ksplit) {
    const int old = g_wq_geom;
    const bool ok = (cseg == 128 || cseg == 256) && (waves == 4 || waves == 8) && ksplit >= 1 && ksplit <= waves && waves % ksplit == 0;
    g_wq_geom = ok ? (cseg << 16 | waves << 8 | ksplit) : 0;
    return old;
}

// Times ll_gemv_fused_wq (kind 0) or ll_linear_rows16_wq (kind 1) on synthetic operands over `nweights` distinct packed matrices
// (defeats the 256 MiB Infinity Cache).
int ll_wq_bench(int kind, int bits, int M, int N, int K, int epi, int norm, int iters, int nweights, float *ms) {
    LL_CHECK(ms && iters > 0 && nweights > 0 && M >= 1 && M <= 16 && (kind == 0 || kind == 1), "bad argument");
    const int rowsW = epi == WQ_SILU_MUL ? 2 * N : N;
    const int64_t pb = ll_wq_bytes(rowsW, K, bits);
    LL_CHECK(pb > 0, "ll_wq_bench: bits=%d (4 or 8), K=%d must be a multiple of 32", bits, K);
    const size_t stride = ((size_t)pb + 255) / 256 * 256, cb = (size_t)rowsW * K / 8 * bits;
    bf16_t *X = nullptr, *C = nullptr, *R = nullptr;
    unsigned char *W = nullptr;
    LL_HIP(hipMalloc(&X, (size_t)16 * K * 2));
    LL_HIP(hipMalloc(&W, (size_t)nweights * stride));
    LL_HIP(hipMalloc(&C, (size_t)16 * N * 2));
    LL_HIP(hipMalloc(&R, (size_t)16 * N * 2));
    LL_HIP(hipMemset(X, 0x11, (size_t)16 * K * 2));
    LL_HIP(hipMemset(R, 0x11, (size_t)16 * N * 2));
    LL_HIP(hipMemset(W, 0x11, (size_t)nweights * stride));
    for (int i = 0; i < nweights; ++i) LL_HIP(hipMemset(W + (size_t)i * stride + cb, 0x7f, (size_t)pb - cb));       // scale bytes: 2^0
    hipStream_t st;
    LL_HIP(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    LL_HIP(hipEventCreate(&e0));
    LL_HIP(hipEventCreate(&e1));
    int rc = LL_OK;
    for (int pass = 0; pass < 2 && rc == LL_OK; ++pass) {
        if (pass == 1) (void)hipEventRecord(e0, st);
        for (int i = 0; i < (pass ? iters : nweights) && rc == LL_OK; ++i) {
            const unsigned char *w = W + (size_t)(i % nweights) * stride;
            rc = kind == 0 ? gemv_fused_wq(X, K, w, bits, nullptr, norm ? X : nullptr, 1e-6f, R, N, C, N, M, N, K, epi, st)
                           : linear_rows16_wq(X, K, w, bits, nullptr, norm ? X : nullptr, 1e-6f, R, N, C, N, M, N, K, epi, st);
        }
    }
    (void)hipEventRecord(e1, st);
    hipError_t he = hipEventSynchronize(e1);
    float t = 0.f;
    (void)hipEventElapsedTime(&t, e0, e1);
    *ms = t / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(st);
    (void)hipFree(X);
    (void)hipFree(W);
    (void)hipFree(C);
    (void)hipFree(R);
    if (rc != LL_OK) return rc;
    LL_HIP(he);
    return LL_OK;
}
#endif

}  // extern "C"
