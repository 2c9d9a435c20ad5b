// Decode-step layer kernels for an untouched HuggingFace Llama-family LLM: the twelve launches
// of one decoder layer at batch <= 4 (RMSNorm, q/k/v GEMV, rotary, KV append, attention, o_proj GEMV, add, RMSNorm,
// gate/up GEMV, SiLU*mul, down GEMV, add) become five:
//   ll_gemv_fused_bf16       x W^T with an optional RMSNorm prologue on x and an epilogue: bias | residual add | SiLU(gate)*up
//   ll_decode_attn_rope_bf16 rotary embedding of q and the new k, KV-cache append, GQA attention over the static cache (llm_attn.hip)
// This file holds the first of the two -- the dense GEMV, its launchers and tuning entries -- and the per-token prologue of the step
// (ll_decode_prologue / ll_suffix_prologue and their dynamic-NTK forms: rotary tables and the causal mask in one launch).
// The arithmetic -- f32 accumulation order, every intermediate bf16 rounding PyTorch's op-by-op evaluation implies --
// is the one of the unfused kernels (gemv_bf16_kernel, rmsnorm/silu_mul in llm_ops.hip),
// so results are bit-identical to them; what goes away is seven launch boundaries and seven HBM/L2 round trips of
// [B, hidden]-sized vectors per layer.
#include "common.h"
#include "gemv_body.h"

namespace ll {

// The dense GEMV: gemv_fused_body (gemv_body.h, shared with the expert kernels of llm_moe.hip) on the rows X + m * ldx.
template <int MROWS, bool NORM, int EPI, bool NT, int XC>
__global__ __launch_bounds__(256) void gemv_fused_kernel(const bf16_t *__restrict__ X, int ldx, const bf16_t *__restrict__ W,
                                                         int ldw, const float *__restrict__ bias,
                                                         const bf16_t *__restrict__ normw, float eps,
                                                         const bf16_t *__restrict__ res, int ldr, bf16_t *__restrict__ C,
                                                         int ldc, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_gemv[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(sm_gemv);   // NORM: [MROWS][K] normalised x
    __shared__ float red[MROWS][4];
    const bf16_t *xr[MROWS], *rr[MROWS];
    bf16_t *cr[MROWS];
    float rs[MROWS];
#pragma unroll
    for (int m = 0; m < MROWS; ++m) {
        xr[m] = X + (int64_t)m * ldx;
        rr[m] = res + (int64_t)m * ldr;
        cr[m] = C + (int64_t)m * ldc;
        rs[m] = 1.f;
    }
    gemv_fused_body<MROWS, NORM, EPI, NT, XC>(xr, W, ldw, bias, normw, eps, rr, cr, rs, N, K, blockIdx.x * 4 + (threadIdx.x >> 6), xs, red);
}

// The same GEMV with the scaled residual epilogue (GEMV_RESIDUAL_SCALED, Granite layout): a kernel of its own, so that the float is an
// argument of this kernel alone and the instantiations above keep their arguments and their code.  No RMSNorm prologue: the Linears that
// carry the residual add (o_proj, down_proj) have none.
template <int MROWS, bool NT>
__global__ __launch_bounds__(256) void gemv_fused_rs_kernel(const bf16_t *__restrict__ X, int ldx, const bf16_t *__restrict__ W, int ldw,
                                                            const float *__restrict__ bias, const bf16_t *__restrict__ res, int ldr,
                                                            bf16_t *__restrict__ C, int ldc, int N, int K, float rscale) {
    __shared__ float red[MROWS][4];
    const bf16_t *xr[MROWS], *rr[MROWS];
    bf16_t *cr[MROWS];
    float rs[MROWS];
#pragma unroll
    for (int m = 0; m < MROWS; ++m) {
        xr[m] = X + (int64_t)m * ldx;
        rr[m] = res + (int64_t)m * ldr;
        cr[m] = C + (int64_t)m * ldc;
        rs[m] = rscale;
    }
    gemv_fused_body<MROWS, false, GEMV_RESIDUAL_SCALED, NT, 2>(xr, W, ldw, bias, nullptr, 0.f, rr, cr, rs, N, K,
                                                                blockIdx.x * 4 + (threadIdx.x >> 6), nullptr, red);
}

// gemv_fused_kernel's prologue-free form (down_proj: no RMSNorm, long K) for ONE token row with x staged in LDS: in the
// generic kernel every wave re-reads its x chunks from L1/L2 next to the weight stream (8 more loads per lane and block,
// 24 in flight); here the workgroup copies x into LDS once, with its first weight loads already in flight, and the stream
// keeps 16 loads per lane.  Same FMA order per output row, so the result is bit-identical.
// RS: empty, or one float = the multiplier of GEMV_RESIDUAL_SCALED (pack_scale, common.h).
template <int EPI, typename... RS>
__global__ __launch_bounds__(256) void gemv_stage_kernel(const bf16_t *__restrict__ X, const bf16_t *__restrict__ W, int ldw,
                                                         const float *__restrict__ bias, const bf16_t *__restrict__ res,
                                                         bf16_t *__restrict__ C, int N, int K, RS... rscale) {
    static_assert(sizeof...(RS) == (EPI == GEMV_RESIDUAL_SCALED ? 1 : 0), "the scale is an argument of the scaled epilogue alone");
    constexpr int R = 2, UNR = LL_GEMV_STAGE_UNR, XCS = 10;       // XCS 16-byte chunks of x per thread: K <= 20480
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_gemvs[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(sm_gemvs);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = blockIdx.x * 4 + (tid >> 6);
    const int n0 = wave * R;
    const bool active = n0 < N;
    const bf16_t *wr[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wr[r] = W + (int64_t)(n0 + r < N ? n0 + r : N - 1) * ldw;
    const int nchunk = K / 8;
    u32x4 xv0[XCS];
#pragma unroll
    for (int c = 0; c < XCS; ++c) {
        const int ch = tid + c * 256;
        xv0[c] = ch < nchunk ? *reinterpret_cast<const u32x4 *>(X + ch * 8) : (u32x4)(0);
    }
    u32x4 wv[UNR][R];
    gemv_load_w<UNR, true>(wv, wr, lane, nchunk, active);
#pragma unroll
    for (int c = 0; c < XCS; ++c) {
        const int ch = tid + c * 256;
        if (ch < nchunk) *reinterpret_cast<u32x4 *>(xs + ch * 8) = xv0[c];
    }
    __syncthreads();
    if (!active) return;
    float acc[1][R] = {{0.f, 0.f}};
    gemv_fma<1, UNR, true>(acc, wv, xs, K, lane, nchunk);
    for (int c0 = lane + 64 * UNR; c0 < nchunk; c0 += 64 * UNR) {
        gemv_load_w<UNR, true>(wv, wr, c0, nchunk, true);
        gemv_fma<1, UNR, true>(acc, wv, xs, K, c0, nchunk);
    }
    float v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = wave_sum(acc[0][r]);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (n0 + r < N) {
                float o = v[r] + (bias ? bias[n0 + r] : 0.f);
                if (EPI == GEMV_RESIDUAL) o = bf16_to_f32(res[n0 + r]) + bfr2(o);
                if (EPI == GEMV_RESIDUAL_SCALED) o = bf16_to_f32(res[n0 + r]) + bfr2(bfr2(o) * pack_scale(rscale...));
                C[n0 + r] = f32_to_bf16(o);
            }
        }
    }
}

// Per-token prologue of the decode step: what Qwen2RotaryEmbedding.forward (freqs = inv_freq * position, cos/sin in f32,
// * attention_scaling, cast to bf16) and create_causal_mask (key j visible iff j <= query position and not padding) compute
// with ~12 small ATen launches, as one.  grid B.  The scaled rope types whose inv_freq / attention_scaling are fixed at construction
// (linear, llama3, yarn) are this kernel with other constants.
__device__ __forceinline__ void prologue_row(const long long *__restrict__ posid, const float *__restrict__ inv_freq, float scaling,
                                             const long long *__restrict__ mask2d, int64_t ms, const long long *__restrict__ pos_ptr,
                                             bf16_t *__restrict__ cos_o, bf16_t *__restrict__ sin_o, unsigned char *__restrict__ mask_o,
                                             int D, int maxlen, int S) {
    // row r = b*S + s: the s-th new position of sequence b (S = 1: a decode step)
    const int r = blockIdx.x, tid = threadIdx.x;
    const int b = r / S, s = r - b * S;
    const int half = D / 2;
    if (tid < half) {
        const float f = inv_freq[tid] * (float)posid[r];
        const bf16_t c = f32_to_bf16(cosf(f) * scaling), sn = f32_to_bf16(sinf(f) * scaling);
        cos_o[(int64_t)r * D + tid] = c;
        cos_o[(int64_t)r * D + tid + half] = c;
        sin_o[(int64_t)r * D + tid] = sn;
        sin_o[(int64_t)r * D + tid + half] = sn;
    }
    const long long p = *pos_ptr + s;
    for (int j = tid; j < maxlen; j += 256) mask_o[(int64_t)r * maxlen + j] = (j <= p && mask2d[b * ms + j] != 0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void decode_prologue_kernel(const long long *__restrict__ posid, const float *__restrict__ inv_freq,
                                                              float scaling, const long long *__restrict__ mask2d, int64_t ms,
                                                              const long long *__restrict__ pos_ptr, bf16_t *__restrict__ cos_o,
                                                              bf16_t *__restrict__ sin_o, unsigned char *__restrict__ mask_o,
                                                              int D, int maxlen, int S) {
    prologue_row(posid, inv_freq, scaling, mask2d, ms, pos_ptr, cos_o, sin_o, mask_o, D, maxlen, S);
}

// Dynamic NTK rope (transformers dynamic_rope_update) without its host read: with L = max(position ids of the call) + 1 the frequencies are
// inv_freq0 (the constructed ones) while L <= max_pos and row L - max_pos - 1 of ``table`` ([table_rows, D/2] f32: HF's own init function at
// sequence lengths max_pos + 1 ...) beyond.  Every workgroup reduces the call's n = gridDim.x position ids itself (n <= 64 at decode, <= 16
// for the suffix: no cross-workgroup traffic), then runs the row exactly as decode_prologue_kernel does.
__global__ __launch_bounds__(256) void decode_prologue_dyn_kernel(const long long *__restrict__ posid, const float *__restrict__ inv_freq0,
                                                                  const float *__restrict__ table, int max_pos, int table_rows,
                                                                  float scaling, const long long *__restrict__ mask2d, int64_t ms,
                                                                  const long long *__restrict__ pos_ptr, bf16_t *__restrict__ cos_o,
                                                                  bf16_t *__restrict__ sin_o, unsigned char *__restrict__ mask_o,
                                                                  int D, int maxlen, int S) {
    __shared__ long long red[256];
    const int tid = threadIdx.x, n = gridDim.x;
    long long m = posid[0];
    for (int i = tid; i < n; i += 256) m = posid[i] > m ? posid[i] : m;
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o && red[tid + o] > red[tid]) red[tid] = red[tid + o];
        __syncthreads();
    }
    const long long L = red[0] + 1;
    const float *inv_freq = inv_freq0;
    if (L > max_pos && table_rows > 0) {
        long long row = L - max_pos - 1;
        if (row > table_rows - 1) row = table_rows - 1;      // a position id past the cache length: stay inside the table
        inv_freq = table + row * (D / 2);
    }
    prologue_row(posid, inv_freq, scaling, mask2d, ms, pos_ptr, cos_o, sin_o, mask_o, D, maxlen, S);
}

static int g_gemv_nt = 1;   // non-temporal weight loads (tools/gemv_fused_sweep.py)
static int g_gemv_stage = 1;   // one-row GEMVs without RMSNorm stage x in LDS (gemv_stage_kernel)

template <int MROWS, bool NORM, int EPI>
static void launch_fused(bool nt, dim3 grid, size_t lds, hipStream_t s, const bf16_t *X, int ldx, const bf16_t *W, int ldw,
                         const float *bias, const bf16_t *normw, float eps, const bf16_t *res, int ldr, bf16_t *C, int ldc, int N,
                         int K) {
#define LL_GF(NT_, XC_) hipLaunchKernelGGL((gemv_fused_kernel<MROWS, NORM, EPI, NT_, XC_>), grid, dim3(256), lds, s, X, ldx, W, ldw, bias, \
                                           normw, eps, res, ldr, C, ldc, N, K)
    if (!NORM || K <= 4096) {
        if (nt) LL_GF(true, 2); else LL_GF(false, 2);
    } else {
        if (nt) LL_GF(true, 4); else LL_GF(false, 4);
    }
#undef LL_GF
}

template <int MROWS>
static int dispatch_fused(bool nt, hipStream_t s, const bf16_t *X, int ldx, const bf16_t *W, int ldw, const float *bias,
                          const bf16_t *normw, float eps, const bf16_t *res, int ldr, bf16_t *C, int ldc, int N, int K, int epi) {
    const bool norm = normw != nullptr;
    const size_t lds = norm ? (size_t)MROWS * K * 2 : 0;
    const dim3 grid(epi == GEMV_SILU_MUL ? cdiv(N, 4) : cdiv(N, 8));
#define LL_FUSED_CASE(NORM_, EPI_)                                                                                          \
    launch_fused<MROWS, NORM_, EPI_>(nt, grid, lds, s, X, ldx, W, ldw, bias, normw, eps, res, ldr, C, ldc, N, K)
    if (norm) {
        if (epi == GEMV_PLAIN) LL_FUSED_CASE(true, GEMV_PLAIN);
        else if (epi == GEMV_RESIDUAL) LL_FUSED_CASE(true, GEMV_RESIDUAL);
        else LL_FUSED_CASE(true, GEMV_SILU_MUL);
    } else {
        if (epi == GEMV_PLAIN) LL_FUSED_CASE(false, GEMV_PLAIN);
        else if (epi == GEMV_RESIDUAL) LL_FUSED_CASE(false, GEMV_RESIDUAL);
        else LL_FUSED_CASE(false, GEMV_SILU_MUL);
    }
#undef LL_FUSED_CASE
    LL_LAUNCH_CHECK();
    return LL_OK;
}

static int gemv_fused(bool nt, const void *x, int ldx, const void *W, int ldw, const float *bias, const void *norm_w, float eps,
                      const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, hipStream_t s) {
    LL_CHECK(x && W && out, "ll_gemv_fused_bf16: null argument");
    LL_CHECK(M >= 1 && M <= 4, "ll_gemv_fused_bf16: M=%d rows (decode shapes only, 1..4)", M);
    LL_CHECK(N >= 1 && K >= 8 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0, "ll_gemv_fused_bf16: K, ldx, ldw must be multiples of 8");
    LL_CHECK(epi >= GEMV_PLAIN && epi <= GEMV_SILU_MUL, "ll_gemv_fused_bf16: epilogue %d", epi);
    LL_CHECK(epi != GEMV_RESIDUAL || residual, "ll_gemv_fused_bf16: residual epilogue without a residual");
    LL_CHECK(!norm_w || (K <= 8192 && (size_t)M * K * 2 <= 65536), "ll_gemv_fused_bf16: RMSNorm prologue needs K <= 8192 and M*K <= 32768");
    const bf16_t *X = (const bf16_t *)x, *Wt = (const bf16_t *)W, *nw = (const bf16_t *)norm_w, *rs = (const bf16_t *)residual;
    bf16_t *C = (bf16_t *)out;
    if (g_gemv_stage && nt && M == 1 && !nw && epi != GEMV_SILU_MUL && K >= 8192 && K <= 20480) {
        // one row, no RMSNorm, long K (down_proj): x staged in LDS once per workgroup (down_proj 25.0 -> 23.8 us; for the short K of
        // o_proj the extra barrier costs more than the eight x loads per block it removes: 6.4 -> 7.0 us)
        const dim3 grid(cdiv(N, 8));
        if (epi == GEMV_RESIDUAL)
            hipLaunchKernelGGL((gemv_stage_kernel<GEMV_RESIDUAL>), grid, dim3(256), (size_t)K * 2, s, X, Wt, ldw, bias, rs, C, N, K);
        else
            hipLaunchKernelGGL((gemv_stage_kernel<GEMV_PLAIN>), grid, dim3(256), (size_t)K * 2, s, X, Wt, ldw, bias, rs, C, N, K);
        LL_LAUNCH_CHECK();
        return LL_OK;
    }
    switch (M) {
        case 1: return dispatch_fused<1>(nt, s, X, ldx, Wt, ldw, bias, nw, eps, rs, ldr, C, ldc, N, K, epi);
        case 2: return dispatch_fused<2>(nt, s, X, ldx, Wt, ldw, bias, nw, eps, rs, ldr, C, ldc, N, K, epi);
        case 3: return dispatch_fused<3>(nt, s, X, ldx, Wt, ldw, bias, nw, eps, rs, ldr, C, ldc, N, K, epi);
        default: return dispatch_fused<4>(nt, s, X, ldx, Wt, ldw, bias, nw, eps, rs, ldr, C, ldc, N, K, epi);
    }
}

// ll_gemv_fused_rs_bf16: the shapes and the kernel choice of gemv_fused at LL_GEMV_RESIDUAL without a norm, on the scaled instantiations
static int gemv_fused_rs(bool nt, const void *x, int ldx, const void *W, int ldw, const float *bias, const void *residual, int ldr, void *out,
                         int ldc, int M, int N, int K, float rscale, hipStream_t s) {
    LL_CHECK(x && W && out && residual, "ll_gemv_fused_rs_bf16: null argument");
    LL_CHECK(M >= 1 && M <= 4, "ll_gemv_fused_rs_bf16: M=%d rows (decode shapes only, 1..4)", M);
    LL_CHECK(N >= 1 && K >= 8 && K % 8 == 0 && ldx % 8 == 0 && ldw % 8 == 0, "ll_gemv_fused_rs_bf16: K, ldx, ldw must be multiples of 8");
    LL_CHECK(scale_ok(rscale), "ll_gemv_fused_rs_bf16: residual_scale must be finite and non-zero");
    const bf16_t *X = (const bf16_t *)x, *Wt = (const bf16_t *)W, *rs = (const bf16_t *)residual;
    bf16_t *C = (bf16_t *)out;
    const dim3 grid(cdiv(N, 8));
    if (g_gemv_stage && nt && M == 1 && K >= 8192 && K <= 20480) {
        hipLaunchKernelGGL((gemv_stage_kernel<GEMV_RESIDUAL_SCALED, float>), grid, dim3(256), (size_t)K * 2, s, X, Wt, ldw, bias, rs, C, N, K, rscale);
        LL_LAUNCH_CHECK();
        return LL_OK;
    }
#define LL_GRS(M_)                                                                                                                          \
    do {                                                                                                                                    \
        if (nt) hipLaunchKernelGGL((gemv_fused_rs_kernel<M_, true>), grid, dim3(256), 0, s, X, ldx, Wt, ldw, bias, rs, ldr, C, ldc, N, K, rscale); \
        else hipLaunchKernelGGL((gemv_fused_rs_kernel<M_, false>), grid, dim3(256), 0, s, X, ldx, Wt, ldw, bias, rs, ldr, C, ldc, N, K, rscale);  \
    } while (0)
    switch (M) {
        case 1: LL_GRS(1); break;
        case 2: LL_GRS(2); break;
        case 3: LL_GRS(3); break;
        default: LL_GRS(4); break;
    }
#undef LL_GRS
    LL_LAUNCH_CHECK();
    return LL_OK;
}

}  // namespace ll

using namespace ll;

extern "C" {

int ll_gemv_fused_bf16(const void *x, int ldx, const void *W, int ldw, const float *bias, const void *norm_w, float eps,
                       const void *residual, int ldr, void *out, int ldc, int M, int N, int K, int epi, void *stream) {
    return gemv_fused(g_gemv_nt != 0, x, ldx, W, ldw, bias, norm_w, eps, residual, ldr, out, ldc, M, N, K, epi, (hipStream_t)stream);
}

int ll_gemv_fused_rs_bf16(const void *x, int ldx, const void *W, int ldw, const float *bias, const void *residual, int ldr, void *out, int ldc,
                          int M, int N, int K, float residual_scale, void *stream) {
    return gemv_fused_rs(g_gemv_nt != 0, x, ldx, W, ldw, bias, residual, ldr, out, ldc, M, N, K, residual_scale, (hipStream_t)stream);
}

int ll_decode_prologue(const int64_t *position_ids, const float *inv_freq, float attention_scaling, const int64_t *mask2d,
                       int64_t mask_stride, const int64_t *pos, void *cos, void *sin, void *mask_out, int B, int D, int maxlen,
                       void *stream) {
    LL_CHECK(position_ids && inv_freq && mask2d && pos && cos && sin && mask_out, "ll_decode_prologue: null argument");
    LL_CHECK(B >= 1 && D >= 2 && D % 2 == 0 && D <= 512 && maxlen >= 1, "ll_decode_prologue: unsupported shape");
    hipLaunchKernelGGL(decode_prologue_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, (const long long *)position_ids, inv_freq,
                       attention_scaling, (const long long *)mask2d, mask_stride, (const long long *)pos, (bf16_t *)cos, (bf16_t *)sin,
                       (unsigned char *)mask_out, D, maxlen, 1);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_suffix_prologue(const int64_t *position_ids, const float *inv_freq, float attention_scaling, const int64_t *mask2d,
                       int64_t mask_stride, const int64_t *pos, void *cos, void *sin, void *mask_out, int B, int S, int D, int maxlen,
                       void *stream) {
    LL_CHECK(position_ids && inv_freq && mask2d && pos && cos && sin && mask_out, "ll_suffix_prologue: null argument");
    LL_CHECK(B >= 1 && S >= 1 && D >= 2 && D % 2 == 0 && D <= 512 && maxlen >= 1, "ll_suffix_prologue: unsupported shape");
    hipLaunchKernelGGL(decode_prologue_kernel, dim3(B * S), dim3(256), 0, (hipStream_t)stream, (const long long *)position_ids, inv_freq,
                       attention_scaling, (const long long *)mask2d, mask_stride, (const long long *)pos, (bf16_t *)cos, (bf16_t *)sin,
                       (unsigned char *)mask_out, D, maxlen, S);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

static int prologue_dyn(const char *who, const int64_t *position_ids, const float *inv_freq0, const float *table, int max_pos, int table_rows,
                        float attention_scaling, const int64_t *mask2d, int64_t mask_stride, const int64_t *pos, void *cos, void *sin,
                        void *mask_out, int B, int S, int D, int maxlen, void *stream) {
    LL_CHECK(position_ids && inv_freq0 && mask2d && pos && cos && sin && mask_out, "%s: null argument", who);
    LL_CHECK(B >= 1 && S >= 1 && D >= 2 && D % 2 == 0 && D <= 512 && maxlen >= 1 && max_pos >= 1 && table_rows >= 0, "%s: unsupported shape", who);
    // every sequence length that a cache of maxlen slots can reach needs its row
    LL_CHECK(maxlen <= max_pos || (table && table_rows >= maxlen - max_pos),
             "%s: table_rows < maxlen - max_pos (the frequency table does not cover the cache length)", who);
    hipLaunchKernelGGL(decode_prologue_dyn_kernel, dim3(B * S), dim3(256), 0, (hipStream_t)stream, (const long long *)position_ids, inv_freq0,
                       table, max_pos, table ? table_rows : 0, attention_scaling, (const long long *)mask2d, mask_stride,
                       (const long long *)pos, (bf16_t *)cos, (bf16_t *)sin, (unsigned char *)mask_out, D, maxlen, S);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_decode_prologue_dyn(const int64_t *position_ids, const float *inv_freq0, const float *table, int max_pos, int table_rows,
                           float attention_scaling, const int64_t *mask2d, int64_t mask_stride, const int64_t *pos, void *cos, void *sin,
                           void *mask_out, int B, int D, int maxlen, void *stream) {
    return prologue_dyn("ll_decode_prologue_dyn", position_ids, inv_freq0, table, max_pos, table_rows, attention_scaling, mask2d, mask_stride,
                        pos, cos, sin, mask_out, B, 1, D, maxlen, stream);
}

int ll_suffix_prologue_dyn(const int64_t *position_ids, const float *inv_freq0, const float *table, int max_pos, int table_rows,
                           float attention_scaling, const int64_t *mask2d, int64_t mask_stride, const int64_t *pos, void *cos, void *sin,
                           void *mask_out, int B, int S, int D, int maxlen, void *stream) {
    return prologue_dyn("ll_suffix_prologue_dyn", position_ids, inv_freq0, table, max_pos, table_rows, attention_scaling, mask2d, mask_stride,
                        pos, cos, sin, mask_out, B, S, D, maxlen, stream);
}

// Times ll_gemv_fused_bf16 on synthetic operands, cycling through `nweights` distinct weight matrices (defeats the
// 256 MiB Infinity Cache).  norm != 0 adds the RMSNorm prologue; nt selects non-temporal weight loads.
#if LL_TUNING
int ll_gemv_fused_bench(int M, int N, int K, int epi, int norm, int nt, int iters, int nweights, float *ms) {
    LL_CHECK(ms && iters > 0 && nweights > 0 && M >= 1 && M <= 4, "bad argument");
    const int rowsW = epi == GEMV_SILU_MUL ? 2 * N : N;
    bf16_t *X = nullptr, *W = nullptr, *C = nullptr, *R = nullptr, *NW = nullptr;
    LL_HIP(hipMalloc(&X, (size_t)4 * K * 2));
    LL_HIP(hipMalloc(&NW, (size_t)K * 2));
    LL_HIP(hipMalloc(&W, (size_t)nweights * rowsW * K * 2));
    LL_HIP(hipMalloc(&C, (size_t)4 * N * 2));
    LL_HIP(hipMalloc(&R, (size_t)4 * N * 2));
    LL_HIP(hipMemset(X, 0x11, (size_t)4 * K * 2));
    LL_HIP(hipMemset(NW, 0x11, (size_t)K * 2));
    LL_HIP(hipMemset(R, 0x11, (size_t)4 * N * 2));
    LL_HIP(hipMemset(W, 0x11, (size_t)nweights * rowsW * K * 2));
    hipStream_t st;
    LL_HIP(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    LL_HIP(hipEventCreate(&e0));
    LL_HIP(hipEventCreate(&e1));
    int rc = LL_OK;
    for (int pass = 0; pass < 2 && rc == LL_OK; ++pass) {
        if (pass == 1) (void)hipEventRecord(e0, st);
        for (int i = 0; i < (pass ? iters : nweights) && rc == LL_OK; ++i)
            rc = gemv_fused(nt != 0, X, K, W + (size_t)(i % nweights) * rowsW * K, K, nullptr, norm ? NW : nullptr, 1e-6f, R, N, C, N, M,
                            N, K, epi, st);
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
    (void)hipFree(NW);
    (void)hipFree(W);
    (void)hipFree(C);
    (void)hipFree(R);
    if (rc != LL_OK) return rc;
    LL_HIP(he);
    return LL_OK;
}
#endif

#if LL_TUNING
int ll_set_gemv_stage(int on) {
    const int old = g_gemv_stage;
    g_gemv_stage = on ? 1 : 0;
    return old;
}
#endif

#if LL_TUNING
int ll_set_gemv_nt(int on) {
    const int old = g_gemv_nt;
    g_gemv_nt = on ? 1 : 0;
    return old;
}
#endif

}  // extern "C"
