// Decode-step kernels of a sparse mixture-of-experts MLP block (Qwen3-MoE layout: Qwen3MoeTopKRouter + Qwen3MoeExperts of transformers
// modeling_qwen3_moe.py) for 1..64 token rows.  The router logits are the dense Linear (ll_gemv_fused_bf16 / ll_linear_rows16_bf16 with the
// post-attention RMSNorm as prologue); what is new here:
//   ll_moe_route_bf16    one workgroup: per row the top_k largest logits (descending, ties to the lower index), softmax over ALL experts in
//                        f32, renormalisation over the selected, and the grouping of the (row, slot) pairs by expert for the kernels below
//   ll_moe_experts_bf16  three launches -- gate|up + SiLU*mul, down * routing weight, slot sum + residual -- over the ACTIVE experts only:
//                        blockIdx.y is a slot of the active-expert list (min(E, M*top_k) slots; slots past the list exit at once), and the
//                        workgroups of one expert take all of its token rows in passes of up to 4 rows over their weight tile, so an expert's
//                        matrices come from HBM once per launch (later passes re-read the tile from L2), not once per (row, slot) pair.
//   ll_moe_route_f32 / ll_moe_experts_ex_bf16  the Mixtral and Qwen2-MoE layouts as compile-time variants of the same kernels: routing weights
//                        stored and applied in f32 (the down launch then stores the unweighted projection and the slot sum multiplies), and a
//                        sigmoid-gated shared expert added in the slot sum; with both options off the entry IS ll_moe_experts_bf16.
// The GEMV arithmetic is gemv_fused_body (gemv_body.h), the body of the dense ll_gemv_fused_bf16: a row that is alone on its expert is
// rounded bit for bit like the dense kernel on that expert's matrices.  No floating-point atomics; every sum has a fixed order.
// Workspace (private layout), for P = M * top_k pairs and A = min(E, P) active-expert slots:
//   int32 [0] = number of active experts, [1 .. A+1] = start of each active expert's run in `pair` (ascending expert id; entry nact = P),
//   then pair[P] = pair ids m * top_k + j sorted by (expert, pair id); 16-byte aligned behind it act[P][I] bf16 (SiLU(gate)*up per pair)
//   and z[P][H] bf16 (routing weight times the rounded down projection per pair).
#include "common.h"
#include "gemv_body.h"

namespace ll {

static inline int64_t moe_int_bytes(int M, int E, int top_k) {
    const int64_t P = (int64_t)M * top_k, A = E < P ? E : P;
    return (1 + (A + 1) + P + 3) / 4 * 16;      // int32 entries, rounded up to 16 bytes
}

static inline bool moe_route_shape_ok(int M, int E, int top_k) { return M >= 1 && M <= 64 && E >= 1 && E <= 256 && top_k >= 1 && top_k <= 8 && top_k <= E; }

// (value, index) argmax step: the larger value, equal values by the lower index
__device__ __forceinline__ void route_better(float &bv, int &bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

// One workgroup of 4 waves; wave w routes rows w, w + 4, ...; a lane holds logits lane, lane + 64, lane + 128, lane + 192 of its row.
// WF32 (ll_moe_route_f32, the Mixtral router): the weights leave as the f32 values themselves, never rounded to bf16.
template <bool WF32 = false>
__global__ __launch_bounds__(256) void moe_route_kernel(const bf16_t *__restrict__ logits, int ld, int M, int E, int top_k, int norm_topk,
                                                        int *__restrict__ idx, void *__restrict__ wout, int *__restrict__ ws) {
    __shared__ int sidx[512];      // expert of pair m * top_k + j
    __shared__ int cnt[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int m = wave; m < M; m += 4) {
        float v[4];
        bool live[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = lane + 64 * c;
            live[c] = i < E;
            const float x = live[c] ? bf16_to_f32(logits[(int64_t)m * ld + i]) : -INFINITY;
            v[c] = x == x ? x : -INFINITY;      // a NaN logit ranks last
        }
        float sel[8];
        int seli[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sel[j] = 0.f;
            seli[j] = 0;
            if (j < top_k) {
                float bv = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (live[c]) route_better(bv, bi, v[c], lane + 64 * c);
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float ov = __shfl_xor(bv, off, 64);
                    const int oi = __shfl_xor(bi, off, 64);
                    route_better(bv, bi, ov, oi);
                }
                // top_k <= E: at least one live logit is left, so bi is an expert id
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (bi == lane + 64 * c) live[c] = false;
                sel[j] = bv;
                seli[j] = bi;
            }
        }
        const float mx = sel[0];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (lane + 64 * c < E) s += expf(v[c] - mx);
        s = wave_sum(s);
        float p[8], ps = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p[j] = j < top_k ? expf(sel[j] - mx) / s : 0.f;
            if (j < top_k) ps += p[j];
        }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < top_k) {
                    const int e = min(max(seli[j], 0), E - 1);
                    idx[m * top_k + j] = e;
                    sidx[m * top_k + j] = e;
                    const float wj = norm_topk ? p[j] / ps : p[j];
                    if (WF32) reinterpret_cast<float *>(wout)[m * top_k + j] = wj;
                    else reinterpret_cast<bf16_t *>(wout)[m * top_k + j] = f32_to_bf16(wj);
                }
        }
    }
    __syncthreads();
    // grouping: thread e counts the pairs of expert e, finds its place among the active experts and lists its pairs in pair-id order
    const int P = M * top_k, A = E < P ? E : P;
    int c = 0;
    if (tid < E)
        for (int q = 0; q < P; ++q) c += sidx[q] == tid;
    cnt[tid] = tid < E ? c : 0;
    __syncthreads();
    int start = 0, slot = 0, nact = 0;
    for (int e = 0; e < E; ++e) {
        const int ce = cnt[e];
        if (e < tid) {
            start += ce;
            slot += ce > 0;
        }
        nact += ce > 0;
    }
    int *seg = ws + 1, *pair = ws + 1 + (A + 1);
    if (tid == 0) {
        ws[0] = nact;
        seg[nact] = P;
    }
    if (tid < E && c > 0) {
        seg[slot] = start;
        int o = start;
        for (int q = 0; q < P; ++q)
            if (sidx[q] == tid) pair[o++] = q;
    }
}

// The grouping of one active-expert slot, clamped so that whatever the workspace holds every address below stays inside the operands.
struct MoeGroup {
    int e, beg, end;
};
__device__ __forceinline__ bool moe_group(const int *__restrict__ ws, const int *__restrict__ idx, int s, int P, int A, int E, MoeGroup &g) {
    const int nact = min(ws[0], A);
    if (s >= nact) return false;
    const int *seg = ws + 1, *pair = ws + 1 + (A + 1);
    g.beg = min(max(seg[s], 0), P);
    g.end = min(max(seg[s + 1], g.beg), P);
    if (g.beg >= g.end) return false;
    const int p0 = min(max(pair[g.beg], 0), P - 1);
    g.e = min(max(idx[p0], 0), E - 1);
    return true;
}

// One pass of R (1..4) token rows of the group over this workgroup's weight tile.  GU: gate|up (RMSNorm prologue on the rows of x the pairs
// belong to, SiLU*mul epilogue -> act[pair]); otherwise down (x = act[pair], epilogue bf16(bf16(acc) * w[pair]) -> z[pair]; YRAW: the plain
// epilogue bf16(acc) -> z[pair], the routing weight is not read -- ll_moe_experts_ex_bf16 with f32 weights applies it in the slot sum).
template <int R, bool GU, bool NT, int XC, bool YRAW = false>
__device__ __forceinline__ void moe_pass(const int *__restrict__ pair, int P, int top_k, const bf16_t *__restrict__ X, int ldx,
                                         const bf16_t *__restrict__ normw, float eps, const bf16_t *__restrict__ W,
                                         const bf16_t *__restrict__ rw, bf16_t *__restrict__ outp, int N, int K, bf16_t *xs, float (*red)[4]) {
    const bf16_t *xr[R], *rr[R];
    bf16_t *cr[R];
    float rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = min(max(pair[r], 0), P - 1);
        xr[r] = GU ? X + (int64_t)(q / top_k) * ldx : X + (int64_t)q * ldx;
        rr[r] = nullptr;
        cr[r] = outp + (int64_t)q * N;
        rs[r] = (GU || YRAW) ? 1.f : bf16_to_f32(rw[q]);
    }
    gemv_fused_body<R, GU, GU ? GEMV_SILU_MUL : (YRAW ? GEMV_PLAIN : GEMV_SCALE), NT, XC>(xr, W, K, nullptr, normw, eps, rr, cr, rs, N, K,
                                                                   blockIdx.x * 4 + (threadIdx.x >> 6), xs, red);
}

// grid (weight-row blocks, active-expert slots).  A token row selects top_k DIFFERENT experts, so a group holds at most M rows: MAXR =
// min(M, 4) bounds the rows of a pass at compile time and MULTI (M > 4) says whether a group can need more than one pass -- the one-row
// decode step thus runs the one-row body at the dense GEMV's register count, not at the four-row body's.  Earlier passes of a group load
// the tile with ordinary loads (it is read again), the last pass with non-temporal ones (the dense GEMV's choice for a matrix that is
// streamed once).
template <bool GU, int XC, int MAXR, bool MULTI, bool YRAW = false>
__global__ __launch_bounds__(256) void moe_expert_kernel(const bf16_t *__restrict__ X, int ldx, const bf16_t *__restrict__ normw, float eps,
                                                         const int *__restrict__ idx, const bf16_t *__restrict__ rw,
                                                         const bf16_t *__restrict__ Wall, const int *__restrict__ ws,
                                                         bf16_t *__restrict__ outp, int P, int A, int E, int top_k, int N, int K,
                                                         int64_t wstride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_moe[];
    bf16_t *xs = reinterpret_cast<bf16_t *>(sm_moe);     // GU: [MAXR][K] normalised rows
    __shared__ float red[MAXR][4];
    MoeGroup g;
    if (!moe_group(ws, idx, blockIdx.y, P, A, E, g)) return;      // uniform over the workgroup
    const bf16_t *W = Wall + (int64_t)g.e * wstride;
    const int *pair = ws + 1 + (A + 1);
    if (!MULTI) g.end = min(g.end, g.beg + MAXR);       // cannot happen with a routing of ll_moe_route_bf16; keeps a foreign workspace in bounds
    for (int p0 = g.beg; p0 < g.end; p0 += 4) {
        if (MULTI && p0 > g.beg) __syncthreads();      // xs / red of the previous pass are free
        const int n = g.end - p0;
#define LL_MOE_PASS(R_, NT_) moe_pass<R_, GU, NT_, XC, YRAW>(pair + p0, P, top_k, X, ldx, normw, eps, W, rw, outp, N, K, xs, red)
        if (MULTI && n > 4) LL_MOE_PASS(4, false);
        else if (MAXR >= 4 && n >= 4) LL_MOE_PASS(4, true);
        else if (MAXR >= 3 && n == 3) LL_MOE_PASS(3, true);
        else if (MAXR >= 2 && n == 2) LL_MOE_PASS(2, true);
        else LL_MOE_PASS(1, true);
#undef LL_MOE_PASS
    }
}

template <bool GU, int XC, bool YRAW = false>
static void launch_moe_expert(int M, dim3 grid, size_t lds, hipStream_t s, const bf16_t *X, int ldx, const bf16_t *normw, float eps,
                              const int *idx, const bf16_t *rw, const bf16_t *Wall, const int *ws, bf16_t *outp, int P, int A, int E, int top_k,
                              int N, int K, int64_t wstride) {
#define LL_MOE_K(MAXR_, MULTI_) hipLaunchKernelGGL((moe_expert_kernel<GU, XC, MAXR_, MULTI_, YRAW>), grid, dim3(256), lds, s, X, ldx, normw, eps, idx, rw, \
                                                   Wall, ws, outp, P, A, E, top_k, N, K, wstride)
    if (M == 1) LL_MOE_K(1, false);
    else if (M == 2) LL_MOE_K(2, false);
    else if (M == 3) LL_MOE_K(3, false);
    else if (M == 4) LL_MOE_K(4, false);
    else LL_MOE_K(4, true);
#undef LL_MOE_K
}

// out[m] = bf16( residual[m] + bf16( sum_j z[m * top_k + j] ) ), the sum in f32 in slot order.  grid M.
__global__ __launch_bounds__(256) void moe_combine_kernel(const bf16_t *__restrict__ z, const bf16_t *__restrict__ res, int ldr,
                                                          bf16_t *__restrict__ out, int ldo, int top_k, int H) {
    const int m = blockIdx.x;
    for (int ch = threadIdx.x; ch < H / 8; ch += 256) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < top_k; ++j) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(z + ((int64_t)m * top_k + j) * H + ch * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[2 * t] += __uint_as_float(v[t] << 16);
                acc[2 * t + 1] += __uint_as_float(v[t] & 0xffff0000u);
            }
        }
        const u32x4 r = *reinterpret_cast<const u32x4 *>(res + (int64_t)m * ldr + ch * 8);
        u32x4 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float a = __uint_as_float(r[t] << 16) + bfr2(acc[2 * t]), b = __uint_as_float(r[t] & 0xffff0000u) + bfr2(acc[2 * t + 1]);
            o[t] = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
        }
        *reinterpret_cast<u32x4 *>(out + (int64_t)m * ldo + ch * 8) = o;
    }
}

// The slot sum of ll_moe_experts_ex_bf16.  grid M.
//   WF32:   z holds the unweighted y; the sum is sum_j f32(w[m, j] * float(y_mj)) with w in f32 -- every product rounded to f32 on its own
//           (no fused multiply-add), added in slot order, ONE rounding to bf16;  otherwise the sum of moe_combine_kernel.
//   SHARED: out = bf16(res + bf16(float(bf16(sum)) + float(bf16(float(sig) * float(s))))),  sig = bf16(1 / (1 + exp(-float(g[m * ldg])))).
template <bool WF32, bool SHARED>
__global__ __launch_bounds__(256) void moe_combine_ex_kernel(const bf16_t *__restrict__ z, const void *__restrict__ wv,
                                                             const bf16_t *__restrict__ res, int ldr, const bf16_t *__restrict__ sh, int lds,
                                                             const bf16_t *__restrict__ gate, int ldg, bf16_t *__restrict__ out, int ldo,
                                                             int top_k, int H) {
    const int m = blockIdx.x;
    float wj[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wj[j] = (WF32 && j < top_k) ? reinterpret_cast<const float *>(wv)[m * top_k + j] : 0.f;
    float sig = 0.f;
    if (SHARED) sig = bfr2(1.f / (1.f + expf(-bf16_to_f32(gate[(int64_t)m * ldg]))));
    for (int ch = threadIdx.x; ch < H / 8; ch += 256) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < top_k) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(z + ((int64_t)m * top_k + j) * H + ch * 8);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const float a = __uint_as_float(v[t] << 16), b = __uint_as_float(v[t] & 0xffff0000u);
                    if (WF32) {
                        acc[2 * t] = __fadd_rn(acc[2 * t], __fmul_rn(wj[j], a));
                        acc[2 * t + 1] = __fadd_rn(acc[2 * t + 1], __fmul_rn(wj[j], b));
                    } else {
                        acc[2 * t] += a;
                        acc[2 * t + 1] += b;
                    }
                }
            }
        }
        if (SHARED) {
            const u32x4 sv = *reinterpret_cast<const u32x4 *>(sh + (int64_t)m * lds + ch * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[2 * t] = __fadd_rn(bfr2(acc[2 * t]), bfr2(__fmul_rn(sig, __uint_as_float(sv[t] << 16))));
                acc[2 * t + 1] = __fadd_rn(bfr2(acc[2 * t + 1]), bfr2(__fmul_rn(sig, __uint_as_float(sv[t] & 0xffff0000u))));
            }
        }
        const u32x4 r = *reinterpret_cast<const u32x4 *>(res + (int64_t)m * ldr + ch * 8);
        u32x4 o;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float a = __uint_as_float(r[t] << 16) + bfr2(acc[2 * t]), b = __uint_as_float(r[t] & 0xffff0000u) + bfr2(acc[2 * t + 1]);
            o[t] = (uint32_t)f32_to_bf16(a) | ((uint32_t)f32_to_bf16(b) << 16);
        }
        *reinterpret_cast<u32x4 *>(out + (int64_t)m * ldo + ch * 8) = o;
    }
}

}  // namespace ll

using namespace ll;

extern "C" {

int64_t ll_moe_workspace_bytes(int M, int E, int top_k, int H, int I) {
    if (!moe_route_shape_ok(M, E, top_k) || H < 8 || I < 8) return -1;
    return moe_int_bytes(M, E, top_k) + (int64_t)M * top_k * ((int64_t)I + H) * 2;
}

int ll_moe_route_f32(const void *logits, int ld, int M, int E, int top_k, int norm_topk, int32_t *idx, float *w, void *workspace,
                     int64_t workspace_bytes, void *stream) {
    LL_CHECK(logits && idx && w && workspace, "ll_moe_route_f32: null argument");
    LL_CHECK(moe_route_shape_ok(M, E, top_k), "ll_moe_route_f32: M=%d rows (1..64), E=%d experts (<= 256), top_k=%d (1..min(E, 8))", M, E, top_k);
    LL_CHECK(ld >= E, "ll_moe_route_f32: row stride %d < E", ld);
    LL_CHECK(workspace_bytes >= moe_int_bytes(M, E, top_k) && ((uintptr_t)workspace & 15) == 0,
             "ll_moe_route_f32: workspace too small or not 16-byte aligned (ll_moe_workspace_bytes)");
    hipLaunchKernelGGL(moe_route_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)logits, ld, M, E, top_k, norm_topk,
                       (int *)idx, (void *)w, (int *)workspace);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_moe_route_bf16(const void *logits, int ld, int M, int E, int top_k, int norm_topk, int32_t *idx, void *w, void *workspace,
                      int64_t workspace_bytes, void *stream) {
    LL_CHECK(logits && idx && w && workspace, "ll_moe_route_bf16: null argument");
    LL_CHECK(moe_route_shape_ok(M, E, top_k), "ll_moe_route_bf16: M=%d rows (1..64), E=%d experts (<= 256), top_k=%d (1..min(E, 8))", M, E, top_k);
    LL_CHECK(ld >= E, "ll_moe_route_bf16: row stride %d < E", ld);
    LL_CHECK(workspace_bytes >= moe_int_bytes(M, E, top_k) && ((uintptr_t)workspace & 15) == 0,
             "ll_moe_route_bf16: workspace too small or not 16-byte aligned (ll_moe_workspace_bytes)");
    hipLaunchKernelGGL(moe_route_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)logits, ld, M, E, top_k, norm_topk,
                       (int *)idx, w, (int *)workspace);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

// The bounds ll_moe_experts_bf16 and ll_moe_experts_ex_bf16 share; `fn` names the entry in the message.
static int moe_experts_check(const char *fn, const void *x, int ldx, const void *norm_w, float eps, const int32_t *idx, const void *w, const void *Wgu,
                             const void *Wd, const void *residual, int ldr, const void *out, int ldo, int M, int E, int top_k, int H, int I,
                             const void *workspace, int64_t workspace_bytes) {
    LL_CHECK(x && norm_w && idx && w && Wgu && Wd && residual && out && workspace, "%s: null argument", fn);
    LL_CHECK(moe_route_shape_ok(M, E, top_k), "%s: M=%d rows (1..64), E=%d experts (<= 256), top_k=%d (1..min(E, 8))", fn, M, E, top_k);
    LL_CHECK(H >= 8 && H % 8 == 0 && H <= 8192 && I >= 8 && I % 8 == 0 && I <= 32768, "%s: H=%d (multiple of 8 up to 8192), I=%d (multiple of 8 up to 32768)", fn, H, I);
    LL_CHECK(ldx >= H && ldr >= H && ldo >= H && ldx % 8 == 0 && ldr % 8 == 0 && ldo % 8 == 0, "%s: row strides must be multiples of 8, at least H", fn);
    LL_CHECK(eps > 0.f, "%s: eps must be positive", fn);
    LL_CHECK(workspace_bytes >= ll_moe_workspace_bytes(M, E, top_k, H, I) && ((uintptr_t)workspace & 15) == 0,
             "%s: workspace too small or not 16-byte aligned (ll_moe_workspace_bytes)", fn);
    LL_CHECK((((uintptr_t)x | (uintptr_t)norm_w | (uintptr_t)Wgu | (uintptr_t)Wd | (uintptr_t)residual | (uintptr_t)out) & 15) == 0,
             "%s: operands must be 16-byte aligned", fn);
    return LL_OK;
}

// The gate|up launch of both entries: act[pair] = SiLU(gate) * up over the active experts (the routing weights are not read).
static void moe_launch_gate_up(int M, hipStream_t s, const void *x, int ldx, const void *norm_w, float eps, const int32_t *idx, const void *Wgu,
                               const int *ws, bf16_t *act, int E, int top_k, int H, int I) {
    const int P = M * top_k, A = E < P ? E : P;
    const size_t lds = (size_t)(M < 4 ? M : 4) * H * 2;
    const dim3 g1(cdiv(I, 4), A);
    if (H <= 4096)
        launch_moe_expert<true, 2>(M, g1, lds, s, (const bf16_t *)x, ldx, (const bf16_t *)norm_w, eps, (const int *)idx, nullptr,
                                   (const bf16_t *)Wgu, ws, act, P, A, E, top_k, I, H, (int64_t)2 * I * H);
    else
        launch_moe_expert<true, 4>(M, g1, lds, s, (const bf16_t *)x, ldx, (const bf16_t *)norm_w, eps, (const int *)idx, nullptr,
                                   (const bf16_t *)Wgu, ws, act, P, A, E, top_k, I, H, (int64_t)2 * I * H);
}

int ll_moe_experts_bf16(const void *x, int ldx, const void *norm_w, float eps, const int32_t *idx, const void *w, const void *Wgu,
                        const void *Wd, const void *residual, int ldr, void *out, int ldo, int M, int E, int top_k, int H, int I,
                        void *workspace, int64_t workspace_bytes, void *stream) {
    LL_TRY(moe_experts_check("ll_moe_experts_bf16", x, ldx, norm_w, eps, idx, w, Wgu, Wd, residual, ldr, out, ldo, M, E, top_k, H, I, workspace,
                             workspace_bytes));
    const int P = M * top_k, A = E < P ? E : P;
    const int *ws = (const int *)workspace;
    bf16_t *act = (bf16_t *)((char *)workspace + moe_int_bytes(M, E, top_k));
    bf16_t *z = act + (int64_t)P * I;
    hipStream_t s = (hipStream_t)stream;
    moe_launch_gate_up(M, s, x, ldx, norm_w, eps, idx, Wgu, ws, act, E, top_k, H, I);
    LL_LAUNCH_CHECK();
    launch_moe_expert<false, 2>(M, dim3(cdiv(H, 8), A), 0, s, (const bf16_t *)act, I, nullptr, 0.f, (const int *)idx, (const bf16_t *)w,
                                (const bf16_t *)Wd, ws, z, P, A, E, top_k, H, I, (int64_t)H * I);
    LL_LAUNCH_CHECK();
    hipLaunchKernelGGL(moe_combine_kernel, dim3(M), dim3(256), 0, s, (const bf16_t *)z, (const bf16_t *)residual, ldr, (bf16_t *)out, ldo, top_k, H);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_moe_experts_ex_bf16(const void *x, int ldx, const void *norm_w, float eps, const int32_t *idx, const void *w, int w_f32, const void *Wgu,
                           const void *Wd, const void *residual, int ldr, const void *shared, int lds, const void *gate, int ldg, void *out,
                           int ldo, int M, int E, int top_k, int H, int I, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!w_f32 && !shared)      // both options off: the call it extends, bit for bit
        return ll_moe_experts_bf16(x, ldx, norm_w, eps, idx, w, Wgu, Wd, residual, ldr, out, ldo, M, E, top_k, H, I, workspace, workspace_bytes,
                                   stream);
    LL_TRY(moe_experts_check("ll_moe_experts_ex_bf16", x, ldx, norm_w, eps, idx, w, Wgu, Wd, residual, ldr, out, ldo, M, E, top_k, H, I, workspace,
                             workspace_bytes));
    LL_CHECK(!w_f32 || ((uintptr_t)w & 3) == 0, "ll_moe_experts_ex_bf16: f32 routing weights must be 4-byte aligned");
    LL_CHECK(!shared || (gate && lds >= H && lds % 8 == 0 && ldg >= 1 && ((uintptr_t)shared & 15) == 0 && ((uintptr_t)gate & 1) == 0),
             "ll_moe_experts_ex_bf16: the shared expert's rows need a gate column, a row stride that is a multiple of 8, at least H, and 16-byte alignment");
    const int P = M * top_k, A = E < P ? E : P;
    const int *ws = (const int *)workspace;
    bf16_t *act = (bf16_t *)((char *)workspace + moe_int_bytes(M, E, top_k));
    bf16_t *z = act + (int64_t)P * I;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g2(cdiv(H, 8), A);
    moe_launch_gate_up(M, s, x, ldx, norm_w, eps, idx, Wgu, ws, act, E, top_k, H, I);
    LL_LAUNCH_CHECK();
    if (w_f32)      // the unweighted projection: the f32 weights are read by the slot sum only
        launch_moe_expert<false, 2, true>(M, g2, 0, s, (const bf16_t *)act, I, nullptr, 0.f, (const int *)idx, nullptr, (const bf16_t *)Wd, ws, z, P, A,
                                          E, top_k, H, I, (int64_t)H * I);
    else
        launch_moe_expert<false, 2>(M, g2, 0, s, (const bf16_t *)act, I, nullptr, 0.f, (const int *)idx, (const bf16_t *)w, (const bf16_t *)Wd, ws, z, P,
                                    A, E, top_k, H, I, (int64_t)H * I);
    LL_LAUNCH_CHECK();
#define LL_MOE_COMBINE(WF32_, SHARED_) hipLaunchKernelGGL((moe_combine_ex_kernel<WF32_, SHARED_>), dim3(M), dim3(256), 0, s, (const bf16_t *)z, w, \
                                                          (const bf16_t *)residual, ldr, (const bf16_t *)shared, lds, (const bf16_t *)gate, ldg,  \
                                                          (bf16_t *)out, ldo, top_k, H)
    if (w_f32 && shared) LL_MOE_COMBINE(true, true);
    else if (w_f32) LL_MOE_COMBINE(true, false);
    else LL_MOE_COMBINE(false, true);
#undef LL_MOE_COMBINE
    LL_LAUNCH_CHECK();
    return LL_OK;
}

}  // extern "C"
