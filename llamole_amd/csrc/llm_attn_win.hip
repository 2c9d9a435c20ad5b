// Key-split decode attention for sliding-window layers: ll_decode_attn_rope_win_bf16 and ll_suffix_attn_rope_win_bf16 -- the two launches of
// llm_attn_split.hip with HF's sliding_window_causal_mask_function applied in the kernel: key j is visible to query row (b, s) iff its mask byte
// is set and j > *pos + s - window.  The geometry depends on the shapes and the window only, not on the cache length:
//   attn_win_partial_kernel  grid (nrw, head groups, rows), nrw = min(ceil(maxlen / 512), ceil((window + S - 2) / 512) + 1): workgroup x takes the
//       ABSOLUTE range first + x of SPLIT_RANGE = 512 keys, first = max(0, *pos - window + 1) / 512 computed on the device from *pos.  The S
//       windows of a call span at most window + S - 1 consecutive slots, which touch at most nrw ranges aligned to multiples of 512; a range
//       index past the end of the cache writes the empty partial (-inf, 0).  Mask bytes below the window are not read.
//   attn_win_combine_kernel  grid (nh, rows): attn_split_combine_kernel with thread a owning absolute range a (the ranges outside
//       [first, first + nrw) weigh nothing), so every sum has the operands, the lanes and the order it has in attn_split_combine_kernel over all
//       ceil(maxlen / 512) ranges: the result is bit for bit that of the split entries called with the window cut out of their mask.
// The body of the partial kernel is attn_split_partial_kernel's (llm_attn_split.hip: access pattern, lane roles, the new rows rotated in the launch
// and stored by exactly one workgroup, no atomics); what differs is the range a workgroup takes, the window in the visibility of a key and the
// workspace indexed by x: ml [rows][nh][nrw][2] f32 (m, l), acc [rows][nh][nrw][D] f32.
#include "common.h"
#include "attn_decode.h"
#include "attn_split.h"
#include "head_pair.h"

namespace ll {

// first absolute range a window layer's call can see: the range of slot max(0, p0 - window + 1), the lowest slot visible to query row s = 0
__device__ __forceinline__ long long win_first_range(long long p0, int window) {
    const long long low = p0 - (long long)window + 1;
    return (low > 0 ? low : 0) / SPLIT_RANGE;
}

static inline int win_ranges(int S, int maxlen, int window) {
    const int64_t nr = cdiv(maxlen, SPLIT_RANGE), nw = ((int64_t)window + S - 2 + SPLIT_RANGE - 1) / SPLIT_RANGE + 1;
    return (int)(nw < nr ? nw : nr);
}

template <int D, int GT>
__global__ __launch_bounds__(ATTN_THREADS) void attn_win_partial_kernel(const bf16_t *__restrict__ qkv, int64_t ld_qkv,
                                                                    const bf16_t *__restrict__ cs, const bf16_t *__restrict__ sn, int64_t cs0,
                                                                    bf16_t *K, bf16_t *V, const long long *__restrict__ pos_ptr,
                                                                    const unsigned char *__restrict__ mask, int64_t ms0,
                                                                    float *__restrict__ ml, float *__restrict__ accw, int S, int nh, int nkv,
                                                                    int maxlen, float scale, const bf16_t *__restrict__ qnw,
                                                                    const bf16_t *__restrict__ knw, float eps, int window) {
    constexpr int LPR = AttnGeom<D>::LPR, NI = AttnGeom<D>::NI, half = D / 2;
    // tiles whose loads a lane has in flight at once: the whole range, except for seven heads of 128 (one tile: 255 VGPRs spilled otherwise)
    constexpr int TF = (GT == 7 && D == 128) ? 1 : SPLIT_TILES, NL = TF * NI;
    __shared__ __attribute__((aligned(16))) float qs[GT * D];                 // rotated queries, f32 of their bf16 values
    __shared__ __attribute__((aligned(16))) bf16_t kn[SPLIT_MAX_S * D];      // rotated new keys of this range (bf16), row t at t * D
    __shared__ __attribute__((aligned(16))) bf16_t vn[SPLIT_MAX_S * D];      // new values
    __shared__ float sc[GT * SPLIT_RANGE];                                     // scores -> exponentials
    __shared__ float part[GT * ATTN_WAVES * D];                                // per-wave partial outputs
    __shared__ float red[2 * GT * ATTN_WAVES];
    const int x = blockIdx.x, hg = blockIdx.y, r = blockIdx.z;
    const int nr = gridDim.x;                                                  // nrw: ranges per (head, row) in the workspace
    const int b = r / S, s = r - b * S;
    const int G = nh / nkv, h0 = hg * GT, kvh = h0 / G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p0 = *pos_ptr;
    const long long rho = win_first_range(p0, window) + x;                    // the absolute range of this workgroup
    const int64_t wbase = ((int64_t)r * nh + h0) * nr + x;                     // + g * nr per head
    if (rho * SPLIT_RANGE >= (long long)maxlen) {                              // past the end of the cache: the empty partial
        if (tid < GT) {
            ml[(wbase + (int64_t)tid * nr) * 2] = -INFINITY;
            ml[(wbase + (int64_t)tid * nr) * 2 + 1] = 0.f;
        }
        return;
    }
    const int j0 = (int)rho * SPLIT_RANGE, j1 = min(j0 + SPLIT_RANGE, maxlen);
    const unsigned char *mrow = mask + (int64_t)r * ms0;
    // visible: the mask byte AND inside the window of this row (slot p0 + s): j > p0 + s - window
    const unsigned char mk = j0 + tid < j1 && (long long)(j0 + tid) > p0 + s - (long long)window ? mrow[j0 + tid] : (unsigned char)0;
    // the new rows t whose slot p0 + t lies in this range: t in [tlo, thi)
    const long long lo = p0 > (long long)j0 ? p0 : (long long)j0, hi = p0 + S < (long long)j1 ? p0 + S : (long long)j1;
    const int tlo = lo < hi ? (int)(lo - p0) : 0, thi = lo < hi ? (int)(hi - p0) : 0;
    const bool writer = h0 % G == 0 && s >= tlo && s < thi;                    // this workgroup stores the row of slot p0 + s
    const int any = __syncthreads_or(mk != 0);
    if (!any && !writer) {
        if (tid < GT) {
            ml[(wbase + (int64_t)tid * nr) * 2] = -INFINITY;
            ml[(wbase + (int64_t)tid * nr) * 2 + 1] = 0.f;
        }
        return;
    }
    bf16_t *Kb = K + ((int64_t)b * nkv + kvh) * maxlen * D;
    bf16_t *Vb = V + ((int64_t)b * nkv + kvh) * maxlen * D;
    const int c = lane % LPR, rr = lane / LPR;
    // slot of (tile, instruction i, lane); a slot is fetched from the cache iff it lies in the range and is none of the new rows
    auto fetch = [&](int j) { return j < j1 && !((long long)j >= lo && (long long)j < hi); };
    au32x4 kk[NL];
    auto load_rows = [&](au32x4 (&xr)[NL], const bf16_t *base, int jt) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int j = attn_key<D>(jt + (i / NI) * 256, wave, i % NI, lane);
            xr[i] = fetch(j) ? *reinterpret_cast<const au32x4 *>(base + (int64_t)j * D + c * 8) : (au32x4)(0);
        }
    };
    load_rows(kk, Kb, j0);
    // ---- roles 0..GT-1: the query heads of the group (row r's angles); GT + t: new row t (its own angles), for the slots of this range
    for (int role = wave; role < GT + S; role += ATTN_WAVES) {
        float x1, x2, y1, y2;
        if (role < GT) {
            const bf16_t *src = qkv + (int64_t)r * ld_qkv + (h0 + role) * D;
            if (qnw) head_pair<D, true>(src, qnw, eps, lane, x1, x2);
            if (lane < half) {
                if (!qnw) head_pair<D, false>(src, qnw, eps, lane, x1, x2);
                rope_pair<D>(x1, x2, cs + (int64_t)r * cs0, sn + (int64_t)r * cs0, lane, y1, y2);
                qs[role * D + lane] = bfr2(y1);
                qs[role * D + lane + half] = bfr2(y2);
            }
        } else {
            const int t = role - GT;
            if (t < tlo || t >= thi) continue;
            const int rt = b * S + t;
            const bf16_t *src = qkv + (int64_t)rt * ld_qkv + (nh + kvh) * D;
            if (knw) head_pair<D, true>(src, knw, eps, lane, x1, x2);
            if (lane < half) {
                if (!knw) head_pair<D, false>(src, knw, eps, lane, x1, x2);
                rope_pair<D>(x1, x2, cs + (int64_t)rt * cs0, sn + (int64_t)rt * cs0, lane, y1, y2);
                const bf16_t k1 = f32_to_bf16(y1), k2 = f32_to_bf16(y2);
                kn[t * D + lane] = k1;
                kn[t * D + lane + half] = k2;
                const bf16_t *vsrc = qkv + (int64_t)rt * ld_qkv + (nh + nkv + kvh) * D;
                const uint32_t v2 = *reinterpret_cast<const uint32_t *>(vsrc + lane * 2);
                *reinterpret_cast<uint32_t *>(vn + t * D + lane * 2) = v2;
                if (writer && t == s) {
                    const long long p = p0 + t;
                    Kb[p * D + lane] = k1;
                    Kb[p * D + lane + half] = k2;
                    *reinterpret_cast<uint32_t *>(Vb + p * D + lane * 2) = v2;
                }
            }
        }
    }
    __syncthreads();
    if (!any) {      // the writer of a row nobody sees in this range
        if (tid < GT) {
            ml[(wbase + (int64_t)tid * nr) * 2] = -INFINITY;
            ml[(wbase + (int64_t)tid * nr) * 2 + 1] = 0.f;
        }
        return;
    }
    // ---- scores
    {
        float q[GT][8];
#pragma unroll
        for (int g = 0; g < GT; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) q[g][e] = qs[g * D + c * 8 + e];
#pragma unroll 1
        for (int jt = j0; jt < j0 + SPLIT_RANGE; jt += TF * 256) {
            if (jt != j0) load_rows(kk, Kb, jt);
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int j = attn_key<D>(jt + (i / NI) * 256, wave, i % NI, lane);
                if ((long long)j >= lo && (long long)j < hi) kk[i] = *reinterpret_cast<const au32x4 *>(kn + (int)(j - p0) * D + c * 8);
#pragma unroll
                for (int g = 0; g < GT; ++g) {
                    const float d = attn_row_sum<LPR>(attn_dot8(q[g], kk[i]));
                    if (c == 0 && j < j1) sc[g * SPLIT_RANGE + (j - j0)] = d * scale;
                }
            }
        }
    }
    __syncthreads();
    // the values are requested behind the barrier (the key registers are free) and arrive under the softmax statistics
    au32x4 vv[NL];
    load_rows(vv, Vb, j0);
    // ---- softmax statistics of the range: thread tid owns key j0 + tid
    float sg[GT];
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        sg[g] = mk != 0 ? sc[g * SPLIT_RANGE + tid] : -INFINITY;      // a select: a masked key's score may be NaN
        const float mx = wave_max(sg[g]);
        if (lane == 0) red[g * ATTN_WAVES + wave] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GT; ++g) {
        float mx = red[g * ATTN_WAVES];
#pragma unroll
        for (int w = 1; w < ATTN_WAVES; ++w) mx = fmaxf(mx, red[g * ATTN_WAVES + w]);
        const float e = mk != 0 ? expf(sg[g] - mx) : 0.f;           // mx is finite: the range has a visible key
        sc[g * SPLIT_RANGE + tid] = e;
        const float sum = wave_sum(e);
        if (lane == 0) red[(GT + g) * ATTN_WAVES + wave] = sum;
    }
    __syncthreads();
    if (tid < GT) {
        float den = red[(GT + tid) * ATTN_WAVES];
        for (int w = 1; w < ATTN_WAVES; ++w) den += red[(GT + tid) * ATTN_WAVES + w];
        float mx = red[tid * ATTN_WAVES];
        for (int w = 1; w < ATTN_WAVES; ++w) mx = fmaxf(mx, red[tid * ATTN_WAVES + w]);
        ml[(wbase + (int64_t)tid * nr) * 2] = mx;
        ml[(wbase + (int64_t)tid * nr) * 2 + 1] = den;
    }
    // ---- un-normalised P V: lane (rr, c) accumulates columns 8c..8c+7 over the rows it sees, for every head of the group
    float acc[GT][8];
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
#pragma unroll 1
    for (int jt = j0; jt < j0 + SPLIT_RANGE; jt += TF * 256) {
        if (jt != j0) load_rows(vv, Vb, jt);
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int j = attn_key<D>(jt + (i / NI) * 256, wave, i % NI, lane);
            float pj[GT];
            bool zero = true;
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                pj[g] = j < j1 ? sc[g * SPLIT_RANGE + (j - j0)] : 0.f;
                zero = zero && pj[g] == 0.f;
            }
            if ((long long)j >= lo && (long long)j < hi) vv[i] = *reinterpret_cast<const au32x4 *>(vn + (int)(j - p0) * D + c * 8);
            if (zero) vv[i] = (au32x4)(0);                             // masked rows may hold anything (NaN from padded positions)
#pragma unroll
            for (int g = 0; g < GT; ++g) attn_axpy8(acc[g], pj[g], vv[i]);
        }
    }
    // the RPI row groups of a wave are combined across lanes (xor LPR, 2 LPR, ...), the waves through LDS
    attn_fold_rows<D, GT>(acc);
    if (rr == 0) {
#pragma unroll
        for (int g = 0; g < GT; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) part[(g * ATTN_WAVES + wave) * D + c * 8 + e] = acc[g][e];
    }
    __syncthreads();
    for (int idx = tid; idx < GT * D; idx += ATTN_THREADS) {
        const int g = idx / D, d = idx - g * D;
        float o = 0.f;
#pragma unroll
        for (int w = 0; w < ATTN_WAVES; ++w) o += part[(g * ATTN_WAVES + w) * D + d];
        accw[(wbase + (int64_t)g * nr) * D + d] = o;
    }
}

// grid (nh, rows), COMBINE_THREADS threads: attn_split_combine_kernel over the nrw ranges first .. first + nrw - 1 of the workspace.  Thread a
// owns ABSOLUTE range a (its statistics sit at x = a - first) and thread (k, d) sums the absolute ranges a = k, k + NS, ... of column d in
// rising order, as attn_split_combine_kernel does over all ranges of the cache; the ranges that are not in the workspace would weigh 0 there.
template <int D>
__global__ __launch_bounds__(COMBINE_THREADS) void attn_win_combine_kernel(const float *__restrict__ ml, const float *__restrict__ accw,
                                                                       bf16_t *__restrict__ out, const long long *__restrict__ pos_ptr, int nh,
                                                                       int nrw, int window) {
    constexpr int NS = COMBINE_THREADS / D, NW = COMBINE_THREADS / 64;
    __shared__ float w[SPLIT_MAX_RANGES];
    __shared__ float red[2 * NW];
    __shared__ float part[NS * D];
    const int h = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = ((int64_t)r * nh + h) * nrw;
    const long long first = win_first_range(*pos_ptr, window);
    const long long xo = (long long)tid - first;                       // this thread's range in the workspace
    const bool own = xo >= 0 && xo < nrw;
    const float m = own ? ml[(base + xo) * 2] : -INFINITY;
    const float l = own ? ml[(base + xo) * 2 + 1] : 0.f;
    const float mx = wave_max(m);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    float M = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) M = fmaxf(M, red[i]);
    const float wr = m == -INFINITY ? 0.f : expf(m - M);             // a range without a visible key weighs nothing (no -inf - -inf)
    if (own) w[xo] = wr;
    const float wl = wave_sum(wr == 0.f ? 0.f : wr * l);
    if (lane == 0) red[NW + wave] = wl;
    __syncthreads();
    float L = red[NW];
#pragma unroll
    for (int i = 1; i < NW; ++i) L += red[NW + i];
    const int k = tid / D, d = tid - k * D;
    float o = 0.f;
    // the first x whose absolute range first + x is congruent to k modulo NS
    const int x0 = (int)(((long long)k - first % NS + NS) % NS);
    for (int xg = x0; xg < nrw; xg += NS) {
        const float wg = w[xg];
        const float a = wg != 0.f ? accw[(base + xg) * D + d] : 0.f;  // nothing was written for an empty range
        o = fmaf(wg, a, o);
    }
    part[k * D + d] = o;
    __syncthreads();
    if (tid < D) {
        float t = part[tid];
#pragma unroll
        for (int i = 1; i < NS; ++i) t += part[i * D + tid];
        out[((int64_t)r * nh + h) * D + tid] = f32_to_bf16(L > 0.f ? t * (1.f / L) : 0.f);     // no visible key at all: zeros
    }
}

static inline int64_t win_workspace_bytes(int B, int S, int nh, int maxlen, int D, int window) {
    return (int64_t)B * S * nh * win_ranges(S, maxlen, window) * (D + 2) * 4;
}

static int attn_win(const char *who, const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs0, void *Kc, void *Vc,
                    const int64_t *pos, const void *mask, int64_t ms0, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                    const void *q_norm_w, const void *k_norm_w, float eps, int window, void *workspace, int64_t workspace_bytes, void *stream) {
    LL_CHECK(qkv && cos && sin && Kc && Vc && pos && mask && out && workspace, "%s: null argument", who);
    LL_CHECK((q_norm_w != nullptr) == (k_norm_w != nullptr), "%s: only one of q_norm_w / k_norm_w", who);
    LL_CHECK(!q_norm_w || eps > 0.f, "%s: eps must be positive", who);
    LL_CHECK(split_shape_ok(B, S, nh, nkv, maxlen, D) && ld_qkv % 8 == 0, "%s: unsupported shape", who);
    LL_CHECK(window >= 1, "%s: window=%d is not positive", who, window);
    LL_CHECK(workspace_bytes >= win_workspace_bytes(B, S, nh, maxlen, D, window) && (uintptr_t)workspace % 16 == 0,
             "%s: the workspace is smaller than ll_attn_win_workspace_bytes or not 16-byte aligned", who);
    const int nrw = win_ranges(S, maxlen, window), rows = B * S, GT = split_group(nh, nkv);
    float *ml = (float *)workspace, *accw = ml + (int64_t)rows * nh * nrw * 2;
    dim3 grid(nrw, nh / GT, rows);
#define LL_WIN(D_, G_)                                                                                                                 \
    hipLaunchKernelGGL((attn_win_partial_kernel<D_, G_>), grid, dim3(ATTN_THREADS), 0, (hipStream_t)stream, (const bf16_t *)qkv, ld_qkv, \
                       (const bf16_t *)cos, (const bf16_t *)sin, cs0, (bf16_t *)Kc, (bf16_t *)Vc, (const long long *)pos,              \
                       (const unsigned char *)mask, ms0, ml, accw, S, nh, nkv, maxlen, scale, (const bf16_t *)q_norm_w,               \
                       (const bf16_t *)k_norm_w, eps, window)
    if (D == 128) {
        if (GT == 1) LL_WIN(128, 1); else if (GT == 2) LL_WIN(128, 2); else if (GT == 4) LL_WIN(128, 4); else LL_WIN(128, 7);
    } else {
        if (GT == 1) LL_WIN(64, 1); else if (GT == 2) LL_WIN(64, 2); else if (GT == 4) LL_WIN(64, 4); else LL_WIN(64, 7);
    }
#undef LL_WIN
    LL_LAUNCH_CHECK();
    if (D == 128)
        hipLaunchKernelGGL((attn_win_combine_kernel<128>), dim3(nh, rows), dim3(COMBINE_THREADS), 0, (hipStream_t)stream, ml, accw,
                           (bf16_t *)out, (const long long *)pos, nh, nrw, window);
    else
        hipLaunchKernelGGL((attn_win_combine_kernel<64>), dim3(nh, rows), dim3(COMBINE_THREADS), 0, (hipStream_t)stream, ml, accw,
                           (bf16_t *)out, (const long long *)pos, nh, nrw, window);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

}  // namespace ll

using namespace ll;

extern "C" {

int64_t ll_attn_win_workspace_bytes(int B, int S, int nh, int nkv, int maxlen, int D, int window) {
    if (!split_shape_ok(B, S, nh, nkv, maxlen, D) || window < 1) return -1;
    return win_workspace_bytes(B, S, nh, maxlen, D, window);
}

int ll_decode_attn_rope_win_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc, void *Vc,
                                 const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh, int nkv, int maxlen,
                                 int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps, int window, void *workspace,
                                 int64_t workspace_bytes, void *stream) {
    LL_CHECK(B <= 64, "ll_decode_attn_rope_win_bf16: unsupported shape (B=%d > 64)", B);
    return attn_win("ll_decode_attn_rope_win_bf16", qkv, ld_qkv, cos, sin, cs_stride, Kc, Vc, pos, mask, mask_stride, out, B, 1, nh, nkv,
                    maxlen, D, scale, q_norm_w, k_norm_w, eps, window, workspace, workspace_bytes, stream);
}

int ll_suffix_attn_rope_win_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                                 const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                                 const void *q_norm_w, const void *k_norm_w, float eps, int window, void *workspace, int64_t workspace_bytes,
                                 void *stream) {
    return attn_win("ll_suffix_attn_rope_win_bf16", qkv, ld_qkv, cos, sin, D, Kc, Vc, pos, mask, maxlen, out, B, S, nh, nkv, maxlen, D,
                    scale, q_norm_w, k_norm_w, eps, window, workspace, workspace_bytes, stream);
}

}  // extern "C"
