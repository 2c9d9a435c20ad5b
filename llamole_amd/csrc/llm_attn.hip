// The one-workgroup decode attention over a static KV cache of up to ATTN_MAX_KEYS slots (longer caches: llm_attn_split.hip):
//   ll_decode_attn_bf16               plain GQA attention of S query rows (decode_attn_bf16_kernel)
//   ll_decode_attn_rope_[qkn_]bf16    rotary embedding of q and the new k, KV-cache append and attention for ONE new position per sequence, one
//                                     launch: decode_attn_rope_kernel per query head, decode_attn_rope_gqa_kernel per KV head from 17 sequences on
//   ll_suffix_attn_rope_[qkn_]bf16    the same for S consecutive new positions (suffix_attn_rope_kernel)
// The arithmetic -- f32 accumulation order, every intermediate bf16 rounding PyTorch's op-by-op evaluation implies -- is the one of the unfused
// kernels (rope / kv_append in llm_ops.hip, then decode_attn_bf16_kernel), so the per-head kernels are bit-identical to them.  Every head row is
// rotated by head_row_rotated (head_pair.h); the per-head body is attn_decode.h's.
#include "common.h"
#include "attn_decode.h"
#include "head_pair.h"

namespace ll {

// Decode attention over a static KV cache (GQA): one workgroup per (query head, batch*query position).
//   scores_j = q . K[j] * scale for keys with mask[b,0,s,j] true; softmax in f32; out = sum_j p_j V[j].
// Replaces repeat_kv (two full-cache copies) + SDPA + mask fills of the HF sdpa path at decode.  D in {64, 128}.
template <int D>
__global__ __launch_bounds__(ATTN_THREADS) void decode_attn_bf16_kernel(const bf16_t *__restrict__ q, const bf16_t *__restrict__ K,
                                                               const bf16_t *__restrict__ V, const unsigned char *__restrict__ mask,
                                                               bf16_t *__restrict__ out, int nh, int nkv, int S, int maxlen,
                                                               float scale, int64_t qs0, int64_t qs1, int64_t qs2,
                                                               int64_t ms0, int64_t ms2) {
    extern __shared__ __attribute__((aligned(16))) float sm_attn[];
    float *qs = sm_attn;                 // [D]     query in f32 (16-B aligned LDS broadcast reads)
    float *part = qs + D;                // [waves][rows per load][D] partial outputs = ATTN_PART_FLOATS for either D
    float *sc = part + ATTN_PART_FLOATS; // [maxlen] scores -> probabilities
    __shared__ float red[2 * ATTN_WAVES];
    const int h = blockIdx.x, bs = blockIdx.y;
    const int b = bs / S, s = bs - b * S;
    const int kvh = h / (nh / nkv);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16_t *Kb = K + ((int64_t)b * nkv + kvh) * maxlen * D;
    const bf16_t *Vb = V + ((int64_t)b * nkv + kvh) * maxlen * D;
    const unsigned char *mrow = mask + b * ms0 + s * ms2;
    AttnTile0<D> t0;
    attn_prefetch<D>(t0, Kb, Vb, mrow, maxlen, tid, lane, wave);
    if (tid < D) qs[tid] = bf16_to_f32(q[b * qs0 + h * qs1 + s * qs2 + tid]);
    __syncthreads();
    attn_finish<D, false>(t0, qs, part, sc, red, Kb, Vb, mrow, maxlen, -1, nullptr, nullptr, scale,
                          out + (((int64_t)b * S + s) * nh + h) * D, tid, lane, wave);
}

// Rotary embedding + KV append + GQA decode attention for ONE new position per sequence.
// grid (nh, B).  qkv row b = [q: nh*D | k: nkv*D | v: nkv*D] (output of the fused q/k/v GEMV).  The new key / value of
// the head's KV group is rotated in LDS and used from there; the first query head of each group also stores it to the
// cache at *pos.  Nobody reads cache slot *pos in this launch, so there is no cross-workgroup dependency.
// QKN: every q head row and the k head row pass head_pair's RMSNorm (weights qnw / knw, one eps) before the rotation; v does not.
template <int D, bool QKN>
__global__ __launch_bounds__(ATTN_THREADS) void decode_attn_rope_kernel(const bf16_t *__restrict__ qkv, int64_t ld_qkv,
                                                               const bf16_t *__restrict__ cs, const bf16_t *__restrict__ sn,
                                                               int64_t cs0, bf16_t *__restrict__ K, bf16_t *__restrict__ V,
                                                               const long long *__restrict__ pos_ptr,
                                                               const unsigned char *__restrict__ mask, int64_t ms0,
                                                               bf16_t *__restrict__ out, int nh, int nkv, int maxlen, float scale,
                                                               const bf16_t *__restrict__ qnw, const bf16_t *__restrict__ knw, float eps) {
    extern __shared__ __attribute__((aligned(16))) float sm_attn2[];
    float *qs = sm_attn2;                 // [D]     rotated query, f32 of its bf16 value
    float *part = qs + D;                 // [waves][rows per load][D] partial outputs = ATTN_PART_FLOATS for either D
    bf16_t *kn = reinterpret_cast<bf16_t *>(part + ATTN_PART_FLOATS);    // [D] rotated new key (bf16)
    bf16_t *vn = kn + D;                  // [D] new value
    float *sc = reinterpret_cast<float *>(vn + D);           // [maxlen] scores -> probabilities
    __shared__ float red[2 * ATTN_WAVES];
    const int h = blockIdx.x, b = blockIdx.y;
    const int group = nh / nkv, kvh = h / group;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p = *pos_ptr;
    const bool pvalid = p >= 0 && p < maxlen;
    const bf16_t *row = qkv + b * ld_qkv;
    const bf16_t *c = cs + b * cs0, *sv = sn + b * cs0;
    constexpr int half = D / 2;
    bf16_t *Kb = K + ((int64_t)b * nkv + kvh) * maxlen * D;
    bf16_t *Vb = V + ((int64_t)b * nkv + kvh) * maxlen * D;
    const unsigned char *mrow = mask + b * ms0;
    AttnTile0<D> t0;      // first 256 keys / values / mask bytes: requested before the rotary arithmetic
    attn_prefetch<D>(t0, Kb, Vb, mrow, maxlen, tid, lane, wave);
    float y1, y2;
    if (wave == 0) {
        if (head_row_rotated<D>(row + h * D, qnw, QKN, eps, c, sv, lane, y1, y2)) {
            qs[lane] = bfr2(y1);
            qs[lane + half] = bfr2(y2);
        }
    } else if (wave == 1) {
        if (head_row_rotated<D>(row + (nh + kvh) * D, knw, QKN, eps, c, sv, lane, y1, y2)) {
            const bf16_t k1 = f32_to_bf16(y1), k2 = f32_to_bf16(y2);
            kn[lane] = k1;
            kn[lane + half] = k2;
            if (pvalid && h % group == 0) {
                Kb[p * D + lane] = k1;
                Kb[p * D + lane + half] = k2;
            }
        }
    } else if (wave == 2) {
        if (lane < half) {
            const bf16_t *src = row + (nh + nkv + kvh) * D;
            const uint32_t v2 = *reinterpret_cast<const uint32_t *>(src + lane * 2);
            *reinterpret_cast<uint32_t *>(vn + lane * 2) = v2;
            if (pvalid && h % group == 0) *reinterpret_cast<uint32_t *>(Vb + p * D + lane * 2) = v2;
        }
    }
    __syncthreads();
    attn_finish<D, true>(t0, qs, part, sc, red, Kb, Vb, mrow, maxlen, pvalid ? p : -1, kn, vn, scale,
                         out + ((int64_t)b * nh + h) * D, tid, lane, wave);
}

// The same for S consecutive NEW positions of every sequence (the query-token forward on top of the decode's cache,
// modeling_llamole.py:641-646: <design_start> + 8 body tokens at cache slots *pos .. *pos + S - 1).  grid (nh, B*S), row r = b*S + s.
// Query row s attends to the cache up to slot *pos + s, i.e. also to the keys of rows 0..s of THIS launch: the workgroup rotates and
// stores those rows of its KV head itself before it reads them (every workgroup of the sequence that needs a row writes the same bits,
// so nobody waits for anybody), then runs the plain cache attention of decode_attn_bf16_kernel -- bit for bit what rope_bf16_kernel +
// kv_append_bf16_kernel + decode_attn_bf16_kernel compute in three launches.  QKN as in decode_attn_rope_kernel: the same head_row_rotated on
// every q and k row, so a key written here is bitwise the key the decode kernels write, whichever workgroup writes it.
template <int D, bool QKN>
__global__ __launch_bounds__(ATTN_THREADS) void suffix_attn_rope_kernel(const bf16_t *__restrict__ qkv, int64_t ld_qkv,
                                                               const bf16_t *__restrict__ cs, const bf16_t *__restrict__ sn, bf16_t *K,
                                                               bf16_t *V, const long long *__restrict__ pos_ptr,
                                                               const unsigned char *__restrict__ mask, bf16_t *__restrict__ out, int nh,
                                                               int nkv, int S, int maxlen, float scale, const bf16_t *__restrict__ qnw,
                                                               const bf16_t *__restrict__ knw, float eps) {
    extern __shared__ __attribute__((aligned(16))) float sm_attn3[];
    float *qs = sm_attn3;                 // [D]  rotated query, f32 of its bf16 value
    float *part = qs + D;                 // ATTN_PART_FLOATS
    float *sc = part + ATTN_PART_FLOATS;  // [maxlen]
    __shared__ float red[2 * ATTN_WAVES];
    const int h = blockIdx.x, r = blockIdx.y;
    const int b = r / S, s = r - b * S;
    const int group = nh / nkv, kvh = h / group;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p0 = *pos_ptr;
    constexpr int half = D / 2;
    bf16_t *Kb = K + ((int64_t)b * nkv + kvh) * maxlen * D;
    bf16_t *Vb = V + ((int64_t)b * nkv + kvh) * maxlen * D;
    const unsigned char *mrow = mask + (int64_t)r * maxlen;
    float y1, y2;
    if (wave == ATTN_WAVES - 1) {
        if (head_row_rotated<D>(qkv + (int64_t)r * ld_qkv + h * D, qnw, QKN, eps, cs + (int64_t)r * D, sn + (int64_t)r * D, lane, y1, y2)) {
            qs[lane] = bfr2(y1);
            qs[lane + half] = bfr2(y2);
        }
    }
    for (int t = wave; t <= s; t += ATTN_WAVES) {
        const long long p = p0 + t;
        if (p < 0 || p >= maxlen || (!QKN && lane >= half)) continue;      // QKN: uniform over the wave (all lanes take part in the norm); else the lanes without a pair leave here
        const int rt = b * S + t;
        if (!head_row_rotated<D>(qkv + (int64_t)rt * ld_qkv + (nh + kvh) * D, knw, QKN, eps, cs + (int64_t)rt * D, sn + (int64_t)rt * D, lane, y1, y2))
            continue;
        Kb[p * D + lane] = f32_to_bf16(y1);
        Kb[p * D + lane + half] = f32_to_bf16(y2);
        const bf16_t *vsrc = qkv + (int64_t)rt * ld_qkv + (nh + nkv + kvh) * D;
        *reinterpret_cast<uint32_t *>(Vb + p * D + lane * 2) = *reinterpret_cast<const uint32_t *>(vsrc + lane * 2);
    }
    __threadfence_block();
    __syncthreads();            // the rows are in the cache (this CU's L1 is write-through and shared by the workgroup's waves)
    AttnTile0<D> t0;
    attn_prefetch<D>(t0, Kb, Vb, mrow, maxlen, tid, lane, wave);
    attn_finish<D, false>(t0, qs, part, sc, red, Kb, Vb, mrow, maxlen, -1, nullptr, nullptr, scale, out + ((int64_t)r * nh + h) * D, tid,
                          lane, wave);
}

// The same for MANY sequences per step (17..64: BASELINE configs[3] on one GPU): one workgroup per (KV head, sequence) serves all G = nh / nkv
// query heads of the group, so a key / value row is fetched once instead of G times (at 64 sequences x 32 heads the per-head kernel took
// 55 us per layer, most of it G-fold re-reads through L2: profiles/r6_llama64_kernel_stats.csv).  Same access pattern as attn_decode.h --
// a wave instruction covers RPI whole rows, lane (r, c) holds 16 bytes of row r -- with G query pieces in registers per lane: G dot
// products per loaded key piece, G axpys per value piece.  Softmax statistics in f32 per head.  The first 256 keys / values are requested
// before the rotary arithmetic.  Arithmetic per head as decode_attn_rope_kernel up to the f32 summation order of P.V.  QKN as there.
template <int D, int G, int W, bool QKN>      // W waves per workgroup (8 | 16): a wave takes 256 / W keys of a tile
__global__ __launch_bounds__(64 * W) void decode_attn_rope_gqa_kernel(const bf16_t *__restrict__ qkv, int64_t ld_qkv,
                                                                   const bf16_t *__restrict__ cs, const bf16_t *__restrict__ sn,
                                                                   int64_t cs0, bf16_t *__restrict__ K, bf16_t *__restrict__ V,
                                                                   const long long *__restrict__ pos_ptr,
                                                                   const unsigned char *__restrict__ mask, int64_t ms0,
                                                                   bf16_t *__restrict__ out, int nh, int nkv, int maxlen, float scale,
                                                                   const bf16_t *__restrict__ qnw, const bf16_t *__restrict__ knw,
                                                                   float eps) {
    constexpr int LPR = AttnGeom<D, W>::LPR, NI = AttnGeom<D, W>::NI, half = D / 2, THREADS = 64 * W;
    extern __shared__ __attribute__((aligned(16))) float sm_attn3[];
    float *qs = sm_attn3;                         // [G][D] rotated queries, f32 of their bf16 values
    float *part = qs + G * D;                     // [waves][G][D] partial outputs
    bf16_t *kn = reinterpret_cast<bf16_t *>(part + W * G * D);      // [D] rotated new key (bf16)
    bf16_t *vn = kn + D;                          // [D] new value
    float *sc = reinterpret_cast<float *>(vn + D);                           // [G][maxlen] scores -> probabilities
    __shared__ float red[2 * G * W];
    const int kvh = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long p = *pos_ptr;
    const bool pvalid = p >= 0 && p < maxlen;
    const bf16_t *row = qkv + b * ld_qkv;
    const bf16_t *c = cs + b * cs0, *sv = sn + b * cs0;
    bf16_t *Kb = K + ((int64_t)b * nkv + kvh) * maxlen * D;
    bf16_t *Vb = V + ((int64_t)b * nkv + kvh) * maxlen * D;
    const unsigned char *mrow = mask + b * ms0;
    // the first 256 keys (and the mask byte of key `tid`) are requested before the rotary arithmetic; the values of that tile are requested
    // right behind the score pass, into the registers the keys leave free -- <= 128 VGPRs for groups of up to four heads, i.e. two
    // workgroups per CU: at 64 sequences x 8 KV heads all 512 workgroups are resident at once (one round instead of two)
    const int cc = lane % LPR, r = lane / LPR;
    // cache slots behind the position being written hold no keys yet (every mask this kernel is handed hides them: causal decode), so the
    // first tile is only requested up to it: a quarter of the key / value bytes at the average length of a 128 + 128 token generation
    const int jlim = pvalid ? (int)min((long long)maxlen, p + 1) : maxlen;
    au32x4 k0[NI], v0[NI];
    const unsigned char mk0 = tid < maxlen ? mrow[tid] : (unsigned char)0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = attn_key<D, W>(0, wave, i, lane);
        k0[i] = j < jlim ? *reinterpret_cast<const au32x4 *>(Kb + (int64_t)j * D + cc * 8) : (au32x4)(0);
    }
    for (int role = wave; role < G + 2; role += W) {        // roles 0..G-1: query heads; G: the new key; G+1: the new value
        float y1, y2;
        if (role < G) {
            if (head_row_rotated<D>(row + (kvh * G + role) * D, qnw, QKN, eps, c, sv, lane, y1, y2)) {
                qs[role * D + lane] = bfr2(y1);
                qs[role * D + lane + half] = bfr2(y2);
            }
        } else if (role == G) {
            if (head_row_rotated<D>(row + (nh + kvh) * D, knw, QKN, eps, c, sv, lane, y1, y2)) {
                const bf16_t k1 = f32_to_bf16(y1), k2 = f32_to_bf16(y2);
                kn[lane] = k1;
                kn[lane + half] = k2;
                if (pvalid) {
                    Kb[p * D + lane] = k1;
                    Kb[p * D + lane + half] = k2;
                }
            }
        } else {
            if (lane < half) {
                const bf16_t *src = row + (nh + nkv + kvh) * D;
                const uint32_t v2 = *reinterpret_cast<const uint32_t *>(src + lane * 2);
                *reinterpret_cast<uint32_t *>(vn + lane * 2) = v2;
                if (pvalid) *reinterpret_cast<uint32_t *>(Vb + p * D + lane * 2) = v2;
            }
        }
    }
    __syncthreads();
    const long long pn = pvalid ? p : -1;
    float q[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) q[g][e] = qs[g * D + cc * 8 + e];
    // ---- scores: the prefetched tile first (its registers are free afterwards), then any further tile of a longer context
    auto score_tile = [&](int j0, au32x4 (&kk)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = attn_key<D, W>(j0, wave, i, lane);
            if (j == pn) kk[i] = *reinterpret_cast<const au32x4 *>(kn + cc * 8);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float d = attn_row_sum<LPR>(attn_dot8(q[g], kk[i]));
                if (cc == 0 && j < maxlen) sc[g * maxlen + j] = d * scale;
            }
        }
    };
    score_tile(0, k0);
    for (int j0 = 256; j0 < maxlen; j0 += 256) {
        au32x4 kk[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = attn_key<D, W>(j0, wave, i, lane);
            kk[i] = (j < maxlen && mrow[j] != 0) ? *reinterpret_cast<const au32x4 *>(Kb + (int64_t)j * D + cc * 8) : (au32x4)(0);
        }
        score_tile(j0, kk);
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {          // the values of the first tile, into the registers the keys and queries have left: in flight under the softmax
        const int j = attn_key<D, W>(0, wave, i, lane);
        v0[i] = j < jlim ? *reinterpret_cast<const au32x4 *>(Vb + (int64_t)j * D + cc * 8) : (au32x4)(0);
    }
    __syncthreads();
    // ---- softmax statistics per head over the unmasked keys
    float mx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) mx[g] = -INFINITY;
    for (int j = tid; j < maxlen; j += THREADS) {
        const bool ok = (j == tid ? mk0 : mrow[j]) != 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float s = ok ? sc[g * maxlen + j] : -INFINITY;
            sc[g * maxlen + j] = s;
            mx[g] = fmaxf(mx[g], s);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float m = wave_max(mx[g]);
        if (lane == 0) red[g * W + wave] = m;
    }
    __syncthreads();
    float sum[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float m = red[g * W];
#pragma unroll
        for (int w = 1; w < W; ++w) m = fmaxf(m, red[g * W + w]);
        mx[g] = m;
        sum[g] = 0.f;
    }
    for (int j = tid; j < maxlen; j += THREADS) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float s = sc[g * maxlen + j];
            const float e = (s == -INFINITY) ? 0.f : expf(s - mx[g]);
            sc[g * maxlen + j] = e;
            sum[g] += e;
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float t = wave_sum(sum[g]);
        if (lane == 0) red[(G + g) * W + wave] = t;
    }
    __syncthreads();
    // ---- out = P V: lane (r, c) accumulates columns 8c..8c+7 of every head over the rows it sees
    float acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
    auto pv_tile = [&](int j0, au32x4 (&vt)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = attn_key<D, W>(j0, wave, i, lane);
            const bool live = j < maxlen && mrow[j < maxlen ? j : 0] != 0;
            au32x4 vv = vt[i];
            if (j == pn) vv = *reinterpret_cast<const au32x4 *>(vn + cc * 8);
            if (!live) vv = (au32x4)(0);          // masked rows may hold anything (NaN from padded positions)
#pragma unroll
            for (int g = 0; g < G; ++g) attn_axpy8(acc[g], live ? sc[g * maxlen + j] : 0.f, vv);
        }
    };
    pv_tile(0, v0);
    for (int j0 = 256; j0 < maxlen; j0 += 256) {
        au32x4 vt[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int j = attn_key<D, W>(j0, wave, i, lane);
            vt[i] = (j < maxlen && mrow[j] != 0) ? *reinterpret_cast<const au32x4 *>(Vb + (int64_t)j * D + cc * 8) : (au32x4)(0);
        }
        pv_tile(j0, vt);
    }
    // rows of one wave instruction -> one partial per wave, then across waves through LDS
    attn_fold_rows<D, G>(acc);
    if (r == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) part[(wave * G + g) * D + cc * 8 + e] = acc[g][e];
    }
    __syncthreads();
    for (int i = tid; i < G * D; i += THREADS) {
        const int g = i / D, d = i % D;
        float o = 0.f;
#pragma unroll
        for (int w = 0; w < W; ++w) o += part[(w * G + g) * D + d];
        float den = red[(G + g) * W];
#pragma unroll
        for (int w = 1; w < W; ++w) den += red[(G + g) * W + w];
        const float inv = den > 0.f ? 1.f / den : 0.f;      // a fully masked query row (left padding) yields zeros, not NaN
        out[((int64_t)b * nh + kvh * G + g) * D + d] = f32_to_bf16(o * inv);
    }
}

}  // namespace ll

using namespace ll;

template <bool QKN>
static int decode_attn_rope(const char *who, const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc,
                            void *Vc, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh, int nkv,
                            int maxlen, int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps, void *stream) {
    LL_CHECK(qkv && cos && sin && Kc && Vc && pos && mask && out, "%s: null argument", who);
    LL_CHECK(!QKN || (q_norm_w && k_norm_w), "%s: null norm weight", who);
    LL_CHECK(!QKN || eps > 0.f, "%s: eps must be positive", who);
    LL_CHECK((D == 64 || D == 128) && B >= 1 && nkv >= 1 && nh % nkv == 0 && maxlen >= 1 && maxlen <= ATTN_MAX_KEYS && ld_qkv % 8 == 0,
             "%s: unsupported shape", who);
    // many sequences: one workgroup per (KV head, sequence) for the group sizes of the supported models (Llama-3.1-8B / Mistral-7B 4,
    // Qwen2-7B 7, the toy models 2); up to 16 sequences keep the per-head kernel (bit-identical to the op-by-op path)
    const int G = nh / nkv;
    if (B > 16 && (G == 2 || G == 4 || G == 7)) {
        const int gw = G <= 4 ? 16 : 8;
        const size_t l3 = (size_t)(G * D + gw * G * D) * 4 + (size_t)2 * D * 2 + (size_t)G * maxlen * 4;
        if (l3 <= 150 * 1024) {
            dim3 g3(nkv, B);
#define LL_GQA(D_, G_, W_)                                                                                                               \
    do {                                                                                                                                 \
        LL_TRY((allow_dynamic_lds<decode_attn_rope_gqa_kernel<D_, G_, W_, QKN>>(l3)));                                                   \
        hipLaunchKernelGGL((decode_attn_rope_gqa_kernel<D_, G_, W_, QKN>), g3, dim3(64 * W_), l3, (hipStream_t)stream, (const bf16_t *)qkv, ld_qkv, \
                           (const bf16_t *)cos, (const bf16_t *)sin, cs_stride, (bf16_t *)Kc, (bf16_t *)Vc, (const long long *)pos,      \
                           (const unsigned char *)mask, mask_stride, (bf16_t *)out, nh, nkv, maxlen, scale,                             \
                           (const bf16_t *)q_norm_w, (const bf16_t *)k_norm_w, eps);                                                    \
    } while (0)
            // sixteen waves for groups of up to four heads (16 keys per wave and tile: <= 128 VGPRs), eight for seven (Qwen2-7B)
            if (D == 128) {
                if (G == 2) LL_GQA(128, 2, 16); else if (G == 4) LL_GQA(128, 4, 16); else LL_GQA(128, 7, 8);
            } else {
                if (G == 2) LL_GQA(64, 2, 16); else if (G == 4) LL_GQA(64, 4, 16); else LL_GQA(64, 7, 8);
            }
#undef LL_GQA
            LL_LAUNCH_CHECK();
            return LL_OK;
        }
    }
    const size_t lds = (size_t)(D + ATTN_PART_FLOATS) * 4 + (size_t)2 * D * 2 + (size_t)maxlen * 4;
    dim3 grid(nh, B);
#define LL_ATTN(D_)                                                                                                                      \
    do {                                                                                                                                 \
        LL_TRY((allow_dynamic_lds<decode_attn_rope_kernel<D_, QKN>>(lds)));       /* maxlen > ~12 k keys */                              \
        hipLaunchKernelGGL((decode_attn_rope_kernel<D_, QKN>), grid, dim3(ATTN_THREADS), lds, (hipStream_t)stream, (const bf16_t *)qkv,       \
                           ld_qkv, (const bf16_t *)cos, (const bf16_t *)sin, cs_stride, (bf16_t *)Kc, (bf16_t *)Vc,                      \
                           (const long long *)pos, (const unsigned char *)mask, mask_stride, (bf16_t *)out, nh, nkv, maxlen, scale,     \
                           (const bf16_t *)q_norm_w, (const bf16_t *)k_norm_w, eps);                                                    \
    } while (0)
    if (D == 128) LL_ATTN(128); else LL_ATTN(64);
#undef LL_ATTN
    LL_LAUNCH_CHECK();
    return LL_OK;
}

template <bool QKN>
static int suffix_attn_rope(const char *who, const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc,
                            const int64_t *pos, const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                            const void *q_norm_w, const void *k_norm_w, float eps, void *stream) {
    LL_CHECK(qkv && cos && sin && Kc && Vc && pos && mask && out, "%s: null argument", who);
    LL_CHECK(!QKN || (q_norm_w && k_norm_w), "%s: null norm weight", who);
    LL_CHECK(!QKN || eps > 0.f, "%s: eps must be positive", who);
    LL_CHECK((D == 64 || D == 128) && B >= 1 && S >= 1 && S <= 16 && nkv >= 1 && nh % nkv == 0 && maxlen >= 1 && maxlen <= ATTN_MAX_KEYS &&
                 ld_qkv % 8 == 0,
             "%s: unsupported shape", who);
    const size_t lds = ((size_t)maxlen + D + ATTN_PART_FLOATS) * 4;
    dim3 grid(nh, B * S);
#define LL_ATTN(D_)                                                                                                                      \
    do {                                                                                                                                 \
        LL_TRY((allow_dynamic_lds<suffix_attn_rope_kernel<D_, QKN>>(lds)));       /* maxlen > ~12 k keys */                              \
        hipLaunchKernelGGL((suffix_attn_rope_kernel<D_, QKN>), grid, dim3(ATTN_THREADS), lds, (hipStream_t)stream, (const bf16_t *)qkv,       \
                           ld_qkv, (const bf16_t *)cos, (const bf16_t *)sin, (bf16_t *)Kc, (bf16_t *)Vc, (const long long *)pos,         \
                           (const unsigned char *)mask, (bf16_t *)out, nh, nkv, S, maxlen, scale, (const bf16_t *)q_norm_w,             \
                           (const bf16_t *)k_norm_w, eps);                                                                              \
    } while (0)
    if (D == 128) LL_ATTN(128); else LL_ATTN(64);
#undef LL_ATTN
    LL_LAUNCH_CHECK();
    return LL_OK;
}

extern "C" {

int ll_decode_attn_bf16(const void *q, const void *K, const void *V, const void *mask, void *out, int B, int nh, int nkv, int S,
                        int maxlen, int D, float scale, const int64_t *qstr, const int64_t *mstr, void *stream) {
    LL_CHECK(q && K && V && mask && out && qstr && mstr, "null argument");
    LL_CHECK((D == 64 || D == 128) && nh % nkv == 0 && maxlen >= 1 && maxlen <= ATTN_MAX_KEYS, "ll_decode_attn_bf16: unsupported shape");
    const size_t lds = ((size_t)maxlen + D + ATTN_PART_FLOATS) * 4;
    dim3 grid(nh, B * S);
#define LL_ATTN(D_)                                                                                                                      \
    do {                                                                                                                                 \
        LL_TRY((allow_dynamic_lds<decode_attn_bf16_kernel<D_>>(lds)));       /* maxlen > ~12 k keys */                                   \
        hipLaunchKernelGGL((decode_attn_bf16_kernel<D_>), grid, dim3(ATTN_THREADS), lds, (hipStream_t)stream, (const bf16_t *)q,         \
                           (const bf16_t *)K, (const bf16_t *)V, (const unsigned char *)mask, (bf16_t *)out, nh, nkv, S, maxlen, scale,  \
                           qstr[0], qstr[1], qstr[2], mstr[0], mstr[1]);                                                                 \
    } while (0)
    if (D == 128) LL_ATTN(128); else LL_ATTN(64);
#undef LL_ATTN
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_decode_attn_rope_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc,
                             void *Vc, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh,
                             int nkv, int maxlen, int D, float scale, void *stream) {
    return decode_attn_rope<false>("ll_decode_attn_rope_bf16", qkv, ld_qkv, cos, sin, cs_stride, Kc, Vc, pos, mask, mask_stride, out, B, nh,
                                   nkv, maxlen, D, scale, nullptr, nullptr, 0.f, stream);
}

int ll_decode_attn_rope_qkn_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kc,
                                 void *Vc, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh,
                                 int nkv, int maxlen, int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps,
                                 void *stream) {
    return decode_attn_rope<true>("ll_decode_attn_rope_qkn_bf16", qkv, ld_qkv, cos, sin, cs_stride, Kc, Vc, pos, mask, mask_stride, out, B,
                                  nh, nkv, maxlen, D, scale, q_norm_w, k_norm_w, eps, stream);
}

int ll_suffix_attn_rope_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                             const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale, void *stream) {
    return suffix_attn_rope<false>("ll_suffix_attn_rope_bf16", qkv, ld_qkv, cos, sin, Kc, Vc, pos, mask, out, B, S, nh, nkv, maxlen, D,
                                   scale, nullptr, nullptr, 0.f, stream);
}

int ll_suffix_attn_rope_qkn_bf16(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kc, void *Vc, const int64_t *pos,
                                 const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                                 const void *q_norm_w, const void *k_norm_w, float eps, void *stream) {
    return suffix_attn_rope<true>("ll_suffix_attn_rope_qkn_bf16", qkv, ld_qkv, cos, sin, Kc, Vc, pos, mask, out, B, S, nh, nkv, maxlen, D,
                                  scale, q_norm_w, k_norm_w, eps, stream);
}

}  // extern "C"
