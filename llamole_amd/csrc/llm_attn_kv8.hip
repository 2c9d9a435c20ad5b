// The microscaled FP8 (OCP MXFP8) KV cache of the fused decode: ll_kv8_store_bf16, ll_kv8_load_bf16, ll_decode_attn_rope_kv8 and
// ll_suffix_attn_rope_kv8.
//
// Storage, per cache layer four contiguous uint8 tensors: K codes and V codes [B, nkv, maxlen, D] (FP8 E4M3, OCP e4m3fn) and K scales and V
// scales [B, nkv, maxlen, D / 32] (E8M0: the byte e + 127 of the scale 2^e shared by 32 consecutive elements of head_dim).  The stored row of
// a slot is llm_quant.mx_round(row, 8) of the bf16 row a bf16 cache stores (K behind the optional head RMSNorm and the rotation, V as it
// leaves q|k|v): the quantiser is mx_quant.h's, the one ll_wq_quantize_bf16 runs, bit for bit.  code * 2^e is exactly a bf16 number, so
// ll_kv8_load_bf16 loses nothing and HF's attention on its output sees the numbers the kernels here see.  A row is D + D / 32 bytes against 2 D.
//
// The attention is the key-split one of llm_attn_split.hip -- same grid, same ranges of SPLIT_RANGE = 512 keys, same lane roles (lane (r, c)
// holds columns 8c .. 8c+7 of its row: here 8 code bytes and the scale byte of their block), same f32 dots, DPP row sums and summation orders,
// the same second launch (attn_split_combine_kernel, attn_split.h), no atomics -- with the codes expanded to f32 in registers by
// v_cvt_scalef32_pk_f32_fp8 (exact).  Masked keys and zero-weight values are dropped by a select, never by a multiplication: padded slots may
// hold NaN codes (0x7f) and the scale byte 0xff.
//
// The new rows: a workgroup whose range holds a new slot rotates the row, rounds it to bf16, quantises it (one 32-lane maximum per block)
// into LDS in the cache's own format and attends to it from there, i.e. to its DEQUANTISED value -- what every later step reads from the cache.
// Codes and scales of slot *pos + t are stored by exactly one workgroup, under the writer rule of the bf16 kernel.
#include "common.h"
#include "attn_decode.h"
#include "attn_split.h"
#include "head_pair.h"
#include "mx_quant.h"

namespace ll {

typedef uint32_t ku32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((ext_vector_type(2))) float kf32x2;

constexpr uint32_t KV8_ONE = 127;        // the scale byte of 2^0: what stands in for the scale of a row that is not read

__device__ __forceinline__ float kv8_scale(uint32_t byte) { return __uint_as_float(byte << 23); }

// Quantise the element pair (lane, lane + D/2) of a bf16 row held one pair per lane < D/2 (b1 / b2: the bf16 bits; 0 on the other lanes).
// Called by ALL 64 lanes.  The 32 lanes of a half wave hold the 32 elements of one block in b1 and of another in b2: blocks lane / 32 and
// (lane + D/2) / 32.  c1 / c2: the E4M3 codes, s1 / s2: the scale bytes of those two blocks.
template <int D>
__device__ __forceinline__ void kv8_quant_pair(uint32_t b1, uint32_t b2, uint32_t &c1, uint32_t &c2, uint32_t &s1, uint32_t &s2) {
    uint32_t a1 = b1 & 0x7fffu, a2 = b2 & 0x7fffu;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
        const uint32_t o1 = (uint32_t)__shfl_xor((int)a1, off, 64), o2 = (uint32_t)__shfl_xor((int)a2, off, 64);
        a1 = a1 > o1 ? a1 : o1;
        a2 = a2 > o2 ? a2 : o2;
    }
    const int e1 = wq_block_exp<8>(a1), e2 = wq_block_exp<8>(a2);
    float g;
    c1 = wq_encode<8>(fabsf(bf16_to_f32((bf16_t)b1)) * __uint_as_float((uint32_t)(127 - e1) << 23), &g) | ((b1 >> 15) << 7);
    c2 = wq_encode<8>(fabsf(bf16_to_f32((bf16_t)b2)) * __uint_as_float((uint32_t)(127 - e2) << 23), &g) | ((b2 >> 15) << 7);
    s1 = (uint32_t)(e1 + 127);
    s2 = (uint32_t)(e2 + 127);
}

// the pair of a lane < D/2 into a row of codes and its scale bytes (global memory or LDS)
template <int D>
__device__ __forceinline__ void kv8_put_pair(unsigned char *codes, unsigned char *scales, int lane, uint32_t c1, uint32_t c2, uint32_t s1,
                                             uint32_t s2) {
    constexpr int half = D / 2;
    codes[lane] = (unsigned char)c1;
    codes[lane + half] = (unsigned char)c2;
    if ((lane & 31) == 0) {
        scales[lane >> 5] = (unsigned char)s1;
        scales[(lane + half) >> 5] = (unsigned char)s2;
    }
}

__device__ __forceinline__ float kv8_dot8(const float (&q)[8], ku32x2 w, float s) {
    const kf32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], s, false), b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[0], s, true);
    const kf32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], s, false), d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[1], s, true);
    float r = 0.f;
    r = fmaf(q[0], a.x, r);
    r = fmaf(q[1], a.y, r);
    r = fmaf(q[2], b.x, r);
    r = fmaf(q[3], b.y, r);
    r = fmaf(q[4], c.x, r);
    r = fmaf(q[5], c.y, r);
    r = fmaf(q[6], d.x, r);
    r = fmaf(q[7], d.y, r);
    return r;
}

// one wave per (sequence, KV head, new position): the row of k_new and of v_new into slot *pos + s
template <int D>
__global__ __launch_bounds__(64) void kv8_store_kernel(unsigned char *__restrict__ Kq, unsigned char *__restrict__ Ks,
                                                       unsigned char *__restrict__ Vq, unsigned char *__restrict__ Vs,
                                                       const bf16_t *__restrict__ kn, const bf16_t *__restrict__ vn,
                                                       const long long *__restrict__ pos, int nkv, int S, int maxlen, int64_t ks0, int64_t ks1,
                                                       int64_t ks2, int64_t vs0, int64_t vs1, int64_t vs2) {
    constexpr int half = D / 2, NB = D / 32;
    const int r = blockIdx.x;            // (b*nkv + h)*S + s
    const int s = r % S, h = (r / S) % nkv, b = r / (S * nkv);
    const long long p = *pos + s;
    if (p < 0 || p >= maxlen) return;
    const int lane = threadIdx.x;
    const bool on = lane < half;
    const bf16_t *ksrc = kn + b * ks0 + h * ks1 + s * ks2;
    const bf16_t *vsrc = vn + b * vs0 + h * vs1 + s * vs2;
    const uint32_t k1 = on ? ksrc[lane] : 0u, k2 = on ? ksrc[lane + half] : 0u;
    const uint32_t v1 = on ? vsrc[lane] : 0u, v2 = on ? vsrc[lane + half] : 0u;
    uint32_t kc1, kc2, ke1, ke2, vc1, vc2, ve1, ve2;
    kv8_quant_pair<D>(k1, k2, kc1, kc2, ke1, ke2);
    kv8_quant_pair<D>(v1, v2, vc1, vc2, ve1, ve2);
    if (on) {
        const int64_t row = ((int64_t)b * nkv + h) * maxlen + p;
        kv8_put_pair<D>(Kq + row * D, Ks + row * NB, lane, kc1, kc2, ke1, ke2);
        kv8_put_pair<D>(Vq + row * D, Vs + row * NB, lane, vc1, vc2, ve1, ve2);
    }
}

// slots [0, min(maxlen, *pos + extra)) of every (sequence, KV head) to bf16: a thread expands 8 codes.  grid (pieces of 256 threads, B * nkv)
template <int D>
__global__ __launch_bounds__(256) void kv8_load_kernel(const unsigned char *__restrict__ Kq, const unsigned char *__restrict__ Ks,
                                                       const unsigned char *__restrict__ Vq, const unsigned char *__restrict__ Vs,
                                                       bf16_t *__restrict__ K, bf16_t *__restrict__ V, const long long *__restrict__ pos,
                                                       int extra, int maxlen) {
    constexpr int LPR = D / 8, NB = D / 32;
    const long long want = *pos + extra;
    const int n = want < 0 ? 0 : (want > maxlen ? maxlen : (int)want);
    const int i = blockIdx.x * 256 + threadIdx.x;       // piece of 8 elements: slot i / LPR, columns 8 (i % LPR) ..
    const int j = i / LPR, c = i - j * LPR;
    if (j >= n) return;
    const int64_t row = (int64_t)blockIdx.y * maxlen + j;
    au32x4 o;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const unsigned char *codes = t ? Vq : Kq, *scales = t ? Vs : Ks;
        const ku32x2 w = *reinterpret_cast<const ku32x2 *>(codes + row * D + c * 8);
        const float s = kv8_scale(scales[row * NB + (c >> 2)]);
        o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], s, false));
        o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], s, true));
        o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], s, false));
        o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], s, true));
        *reinterpret_cast<au32x4 *>((t ? V : K) + row * D + c * 8) = o;
    }
}

// attn_split_partial_kernel (llm_attn_split.hip) on MX8 caches: the same arguments with Kq / Ks / Vq / Vs in place of K / V, the same workspace.
template <int D, int GT>
__global__ __launch_bounds__(ATTN_THREADS) void attn_kv8_partial_kernel(const bf16_t *__restrict__ qkv, int64_t ld_qkv,
                                                                    const bf16_t *__restrict__ cs, const bf16_t *__restrict__ sn, int64_t cs0,
                                                                    unsigned char *Kq, unsigned char *Ks, unsigned char *Vq, unsigned char *Vs,
                                                                    const long long *__restrict__ pos_ptr,
                                                                    const unsigned char *__restrict__ mask, int64_t ms0,
                                                                    float *__restrict__ ml, float *__restrict__ accw, int S, int nh, int nkv,
                                                                    int maxlen, float scale, const bf16_t *__restrict__ qnw,
                                                                    const bf16_t *__restrict__ knw, float eps) {
    constexpr int LPR = AttnGeom<D>::LPR, NI = AttnGeom<D>::NI, half = D / 2, NB = D / 32;
    // tiles whose loads a lane has in flight at once (8 code bytes and one scale byte per row: 3 VGPRs against the 4 of a bf16 piece): the whole
    // range, except for seven heads of 128 (one tile: with two the compiler's report shows 255 VGPRs and 438 spilled, as for the bf16 kernel)
    constexpr int TF = (GT == 7 && D == 128) ? 1 : SPLIT_TILES, NL = TF * NI;
    __shared__ __attribute__((aligned(16))) float qs[GT * D];                       // rotated queries, f32 of their bf16 values
    __shared__ __attribute__((aligned(16))) unsigned char knq[SPLIT_MAX_S * D];     // codes of the rotated new keys of this range, row t at t * D
    __shared__ __attribute__((aligned(16))) unsigned char vnq[SPLIT_MAX_S * D];     // codes of the new values
    __shared__ unsigned char kns[SPLIT_MAX_S * NB], vns[SPLIT_MAX_S * NB];          // their scale bytes
    __shared__ float sc[GT * SPLIT_RANGE];                                           // scores -> exponentials
    __shared__ float part[GT * ATTN_WAVES * D];                                      // per-wave partial outputs
    __shared__ float red[2 * GT * ATTN_WAVES];
    const int rho = blockIdx.x, hg = blockIdx.y, r = blockIdx.z;
    const int nr = gridDim.x;
    const int b = r / S, s = r - b * S;
    const int G = nh / nkv, h0 = hg * GT, kvh = h0 / G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = rho * SPLIT_RANGE, j1 = min(j0 + SPLIT_RANGE, maxlen);
    const unsigned char *mrow = mask + (int64_t)r * ms0;
    const unsigned char mk = j0 + tid < j1 ? mrow[j0 + tid] : (unsigned char)0;
    const long long p0 = *pos_ptr;
    // the new rows t whose slot p0 + t lies in this range: t in [tlo, thi)
    const long long lo = p0 > (long long)j0 ? p0 : (long long)j0, hi = p0 + S < (long long)j1 ? p0 + S : (long long)j1;
    const int tlo = lo < hi ? (int)(lo - p0) : 0, thi = lo < hi ? (int)(hi - p0) : 0;
    const bool writer = h0 % G == 0 && s >= tlo && s < thi;                    // this workgroup stores the row of slot p0 + s
    const int any = __syncthreads_or(mk != 0);
    const int64_t wbase = ((int64_t)r * nh + h0) * nr + rho;                   // + g * nr per head
    if (!any && !writer) {
        if (tid < GT) {
            ml[(wbase + (int64_t)tid * nr) * 2] = -INFINITY;
            ml[(wbase + (int64_t)tid * nr) * 2 + 1] = 0.f;
        }
        return;
    }
    const int64_t head = ((int64_t)b * nkv + kvh) * maxlen;
    unsigned char *Kqb = Kq + head * D, *Vqb = Vq + head * D, *Ksb = Ks + head * NB, *Vsb = Vs + head * NB;
    const int c = lane % LPR, rr = lane / LPR;
    // slot of (tile, instruction i, lane); a slot is fetched from the cache iff it lies in the range and is none of the new rows
    auto fetch = [&](int j) { return j < j1 && !((long long)j >= lo && (long long)j < hi); };
    ku32x2 kk[NL];
    uint32_t ke[NL];
    auto load_rows = [&](ku32x2 (&x)[NL], uint32_t (&e)[NL], const unsigned char *codes, const unsigned char *scales, int jt) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int j = attn_key<D>(jt + (i / NI) * 256, wave, i % NI, lane);
            const bool f = fetch(j);
            x[i] = f ? *reinterpret_cast<const ku32x2 *>(codes + (int64_t)j * D + c * 8) : (ku32x2)(0);
            e[i] = f ? (uint32_t)scales[(int64_t)j * NB + (c >> 2)] : KV8_ONE;
        }
    };
    load_rows(kk, ke, Kqb, Ksb, j0);
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
            uint32_t k1 = 0, k2 = 0, v1 = 0, v2 = 0;
            if (knw) head_pair<D, true>(src, knw, eps, lane, x1, x2);
            if (lane < half) {
                if (!knw) head_pair<D, false>(src, knw, eps, lane, x1, x2);
                rope_pair<D>(x1, x2, cs + (int64_t)rt * cs0, sn + (int64_t)rt * cs0, lane, y1, y2);
                k1 = f32_to_bf16(y1), k2 = f32_to_bf16(y2);
                const bf16_t *vsrc = qkv + (int64_t)rt * ld_qkv + (nh + nkv + kvh) * D;
                v1 = vsrc[lane], v2 = vsrc[lane + half];
            }
            uint32_t kc1, kc2, ke1, ke2, vc1, vc2, ve1, ve2;       // all 64 lanes: the block maxima cross the lanes of a half wave
            kv8_quant_pair<D>(k1, k2, kc1, kc2, ke1, ke2);
            kv8_quant_pair<D>(v1, v2, vc1, vc2, ve1, ve2);
            if (lane < half) {
                kv8_put_pair<D>(knq + t * D, kns + t * NB, lane, kc1, kc2, ke1, ke2);
                kv8_put_pair<D>(vnq + t * D, vns + t * NB, lane, vc1, vc2, ve1, ve2);
                if (writer && t == s) {
                    const long long p = p0 + t;
                    kv8_put_pair<D>(Kqb + p * D, Ksb + p * NB, lane, kc1, kc2, ke1, ke2);
                    kv8_put_pair<D>(Vqb + p * D, Vsb + p * NB, lane, vc1, vc2, ve1, ve2);
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
            if (jt != j0) load_rows(kk, ke, Kqb, Ksb, jt);
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                const int j = attn_key<D>(jt + (i / NI) * 256, wave, i % NI, lane);
                if ((long long)j >= lo && (long long)j < hi) {
                    kk[i] = *reinterpret_cast<const ku32x2 *>(knq + (int)(j - p0) * D + c * 8);
                    ke[i] = kns[(int)(j - p0) * NB + (c >> 2)];
                }
                const float ks = kv8_scale(ke[i]);
#pragma unroll
                for (int g = 0; g < GT; ++g) {
                    const float d = attn_row_sum<LPR>(kv8_dot8(q[g], kk[i], ks));
                    if (c == 0 && j < j1) sc[g * SPLIT_RANGE + (j - j0)] = d * scale;
                }
            }
        }
    }
    __syncthreads();
    // the values are requested behind the barrier (the key registers are free) and arrive under the softmax statistics
    ku32x2 vv[NL];
    uint32_t ve[NL];
    load_rows(vv, ve, Vqb, Vsb, j0);
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
        if (jt != j0) load_rows(vv, ve, Vqb, Vsb, jt);
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
            if ((long long)j >= lo && (long long)j < hi) {
                vv[i] = *reinterpret_cast<const ku32x2 *>(vnq + (int)(j - p0) * D + c * 8);
                ve[i] = vns[(int)(j - p0) * NB + (c >> 2)];
            }
            if (zero) {                                                // masked rows may hold anything (NaN codes, the scale byte 0xff)
                vv[i] = (ku32x2)(0);
                ve[i] = KV8_ONE;
            }
            const float vs = kv8_scale(ve[i]);
            const kf32x2 a0 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vv[i][0], vs, false);
            const kf32x2 a1 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vv[i][0], vs, true);
            const kf32x2 a2 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vv[i][1], vs, false);
            const kf32x2 a3 = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vv[i][1], vs, true);
#pragma unroll
            for (int g = 0; g < GT; ++g) {
                acc[g][0] = fmaf(pj[g], a0.x, acc[g][0]);
                acc[g][1] = fmaf(pj[g], a0.y, acc[g][1]);
                acc[g][2] = fmaf(pj[g], a1.x, acc[g][2]);
                acc[g][3] = fmaf(pj[g], a1.y, acc[g][3]);
                acc[g][4] = fmaf(pj[g], a2.x, acc[g][4]);
                acc[g][5] = fmaf(pj[g], a2.y, acc[g][5]);
                acc[g][6] = fmaf(pj[g], a3.x, acc[g][6]);
                acc[g][7] = fmaf(pj[g], a3.y, acc[g][7]);
            }
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

static int attn_kv8(const char *who, const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs0, void *Kq, void *Ks, void *Vq,
                    void *Vs, const int64_t *pos, const void *mask, int64_t ms0, void *out, int B, int S, int nh, int nkv, int maxlen, int D,
                    float scale, const void *q_norm_w, const void *k_norm_w, float eps, void *workspace, int64_t workspace_bytes, void *stream) {
    LL_CHECK(qkv && cos && sin && Kq && Ks && Vq && Vs && pos && mask && out && workspace, "%s: null argument", who);
    LL_CHECK((q_norm_w != nullptr) == (k_norm_w != nullptr), "%s: only one of q_norm_w / k_norm_w", who);
    LL_CHECK(!q_norm_w || eps > 0.f, "%s: eps must be positive", who);
    LL_CHECK(split_shape_ok(B, S, nh, nkv, maxlen, D) && ld_qkv % 8 == 0, "%s: unsupported shape", who);
    LL_CHECK((uintptr_t)Kq % 8 == 0 && (uintptr_t)Vq % 8 == 0, "%s: the code tensors must be 8-byte aligned", who);
    LL_CHECK(workspace_bytes >= split_workspace_bytes(B, S, nh, maxlen, D) && (uintptr_t)workspace % 16 == 0,
             "%s: the workspace is smaller than ll_attn_split_workspace_bytes or not 16-byte aligned", who);
    const int nr = cdiv(maxlen, SPLIT_RANGE), rows = B * S, GT = split_group(nh, nkv);
    float *ml = (float *)workspace, *accw = ml + (int64_t)rows * nh * nr * 2;
    dim3 grid(nr, nh / GT, rows);
#define LL_KV8(D_, G_)                                                                                                                   \
    hipLaunchKernelGGL((attn_kv8_partial_kernel<D_, G_>), grid, dim3(ATTN_THREADS), 0, (hipStream_t)stream, (const bf16_t *)qkv, ld_qkv,   \
                       (const bf16_t *)cos, (const bf16_t *)sin, cs0, (unsigned char *)Kq, (unsigned char *)Ks, (unsigned char *)Vq,     \
                       (unsigned char *)Vs, (const long long *)pos, (const unsigned char *)mask, ms0, ml, accw, S, nh, nkv, maxlen,     \
                       scale, (const bf16_t *)q_norm_w, (const bf16_t *)k_norm_w, eps)
    if (D == 128) {
        if (GT == 1) LL_KV8(128, 1); else if (GT == 2) LL_KV8(128, 2); else if (GT == 4) LL_KV8(128, 4); else LL_KV8(128, 7);
    } else {
        if (GT == 1) LL_KV8(64, 1); else if (GT == 2) LL_KV8(64, 2); else if (GT == 4) LL_KV8(64, 4); else LL_KV8(64, 7);
    }
#undef LL_KV8
    LL_LAUNCH_CHECK();
    if (D == 128)
        hipLaunchKernelGGL((attn_split_combine_kernel<128>), dim3(nh, rows), dim3(COMBINE_THREADS), 0, (hipStream_t)stream, ml, accw,
                           (bf16_t *)out, nh, nr);
    else
        hipLaunchKernelGGL((attn_split_combine_kernel<64>), dim3(nh, rows), dim3(COMBINE_THREADS), 0, (hipStream_t)stream, ml, accw,
                           (bf16_t *)out, nh, nr);
    LL_LAUNCH_CHECK();
    return LL_OK;
}

}  // namespace ll

using namespace ll;

extern "C" {

int ll_kv8_store_bf16(void *Kq, void *Ks, void *Vq, void *Vs, const void *k_new, const void *v_new, const int64_t *pos, int B, int nkv, int S,
                      int maxlen, int D, const int64_t *kstr, const int64_t *vstr, void *stream) {
    LL_CHECK(Kq && Ks && Vq && Vs && k_new && v_new && pos && kstr && vstr, "ll_kv8_store_bf16: null argument");
    LL_CHECK((D == 64 || D == 128) && B >= 1 && nkv >= 1 && S >= 1 && maxlen >= 1 && (int64_t)B * nkv * S <= 0x7fffffff,
             "ll_kv8_store_bf16: unsupported shape");
#define LL_KV8_STORE(D_)                                                                                                                 \
    hipLaunchKernelGGL((kv8_store_kernel<D_>), dim3(B * nkv * S), dim3(64), 0, (hipStream_t)stream, (unsigned char *)Kq, (unsigned char *)Ks, \
                       (unsigned char *)Vq, (unsigned char *)Vs, (const bf16_t *)k_new, (const bf16_t *)v_new, (const long long *)pos,  \
                       nkv, S, maxlen, kstr[0], kstr[1], kstr[2], vstr[0], vstr[1], vstr[2])
    if (D == 128) LL_KV8_STORE(128); else LL_KV8_STORE(64);
#undef LL_KV8_STORE
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_kv8_load_bf16(const void *Kq, const void *Ks, const void *Vq, const void *Vs, void *K, void *V, const int64_t *pos, int extra, int B,
                     int nkv, int maxlen, int D, void *stream) {
    LL_CHECK(Kq && Ks && Vq && Vs && K && V && pos, "ll_kv8_load_bf16: null argument");
    LL_CHECK((D == 64 || D == 128) && B >= 1 && nkv >= 1 && maxlen >= 1 && maxlen <= SPLIT_MAXLEN && (int64_t)B * nkv <= 65535 && extra >= 0,
             "ll_kv8_load_bf16: unsupported shape");
    LL_CHECK((uintptr_t)Kq % 8 == 0 && (uintptr_t)Vq % 8 == 0 && (uintptr_t)K % 16 == 0 && (uintptr_t)V % 16 == 0,
             "ll_kv8_load_bf16: the code tensors must be 8-byte and the bf16 tensors 16-byte aligned");
    dim3 grid(cdiv(maxlen * (D / 8), 256), B * nkv);
#define LL_KV8_LOAD(D_)                                                                                                                  \
    hipLaunchKernelGGL((kv8_load_kernel<D_>), grid, dim3(256), 0, (hipStream_t)stream, (const unsigned char *)Kq, (const unsigned char *)Ks, \
                       (const unsigned char *)Vq, (const unsigned char *)Vs, (bf16_t *)K, (bf16_t *)V, (const long long *)pos, extra, maxlen)
    if (D == 128) LL_KV8_LOAD(128); else LL_KV8_LOAD(64);
#undef LL_KV8_LOAD
    LL_LAUNCH_CHECK();
    return LL_OK;
}

int ll_decode_attn_rope_kv8(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, int64_t cs_stride, void *Kq, void *Ks, void *Vq,
                            void *Vs, const int64_t *pos, const void *mask, int64_t mask_stride, void *out, int B, int nh, int nkv, int maxlen,
                            int D, float scale, const void *q_norm_w, const void *k_norm_w, float eps, void *workspace,
                            int64_t workspace_bytes, void *stream) {
    LL_CHECK(B <= 64, "ll_decode_attn_rope_kv8: unsupported shape (B=%d > 64)", B);
    return attn_kv8("ll_decode_attn_rope_kv8", qkv, ld_qkv, cos, sin, cs_stride, Kq, Ks, Vq, Vs, pos, mask, mask_stride, out, B, 1, nh, nkv,
                    maxlen, D, scale, q_norm_w, k_norm_w, eps, workspace, workspace_bytes, stream);
}

int ll_suffix_attn_rope_kv8(const void *qkv, int64_t ld_qkv, const void *cos, const void *sin, void *Kq, void *Ks, void *Vq, void *Vs,
                            const int64_t *pos, const void *mask, void *out, int B, int S, int nh, int nkv, int maxlen, int D, float scale,
                            const void *q_norm_w, const void *k_norm_w, float eps, void *workspace, int64_t workspace_bytes, void *stream) {
    return attn_kv8("ll_suffix_attn_rope_kv8", qkv, ld_qkv, cos, sin, D, Kq, Ks, Vq, Vs, pos, mask, maxlen, out, B, S, nh, nkv, maxlen, D, scale,
                    q_norm_w, k_norm_w, eps, workspace, workspace_bytes, stream);
}

}  // extern "C"
