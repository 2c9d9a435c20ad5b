// What the key-split decode attention has in common whatever the cache holds (bf16 rows: llm_attn_split.hip; MX8 codes: llm_attn_kv8.hip): the
// range length and the bounds, the workspace layout ([rows][nh][ranges] (m, l) then [rows][nh][ranges][D] un-normalised f32 outputs) and the
// second launch, attn_split_combine_kernel.
#pragma once
#include "common.h"
#include "attn_decode.h"

namespace ll {

constexpr int SPLIT_RANGE = 512;                                    // keys per workgroup = one mask byte per thread, two tiles of 256 keys
constexpr int SPLIT_TILES = SPLIT_RANGE / 256;
constexpr int SPLIT_MAXLEN = 131072;
constexpr int SPLIT_MAX_RANGES = SPLIT_MAXLEN / SPLIT_RANGE;       // 256
constexpr int SPLIT_MAX_S = 16;
constexpr int COMBINE_THREADS = 512;
static_assert(SPLIT_RANGE == ATTN_THREADS, "one mask byte and one score per thread");

// grid (nh, rows), COMBINE_THREADS threads: thread (k, d) sums the ranges r = k, k + NS, ... of column d, NS = COMBINE_THREADS / D slices.
template <int D>
__global__ __launch_bounds__(COMBINE_THREADS) void attn_split_combine_kernel(const float *__restrict__ ml, const float *__restrict__ accw,
                                                                         bf16_t *__restrict__ out, int nh, int nr) {
    constexpr int NS = COMBINE_THREADS / D, NW = COMBINE_THREADS / 64;
    __shared__ float w[SPLIT_MAX_RANGES];
    __shared__ float red[2 * NW];
    __shared__ float part[NS * D];
    const int h = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = ((int64_t)r * nh + h) * nr;
    const bool own = tid < nr;                                         // nr <= SPLIT_MAX_RANGES <= COMBINE_THREADS: one range per thread
    const float m = own ? ml[(base + tid) * 2] : -INFINITY;
    const float l = own ? ml[(base + tid) * 2 + 1] : 0.f;
    const float mx = wave_max(m);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    float M = red[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) M = fmaxf(M, red[i]);
    const float wr = m == -INFINITY ? 0.f : expf(m - M);             // a range without a visible key weighs nothing (no -inf - -inf)
    if (own) w[tid] = wr;
    const float wl = wave_sum(wr == 0.f ? 0.f : wr * l);
    if (lane == 0) red[NW + wave] = wl;
    __syncthreads();
    float L = red[NW];
#pragma unroll
    for (int i = 1; i < NW; ++i) L += red[NW + i];
    const int k = tid / D, d = tid - k * D;
    float o = 0.f;
#pragma unroll 8
    for (int rg = k; rg < nr; rg += NS) {
        const float wg = w[rg];
        const float a = wg != 0.f ? accw[(base + rg) * D + d] : 0.f;  // nothing was written for an empty range
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

static inline int split_group(int nh, int nkv) {
    const int G = nh / nkv;
    return (G == 2 || G == 4 || G == 7) ? G : 1;
}

static inline bool split_shape_ok(int B, int S, int nh, int nkv, int maxlen, int D) {
    return (D == 64 || D == 128) && B >= 1 && S >= 1 && S <= SPLIT_MAX_S && (int64_t)B * S <= 65535 && nkv >= 1 && nh >= nkv && nh % nkv == 0 &&
           nh / split_group(nh, nkv) <= 65535 && maxlen >= 1 && maxlen <= SPLIT_MAXLEN;
}

static inline int64_t split_workspace_bytes(int B, int S, int nh, int maxlen, int D) {
    const int64_t nr = cdiv(maxlen, SPLIT_RANGE);
    return (int64_t)B * S * nh * nr * (D + 2) * 4;
}

}  // namespace ll
