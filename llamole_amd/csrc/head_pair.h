// The rotation of a q or k head row: head_pair (the load and, for the Qwen3 layout, the per-head RMSNorm of the element pair a rotating lane
// holds), rope_pair (the rotary embedding of that pair) and head_row_rotated (both, with the lane rule between them).  The kernels of llm_attn.hip
// call head_row_rotated; attn_split_partial_kernel (llm_attn_split.hip) spells its three steps out in its role loop, with head_pair and rope_pair
// from here (through the function, one of its instances allocates two more VGPRs).  So a key row is stored with the same bits whichever kernel
// writes it.
#pragma once
#include "common.h"
#include "gemv_body.h"

namespace ll {

// Per-head q/k RMSNorm of the Qwen3 layout (Qwen3RMSNorm over head_dim, between the projection and the rotary embedding), on the pair of
// elements (lane, lane + D/2) a rotating lane holds:  xh = bf16(x * rsqrt(mean_D(x^2) + eps)),  y = bf16(w * xh)  -- f32 arithmetic, each product
// rounded to bf16 once, as the module computes on bf16 data.  The whole head row sits in one wave, so the mean is one wave_sum and no LDS.
// QKN: called by ALL 64 lanes of the wave (D = 64: lanes 32..63 contribute zeros and get zeros back).  Without QKN it is the plain load of the
// pair, called by the lanes < D/2 only.
template <int D, bool QKN>
__device__ __forceinline__ void head_pair(const bf16_t *src, const bf16_t *nw, float eps, int lane, float &x1, float &x2) {
    constexpr int half = D / 2;
    if (!QKN) {
        x1 = bf16_to_f32(src[lane]);
        x2 = bf16_to_f32(src[lane + half]);
        return;
    }
    const bool on = lane < half;
    x1 = on ? bf16_to_f32(src[lane]) : 0.f;
    x2 = on ? bf16_to_f32(src[lane + half]) : 0.f;
    const float w1 = on ? bf16_to_f32(nw[lane]) : 0.f, w2 = on ? bf16_to_f32(nw[lane + half]) : 0.f;
    const float ss = wave_sum(x1 * x1 + x2 * x2);
    const float rstd = rsqrtf(ss / (float)D + eps);
    x1 = bfr2(w1 * bfr2(x1 * rstd));
    x2 = bfr2(w2 * bfr2(x2 * rstd));
}

// rotary embedding of the pair (x1, x2) a lane < D/2 holds: x * cos and rotate_half(x) * sin, every product rounded to bf16 once; the caller rounds
// the sum (bfr2 for a query kept in f32, f32_to_bf16 for a key)
template <int D>
__device__ __forceinline__ void rope_pair(float x1, float x2, const bf16_t *c, const bf16_t *sv, int lane, float &y1, float &y2) {
    constexpr int half = D / 2;
    const float c1 = bf16_to_f32(c[lane]), c2 = bf16_to_f32(c[lane + half]);
    const float s1 = bf16_to_f32(sv[lane]), s2 = bf16_to_f32(sv[lane + half]);
    y1 = bfr2(x1 * c1) + bfr2(-x2 * s1);
    y2 = bfr2(x2 * c2) + bfr2(x1 * s2);
}

// The rotated pair (y1, y2) of the head row at src with the angles c / sv, unrounded sums; false on the lanes >= D/2, which hold no pair.
// Called by ALL 64 lanes of a wave: with norm (uniform over the wave) every lane takes part in head_pair's mean before the upper ones leave.
template <int D>
__device__ __forceinline__ bool head_row_rotated(const bf16_t *src, const bf16_t *nw, bool norm, float eps, const bf16_t *c, const bf16_t *sv,
                                                 int lane, float &y1, float &y2) {
    float x1, x2;
    if (norm) head_pair<D, true>(src, nw, eps, lane, x1, x2);
    if (lane < D / 2) {
        if (!norm) head_pair<D, false>(src, nw, eps, lane, x1, x2);
        rope_pair<D>(x1, x2, c, sv, lane, y1, y2);
    }
    return lane < D / 2;
}

}  // namespace ll
