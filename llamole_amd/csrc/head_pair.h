// head_pair: the load (and, for the Qwen3 layout, the per-head RMSNorm) of the element pair a rotating lane holds.  One device function for every
// kernel that rotates a q or k head row (llm_layer.hip, llm_attn_split.hip), so a key row is stored with the same bits whichever kernel writes it.
#pragma once
#include "common.h"
#include "gemv_body.h"

namespace ll {

// Per-head q/k RMSNorm of the Qwen3 layout (Qwen3RMSNorm over head_dim, between the projection and the rotary embedding), on the pair of
// elements (lane, lane + D/2) a rotating lane holds:  xh = bf16(x * rsqrt(mean_D(x^2) + eps)),  y = bf16(w * xh)  -- f32 arithmetic, each product
// rounded to bf16 once, as the module computes on bf16 data.  The whole head row sits in one wave, so the mean is one wave_sum and no LDS.
// QKN: called by ALL 64 lanes of the wave (D = 64: lanes 32..63 contribute zeros and get zeros back).  Without QKN it is the plain load of the
// pair, called by the lanes < D/2 only, where the kernels always loaded it.
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

}  // namespace ll
