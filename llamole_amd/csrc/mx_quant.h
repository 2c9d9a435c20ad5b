// The OCP MX quantiser of llm_quant.mx_round on the device, in one place: the shared exponent of a block of 32 from the bf16 bits of its largest
// magnitude, and the element encoder (round to nearest, ties to even).  Used by the weight quantiser (llm_wq.hip) and by the MX8 KV cache
// (llm_attn_kv8.hip), which therefore agree with mx_round -- and with each other -- bit for bit.
#pragma once
#include "common.h"

namespace ll {

// shared exponent of a block from the bf16 bits of its amax (sign cleared): amax = m * 2^x, elem_max = M * 2^p -> e = x - p + (m > M)
template <int BITS> __device__ __forceinline__ int wq_block_exp(uint32_t amax_bits) {
    if (amax_bits == 0) return 0;
    constexpr int P = BITS == 8 ? 8 : 2, THR = BITS == 8 ? 0x60 : 0x40, LO = BITS == 8 ? -117 : -125, HI = BITS == 8 ? 119 : 125;
    int e = (int)(amax_bits >> 7) - 127 - P + ((int)(amax_bits & 0x7f) > THR ? 1 : 0);
    return e < LO ? LO : (e > HI ? HI : e);
}
// a >= 0 (already divided by the scale) -> code without the sign bit; *grid = the grid value it stands for.  Round to nearest, ties to even.
template <int BITS> __device__ __forceinline__ uint32_t wq_encode(float a, float *grid) {
    constexpr float MAXV = BITS == 8 ? 448.f : 6.f, MINN = BITS == 8 ? 0.015625f : 1.f, SUB = BITS == 8 ? 512.f : 2.f;
    constexpr int MB = BITS == 8 ? 3 : 1, EB = BITS == 8 ? 7 : 1;       // mantissa bits, exponent bias
    a = fminf(a, MAXV);
    if (a < MINN) {                    // subnormal grid: multiples of 2^-9 (0.5); rintf rounds half to even
        const float q = rintf(a * SUB);
        *grid = q / SUB;
        return (uint32_t)q;            // q == SUB * MINN is the smallest normal code
    }
    uint32_t b = __float_as_uint(a);
    constexpr uint32_t DROP = 23 - MB;
    b += ((1u << (DROP - 1)) - 1u) + ((b >> DROP) & 1u);
    b &= ~((1u << DROP) - 1u);
    *grid = __uint_as_float(b);
    return (((b >> 23) - 127 + EB) << MB) | ((b >> DROP) & ((1u << MB) - 1u));
}

}  // namespace ll
