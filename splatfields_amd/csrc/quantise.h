// The 8-bit round trip of the image files the reference reads its metrics from (include/splatraster.h: SR_QUANT_*), applied
// on load by every evaluation kernel (metrics.hip, lpips.hip):
//   png:  q = trunc(clamp(x 255 + 0.5, 0, 255)),  to8b:  q = trunc(255 clamp(x, 0, 1));  the image becomes q / 255
// (multiply and add rounded separately: a contracted FMA flips pixels at the half-way points).
#pragma once
#include "common.h"

namespace sr {

// -> the quantised value; `level` is q (0 without a quantisation)
template <int kQuant>
__device__ __forceinline__ float quantise(float x, float& level) {
    if (kQuant == SR_QUANT_PNG) {
        float t = __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
        t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
        level = truncf(t);
        return __fdiv_rn(level, 255.0f);
    }
    if (kQuant == SR_QUANT_TO8B) {
        const float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
        level = truncf(__fmul_rn(255.0f, c));
        return __fdiv_rn(level, 255.0f);
    }
    level = 0.0f;
    return x;
}

}  // namespace sr
