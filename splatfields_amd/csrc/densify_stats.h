// The densification bookkeeping of ONE rendered splat (reference train.py:280-286, scene/gaussian_model.py:427-438), shared by the
// two kernels that apply it: k_densification_stats (preprocess.hip: row `at` is the splat's own number) and
// k_densification_stats_rows (subset.hip: row `at` = idx[i] of a subset step).  One function, so both round alike.
#pragma once
#include "common.h"

namespace sr {

#ifdef __HIPCC__

// r = radii of the rendered splat (the caller has tested r > 0), (gx, gy) = its dL_dmeans2D[:2]; any output may be NULL
__device__ __forceinline__ void densification_stats_row(size_t at, int r, float gx, float gy, float* __restrict__ grad_accum,
                                                        float* __restrict__ denom, float* __restrict__ max_radii2D) {
    if (grad_accum) grad_accum[at] += sqrtf(gx * gx + gy * gy);
    if (denom) denom[at] += 1.0f;
    if (max_radii2D) max_radii2D[at] = fmaxf(max_radii2D[at], (float)r);
}

#endif  // __HIPCC__

}  // namespace sr
