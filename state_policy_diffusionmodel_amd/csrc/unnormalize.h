// unnormalize.h -- the U(n) and A(n) of include/spdm.h: a normalised position / action back in the dataset's units, in float64.
// Shared by evaluation.hip (spdm_eval_errors) and policy.hip (spdm_policy_unnormalize), so the two cannot drift apart.
// Every operation is rounded on its own: contraction is switched off inside each function, whatever the including file sets.
#pragma once

#include <hip/hip_runtime.h>

namespace spdm {

// utils/data_utils.py:35-40 in float64: ((n 2 + translation) + 1) / 2 (max - min) + min
__device__ __forceinline__ double unnormalize_position(float n, double tr, double lo, double range) {
#pragma clang fp contract(off)
    const double s = (double)n * 2.0 + tr;
    return (s + 1.0) / 2.0 * range + lo;
}

// utils/data_utils.py:23-26 on a float32 array with float64 statistics: (n + 1) / 2 stays float32, the rest is float64
__device__ __forceinline__ double unnormalize_action(float n, double lo, double range) {
#pragma clang fp contract(off)
    const float h = (n + 1.0f) / 2.0f;
    return (double)h * range + lo;
}

}  // namespace spdm
