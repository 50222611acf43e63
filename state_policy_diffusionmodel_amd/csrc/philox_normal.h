// philox_normal.h -- Philox4x32-10 and the Box-Muller normals of the counter-based noise streams of include/spdm.h (purposes 1-3
// of spdm_train_forward_process, purpose 8 of spdm_policy_warm_start).  Shared by train_noise.hip and policy.hip, so the two
// cannot drift apart.  tests/forward_process_ref.py is the numpy restatement.
#pragma once

#include <hip/hip_runtime.h>

namespace spdm {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// u = ((w >> 8) + 0.5) 2^-24 in (0, 1]: the sum rounds once w >> 8 >= 2^23 (1.0 for 2^24 - 1, where logf gives 0), the same
// rounding as elementwise.hip's philox_normal and oracle/philox_ref.py's _u01
__device__ __forceinline__ float u01(unsigned w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-08f; }

// (wa, wb) -> two normals, the operations of elementwise.hip's philox_normal
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float& zc, float& zs) {
    const float r = sqrtf(-2.0f * logf(u01(wa)));
    const float ang = 6.283185307179586f * u01(wb);
    zc = r * cosf(ang);
    zs = r * sinf(ang);
}

}  // namespace spdm
