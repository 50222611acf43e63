// train_metrics.hip -- the per-sample terms of a validation pass's loss, without a value leaving the device (spdm_loss_terms;
// DESIGN.md 8.12).
//
// Replaces: the body of the reference's validation_step (models/diffusion_ddpm.py:175-214, nn.MSELoss of :49 on one batch) as
// Lightning accumulates it over an epoch: the batch-size-weighted mean of the batch losses, which is the mean over the samples
// of each sample's own mean squared error when every sample has the same H x D elements.  This file forms those per-sample
// means; spdm_eval_reduce (evaluation.hip) takes their mean over the pass.
//
// ONE launch: one wave per sample, LOSS_WAVES samples per workgroup.  Lane l reads elements l, l + 64, l + 128, ... of the
// sample's H x D floats -- the 64 lanes of a wave read 64 consecutive floats, one 256-byte segment per request -- and keeps a
// float64 partial over them in ascending order; the 64 partials are combined by a fixed shuffle tree (offsets 32, 16, 8, 4, 2,
// 1: lane i takes lane i + offset), lane 0 divides by H x D and writes the slot.  The order is a function of H x D alone.  Every
// float64 operation is rounded on its own: FMA contraction is switched off for the whole file.  No LDS, no atomics, no barrier.
//
// Safety: every index is built from scalars the host entry point has validated (include/spdm.h); no value read from device
// memory is used as an index.
#include <hip/hip_runtime.h>

#include "kernels.h"

#pragma clang fp contract(off)

namespace spdm {

namespace {

__global__ __launch_bounds__(LOSS_WAVES * 64) void loss_terms_kernel(const LossTermsArgs a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * LOSS_WAVES + (threadIdx.x >> 6);               // the wave's sample: uniform over the wave
    if (b >= a.B) return;
    const float* eps = a.eps + (size_t)b * a.n;
    const float* noise = a.noise + (size_t)b * a.n;
    double acc = 0.0;
    for (int e = lane; e < a.n; e += 64) {
        const double d = (double)noise[e] - (double)eps[e];
        acc = acc + d * d;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    if (lane == 0) {
        a.terms[a.slot_offset + b] = acc / (double)a.n;
        if (a.slot_t != nullptr) a.slot_t[a.slot_offset + b] = a.t_in[b];
    }
}

}  // namespace

hipError_t launch_loss_terms(const LossTermsArgs& a, hipStream_t s) {
    if (a.B < 1 || a.n < 1 || a.slot_offset < 0 || (a.slot_t != nullptr) != (a.t_in != nullptr)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(((long long)a.B + LOSS_WAVES - 1) / LOSS_WAVES);
    hipLaunchKernelGGL(loss_terms_kernel, dim3(grid), dim3(LOSS_WAVES * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdm
