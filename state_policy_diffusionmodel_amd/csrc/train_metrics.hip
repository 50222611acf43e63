// train_metrics.hip -- the per-sample terms of a validation pass's loss, without a value leaving the device (spdm_loss_terms;
// DESIGN.md 8.12), and the per-frame terms of the autoencoder's (spdm_recon_terms; DESIGN.md 8.23, described at its kernel).
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

// spdm_recon_terms: the mean squared error of each frame of a validation batch against its reconstruction.
//
// Replaces: nn.MSELoss(recon, batch) of the autoencoder's validation_step (models/encoder/autoencoder.py:48, 64-71) as
// Lightning averages it over an epoch; every frame has 27648 elements, so that is the mean over the frames of these terms.
//
// ONE launch, one workgroup of 256 threads per frame.  Thread t owns quads t, t + 256, ..., t + 26 x 256 (a quad = four
// consecutive floats, one 16-byte load from each tensor; the 64 lanes of a wave read 1 KiB in a row) and keeps ONE float64
// partial over them, quads and elements in ascending order.  The 256 partials are combined by the tree of the header: the
// steps 128 and 64 cross waves and go through LDS (a double per thread, stride 8 bytes: conflict-free), the steps 32 .. 1
// are wave 0's shuffles.  Thread 0 divides by 27648 and writes the slot.  No atomics.
__global__ __launch_bounds__(RECON_THREADS) void recon_terms_kernel(const ReconTermsArgs a) {
    __shared__ double sh[RECON_THREADS];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * RECON_FRAME;                      // blockIdx.x < n
    const float4* recon = reinterpret_cast<const float4*>(a.recon + base);
    const float4* target = reinterpret_cast<const float4*>(a.target + base);
    constexpr int QUADS = RECON_FRAME / 4, PER_THREAD = QUADS / RECON_THREADS;  // 6912, 27
    static_assert(QUADS % RECON_THREADS == 0, "whole quads per thread");
    double p = 0.0;
#pragma unroll 9
    for (int k = 0; k < PER_THREAD; ++k) {
        const float4 r = recon[k * RECON_THREADS + t], g = target[k * RECON_THREADS + t];   // quad index < 6912
        const double d0 = (double)g.x - (double)r.x, d1 = (double)g.y - (double)r.y;
        const double d2 = (double)g.z - (double)r.z, d3 = (double)g.w - (double)r.w;
        p = p + d0 * d0;
        p = p + d1 * d1;
        p = p + d2 * d2;
        p = p + d3 * d3;
    }
    if (t >= 128) sh[t] = p;
    __syncthreads();
    if (t < 128) p = p + sh[t + 128];
    if (t >= 64 && t < 128) sh[t] = p;
    __syncthreads();
    if (t >= 64) return;                                                       // whole waves leave: wave 0 goes on
    p = p + sh[t + 64];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_down(p, off, 64);
    if (t == 0) a.terms[a.slot_offset + blockIdx.x] = p / (double)RECON_FRAME;
}

}  // namespace

hipError_t launch_recon_terms(const ReconTermsArgs& a, hipStream_t s) {
    if (a.n < 1 || a.slot_offset < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recon_terms_kernel, dim3((unsigned)a.n), dim3(RECON_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_loss_terms(const LossTermsArgs& a, hipStream_t s) {
    if (a.B < 1 || a.n < 1 || a.slot_offset < 0 || (a.slot_t != nullptr) != (a.t_in != nullptr)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(((long long)a.B + LOSS_WAVES - 1) / LOSS_WAVES);
    hipLaunchKernelGGL(loss_terms_kernel, dim3(grid), dim3(LOSS_WAVES * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdm
