// evaluation.hip -- position and action error of sampled trajectories against a dataset's windows, and the statistics of
// those errors, without a trajectory leaving the device (spdm_eval_errors, spdm_eval_reduce).
//
// Replaces: the per-window body of evaluation/eval_acurracy_diffusion_positions.py:118-140 and of
// evaluation/eval_consistency_diffusion_positions.py -- unnormalize_position (utils/data_utils.py:35-40) of the truth and of the
// prediction, np.linalg.norm(gt[0, obs_horizon:] - pred[inpaint_horizon:], axis=1), and the np.mean / np.std over the runs of
// a window and over all windows -- which the reference runs on the host after a .cpu() of every single trajectory.
//
// Errors: ONE launch, one thread per (trajectory, prediction step).  Every float64 operation is rounded on its own: FMA
// contraction is switched off for the whole file, because a fused a * b + c differs from numpy's two roundings.
// Statistics: per window, a thread per (window, column) sums the window's runs in run order, two-pass, which is bit for bit
// numpy's axis-0 reduction.  Over all rows, each workgroup reduces a block of ROWS_PER_BLOCK rows of one column in a fixed
// order (in thread: rows t, t + 256, ...; in wave: shuffles; across waves: LDS, wave order) and one thread per column adds the
// block partials in block order; the order is a pure function of (N, C), so two calls give the same bits.
//
// Safety: every index is built from scalars the host entry points have validated (include/spdm.h); no value read from device
// memory is used as an index.  No atomics.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "unnormalize.h"

#pragma clang fp contract(off)

namespace spdm {

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void eval_errors_kernel(const EvalErrorsArgs a) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;        // (trajectory, prediction step)
    if (g >= (long long)a.B * a.P) return;
    const int b = (int)(g / a.P), j = (int)(g - (long long)b * a.P);
    const long long slot = (a.first_traj + b) / a.runs - a.window_base;       // in [0, n_slots): checked by the host
    const size_t trow = (size_t)slot * a.seq + a.obs_h + j;                   // obs_h + j < seq
    const float* pred = a.pred + ((size_t)b * a.H + a.inp_h + j) * a.D;       // inp_h + j < H
    const double range = a.pos_max - a.pos_min;
    const double dx = unnormalize_position(a.truth_pos[trow * 2 + 0], a.translation[slot * 2 + 0], a.pos_min, range) -
                      unnormalize_position(pred[0], a.translation[slot * 2 + 0], a.pos_min, range);
    const double dy = unnormalize_position(a.truth_pos[trow * 2 + 1], a.translation[slot * 2 + 1], a.pos_min, range) -
                      unnormalize_position(pred[1], a.translation[slot * 2 + 1], a.pos_min, range);
    a.pos_err[g] = sqrt(dx * dx + dy * dy);
    if (a.act_err != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double r = a.act_max[c] - a.act_min[c];
            a.act_err[(size_t)g * 3 + c] = fabs(unnormalize_action(a.truth_act[trow * 3 + c], a.act_min[c], r) -
                                                unnormalize_action(pred[2 + c], a.act_min[c], r));
        }
    }
}

// np.mean / np.std(axis=0) of one window's (runs, C) rows: a sequential sum in run order, then the squared deviations
__global__ __launch_bounds__(THREADS) void eval_window_kernel(const EvalReduceArgs a) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;        // (window, column)
    if (g >= a.windows * a.C) return;
    const long long k = g / a.C;
    const int c = (int)(g - k * a.C);
    const double* x = a.err + (size_t)k * a.runs * a.C + c;
    double sum = x[0];
    for (int r = 1; r < a.runs; ++r) sum = sum + x[(size_t)r * a.C];
    const double mean = sum / (double)a.runs;
    double d = x[0] - mean;
    double sq = d * d;
    for (int r = 1; r < a.runs; ++r) {
        d = x[(size_t)r * a.C] - mean;
        sq = sq + d * d;
    }
    a.window_mean[g] = mean;
    a.window_std[g] = sqrt(sq / (double)a.runs);
}

// partial[c][blk] = sum over the block's rows of x (SECOND false) or of (x - mean[c])^2 (SECOND true)
template <bool SECOND>
__global__ __launch_bounds__(THREADS) void eval_partial_kernel(const EvalReduceArgs a) {
    __shared__ double sh[THREADS / 64];
    const int c = blockIdx.y;
    const long long row0 = (long long)blockIdx.x * EVAL_ROWS_PER_BLOCK;
    const double mean = SECOND ? a.mean[c] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < EVAL_ROWS_PER_BLOCK / THREADS; ++i) {
        const long long r = row0 + i * THREADS + threadIdx.x;
        if (r < a.N) {
            const double v = a.err[(size_t)r * a.C + c];
            const double d = v - mean;
            acc = acc + (SECOND ? d * d : v);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = sh[0];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) tot = tot + sh[w];
        a.workspace[(size_t)c * gridDim.x + blockIdx.x] = tot;
    }
}

// the block partials of a column added in block order: the mean (SECOND false) or the population std (SECOND true)
template <bool SECOND>
__global__ __launch_bounds__(THREADS) void eval_finish_kernel(const EvalReduceArgs a, int blocks) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= a.C) return;
    const double* p = a.workspace + (size_t)c * blocks;
    double tot = p[0];
    for (int i = 1; i < blocks; ++i) tot = tot + p[i];
    if (SECOND) a.std[c] = sqrt(tot / (double)a.N);
    else a.mean[c] = tot / (double)a.N;
}

}  // namespace

hipError_t launch_eval_errors(const EvalErrorsArgs& a, hipStream_t s) {
    const long long n = (long long)a.B * a.P;
    if (a.B < 1 || a.P < 1 || a.runs < 1 || n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(eval_errors_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_eval_reduce(const EvalReduceArgs& a, hipStream_t s) {
    const long long blocks = eval_reduce_blocks(a.N);
    const long long wc = a.windows * a.C;
    if (a.N < 1 || a.C < 1 || a.C > 65535 || a.runs < 1 || a.windows * a.runs != a.N || blocks > 0x7fffffffLL ||
        wc > 0x7fffffffLL * THREADS)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(eval_window_kernel, dim3((unsigned)((wc + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
    const dim3 grid((unsigned)blocks, (unsigned)a.C), cols((unsigned)((a.C + THREADS - 1) / THREADS));
    hipLaunchKernelGGL(eval_partial_kernel<false>, grid, dim3(THREADS), 0, s, a);
    hipLaunchKernelGGL(eval_finish_kernel<false>, cols, dim3(THREADS), 0, s, a, (int)blocks);
    hipLaunchKernelGGL(eval_partial_kernel<true>, grid, dim3(THREADS), 0, s, a);
    hipLaunchKernelGGL(eval_finish_kernel<true>, cols, dim3(THREADS), 0, s, a, (int)blocks);
    return hipGetLastError();
}

}  // namespace spdm
