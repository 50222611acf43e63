// train_noise.hip -- the forward (noising) process of a training step on the device (spdm_train_forward_process),
// and the device-timestep hand-over of spdm_train_loss_grad_dt.
//
// Replaces: the head of Diffusion_DDPM.training_step (models/diffusion_ddpm.py:128-173): t = torch.randint(0, noise_steps, (B,)),
// noise = torch.randn_like(x), noise_scheduler.add_noise(x, noise, t), add_constraints (:216-219), and -- for simple_Unet.py's
// network -- the Dropout(p) mask of PositionalEncoding (:226-257).
//
// ONE launch, one workgroup per sample.  Randomness is Philox4x32-10 with key = (seed lo, seed hi) and counter
// (q, global sample index, training step, purpose): purpose 2 draws the timestep (q = 0, t = (w0 * T) >> 32), purpose 1 the
// noise (q = flat element / 4, the four words give four Box-Muller normals: ONE Philox per four elements), purpose 3 the
// dropout mask (q = column / 4, one word per column).  Purpose 0 is the sampler's stream (elementwise.hip) and is not drawn
// from here.  tests/forward_process_ref.py is the numpy restatement.
//
// No atomics, no cross-workgroup communication: two calls on the same arguments give the same bits.  The scheduler arithmetic
// is explicitly rounded (no FMA contraction), so x_noisy is torch's `sa * x0 + sb * noise` bit for bit.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "philox_normal.h"

namespace spdm {

namespace {

constexpr int THREADS = 128;

__device__ __forceinline__ int clamp_t(int t, int T) { return t < 0 ? 0 : (t >= T ? T - 1 : t); }

// Work items of sample b = blockIdx.x: noise quads [0, nq), then dropout quads [nq, nq + tq).  Workgroup 0 also counts the
// caller's out-of-range timesteps (fixed-order integer reduction).
__global__ __launch_bounds__(THREADS) void forward_process_kernel(const ForwardProcessArgs a) {
    __shared__ int sh_t;
    __shared__ int sh_cnt[THREADS / 64];
    const int b = blockIdx.x;                            // < a.B: the grid is exactly B workgroups
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
    const unsigned sample = (unsigned)(a.sample_offset + (unsigned long long)b);
    if (threadIdx.x == 0) {
        int t;
        if (a.t_in != nullptr) {
            t = clamp_t(a.t_in[b], a.T);                 // clamped BEFORE any table is read
        } else {
            unsigned w[4];
            philox4x32_10(0u, sample, a.step, 2u, k0, k1, w);
            t = (int)(((unsigned long long)w[0] * (unsigned long long)(unsigned)a.T) >> 32);      // in [0, T)
        }
        sh_t = t;
        if (a.t_out != nullptr && a.t_out != a.t_in) a.t_out[b] = t;
    }
    if (a.clamped != nullptr && b == 0) {                // uniform per workgroup
        int cnt = 0;
        if (a.t_in != nullptr)
            for (int i = threadIdx.x; i < a.B; i += THREADS) {
                const int v = a.t_in[i];
                cnt += (v < 0 || v >= a.T) ? 1 : 0;
            }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if ((threadIdx.x & 63) == 0) sh_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (a.clamped != nullptr && b == 0 && threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) tot += sh_cnt[w];
        *a.clamped = tot;
    }
    const int t = sh_t;                                  // in [0, T)
    const float sa = a.sqrt_abar[t], sb = a.sqrt_1m_abar[t];
    const int HD = a.H * a.D;
    const int nq = (HD + 3) >> 2;
    const int tq = a.time_scale != nullptr ? (a.time_dim + 3) >> 2 : 0;
    const size_t base = (size_t)b * HD;
    const int inp_e = a.inp_h * a.D;                     // elements [0, inp_e) of a window are the in-painted rows
    for (int i = threadIdx.x; i < nq + tq; i += THREADS) {
        if (i < nq) {
            const int e0 = i << 2;
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.noise_in == nullptr) {
                unsigned w[4];
                philox4x32_10((unsigned)i, sample, a.step, 1u, k0, k1, w);
                box_muller(w[0], w[1], z[0], z[1]);
                box_muller(w[2], w[3], z[2], z[3]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = e0 + k;
                if (e >= HD) break;
                const size_t idx = base + e;
                const float zz = a.noise_in != nullptr ? a.noise_in[idx] : z[k];
                if (a.noise_out != nullptr && a.noise_out != a.noise_in) a.noise_out[idx] = zz;
                float xn = __fadd_rn(__fmul_rn(sa, a.x0[idx]), __fmul_rn(sb, zz));
                if (e < inp_e) xn = a.inpaint[(size_t)b * inp_e + e];          // add_constraints
                a.x_noisy[idx] = xn;
            }
        } else {
            const int q = i - nq;
            unsigned w[4];
            philox4x32_10((unsigned)q, sample, a.step, 3u, k0, k1, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = (q << 2) + k;
                if (j >= a.time_dim) break;
                a.time_scale[(size_t)b * a.time_dim + j] = u01(w[k]) >= a.dropout_p ? a.keep_scale : 0.0f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void copy_t_clamped_kernel(const int* __restrict__ src, int n, int T, int* __restrict__ dst) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = clamp_t(src[i], T);
}

}  // namespace

hipError_t launch_forward_process(const ForwardProcessArgs& a, hipStream_t s) {
    if (a.B < 1 || a.H < 1 || a.D < 1 || a.T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(forward_process_kernel, dim3((unsigned)a.B), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_copy_t_clamped(const int* src, int n, int T, int* dst, hipStream_t s) {
    if (n < 1 || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_t_clamped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, n, T, dst);
    return hipGetLastError();
}

}  // namespace spdm
