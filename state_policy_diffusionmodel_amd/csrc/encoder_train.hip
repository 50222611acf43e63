// encoder_train.hip -- training pass of the observation encoder (models/encoder/autoencoder.py:11-20), which the reference
// optimises jointly with the U-Net: configure_optimizers is Adam(self.parameters()) (models/diffusion_ddpm.py:115-116) and
// prepare_obs_cond_vectors (:317-330) runs self.vision_encoder with autograd on.  DESIGN.md 8.6.
//
// The 2x2 stride-2 windows never overlap, so each convolution is a GEMM over space-to-depth rows and every contraction of the
// backward pass goes through the launchers training already has, all exact fp32 MFMA (spdm_api.hip: spdm_encoder_backward):
//     data gradients   launch_gemm on transposed weight copies       weight gradients   launch_wgrad (taps = 1)
//     bias gradients   launch_colsum
// This file supplies the layouts they read and what is too thin for a matrix-core tile:
//   - the training forward: encoder_convs_kernel's arithmetic, statement for statement (so the latents are the same bits), which
//     also keeps conv 2's map as conv 3's space-to-depth rows  x3[n][q][ci*4 + ky*2 + kx] = a2[n][ci][2qy+ky][2qx+kx];
//   - conv 1's map recomputed from the frames as conv 2's rows  x2[r][c1*4 + ky*2 + kx],  r = (n*144 + q)*4 + kk: the four
//     conv-2 positions of conv-3 window q are consecutive rows, so conv 3's data gradient becomes conv 2's output gradient by
//     a permutation inside each 128-float row.  Only conv-1 positions 0..47 appear: row / column 48 has no reader;
//   - the ReLU masks (saved post-activation value > 0, PyTorch's convention at 0) fused into those re-layouts, the saved
//     values' signs settled by a float64 evaluation of the pre-activations (encoder_kinks_kernel);
//   - conv 1's weight and bias gradient (K = 12): VALU, per-wave register accumulators, a fixed-order butterfly over the lanes,
//     one partial row per workgroup that launch_colsum adds in a fixed order.
// No float atomics anywhere: two calls on the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace spdm {
namespace {

constexpr int E_IN = 96, E_C1 = 16, E_C2 = 32, E_S2 = 24, E_C3 = 64, E_S3 = 12;
constexpr int E_Q = E_S3 * E_S3;              // 144 conv-3 positions
constexpr int E_FEAT = E_C3 * E_Q;            // 9216
constexpr int E_K3 = E_C2 * 4;                // 128
constexpr int E_K2 = E_C1 * 4;                // 64

// the 4x4 input patch (3 channels) of conv-2 position (py, px): input rows 4 py - 1 .. 4 py + 2, zero padding outside the image
__device__ __forceinline__ void load_patch(const float* __restrict__ im, int py, int px, float (&p)[3][4][4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int dy = 0; dy < 4; ++dy)
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                const int iy = 4 * py - 1 + dy, ix = 4 * px - 1 + dx;
                p[c][dy][dx] = (iy >= 0 && iy < E_IN && ix >= 0 && ix < E_IN) ? im[((size_t)c * E_IN + iy) * E_IN + ix] : 0.f;
            }
}

// conv 1 + ReLU, channel c1, at the conv-1 position (ky, kx) of the patch -- the forward's accumulation order
__device__ __forceinline__ float conv1_at(const float* __restrict__ w1, const float* __restrict__ b1, int c1, int ky, int kx,
                                          const float (&p)[3][4][4]) {
    float a = b1[c1];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int jy = 0; jy < 2; ++jy)
#pragma unroll
            for (int jx = 0; jx < 2; ++jx) a = fmaf(w1[((c1 * 3 + c) * 2 + jy) * 2 + jx], p[c][2 * ky + jy][2 * kx + jx], a);
    return fmaxf(a, 0.f);
}

// encoder_convs_kernel (encoder.hip) with conv 2's map kept: one workgroup per image
__global__ __launch_bounds__(256) void encoder_train_convs_kernel(const float* __restrict__ img, const float* __restrict__ w1,
                                                                  const float* __restrict__ b1, const float* __restrict__ w2,
                                                                  const float* __restrict__ b2, const float* __restrict__ w3,
                                                                  const float* __restrict__ b3, float* __restrict__ feat,
                                                                  float* __restrict__ x3) {           // [n][144][128]
    extern __shared__ float s2[];                     // [32][24][24] conv-2 map after ReLU
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* im = img + (size_t)n * 3 * E_IN * E_IN;
    for (int p = tid; p < E_S2 * E_S2; p += 256) {
        const int py = p / E_S2, px = p - py * E_S2;
        float px_in[3][4][4];
        load_patch(im, py, px, px_in);
        float acc[E_C2];
#pragma unroll
        for (int o = 0; o < E_C2; ++o) acc[o] = b2[o];
        for (int c1 = 0; c1 < E_C1; ++c1) {
            float v[2][2];
#pragma unroll
            for (int ky = 0; ky < 2; ++ky)
#pragma unroll
                for (int kx = 0; kx < 2; ++kx) v[ky][kx] = conv1_at(w1, b1, c1, ky, kx, px_in);
#pragma unroll
            for (int o = 0; o < E_C2; ++o) {
                const float* w = w2 + ((size_t)o * E_C1 + c1) * 4;
                acc[o] = fmaf(w[0], v[0][0], acc[o]);
                acc[o] = fmaf(w[1], v[0][1], acc[o]);
                acc[o] = fmaf(w[2], v[1][0], acc[o]);
                acc[o] = fmaf(w[3], v[1][1], acc[o]);
            }
        }
#pragma unroll
        for (int o = 0; o < E_C2; ++o) s2[o * (E_S2 * E_S2) + p] = fmaxf(acc[o], 0.f);
    }
    __syncthreads();
    float* f = feat + (size_t)n * E_FEAT;
    for (int idx = tid; idx < E_FEAT; idx += 256) {
        const int co = idx / E_Q, q = idx - co * E_Q;
        const int qy = q / E_S3, qx = q - qy * E_S3;
        float a = b3[co];
        const float* w = w3 + (size_t)co * E_C2 * 4;
        for (int ci = 0; ci < E_C2; ++ci) {
            const float* sp = s2 + ci * (E_S2 * E_S2) + (2 * qy) * E_S2 + 2 * qx;
            a = fmaf(w[ci * 4 + 0], sp[0], a);
            a = fmaf(w[ci * 4 + 1], sp[1], a);
            a = fmaf(w[ci * 4 + 2], sp[E_S2], a);
            a = fmaf(w[ci * 4 + 3], sp[E_S2 + 1], a);
        }
        f[idx] = fmaxf(a, 0.f);
    }
    // ---- the saved conv-2 map, as conv 3's space-to-depth rows ----
    float* xs = x3 + (size_t)n * (E_Q * E_K3);
    for (int idx = tid; idx < E_Q * E_K3; idx += 256) {
        const int q = idx / E_K3, k = idx - q * E_K3;
        const int qy = q / E_S3, qx = q - qy * E_S3, ci = k >> 2, ky = (k >> 1) & 1, kx = k & 1;
        xs[idx] = s2[ci * (E_S2 * E_S2) + (2 * qy + ky) * E_S2 + 2 * qx + kx];
    }
}

// conv 1's pre-activation in float64 (frames and weights are exact in float64, so this is the exact network's value to 1e-16)
__device__ __forceinline__ double conv1_pre64(const float* __restrict__ w1, const float* __restrict__ b1, int c1, int ky, int kx,
                                              const float (&p)[3][4][4]) {
    double a = (double)b1[c1];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int jy = 0; jy < 2; ++jy)
#pragma unroll
            for (int jx = 0; jx < 2; ++jx)
                a = fma((double)w1[((c1 * 3 + c) * 2 + jy) * 2 + jx], (double)p[c][2 * ky + jy][2 * kx + jx], a);
    return a;
}
// a saved fp32 activation whose sign the float64 evaluation contradicts: the smallest normal number where the exact
// pre-activation is positive (mask on, value 1e-38), zero where it is not
__device__ __forceinline__ float kink_value(float a32, bool on64) { return on64 ? fmaxf(a32, 1.17549435e-38f) : 0.f; }

// ReLU kinks decided in float64.  The fp32 forward rounds a pre-activation that lies within ~1e-7 of zero to either side, and a
// unit on the wrong side of its kink carries a whole unit's gradient: about one unit in 2e7 does, enough to move a conv-2
// weight gradient by 3e-4 at 2000 frames (torch's fp32 autograd has the same spread against float64).  This kernel evaluates the
// three convolutions of a frame again in float64 -- the fp32 kernel's structure, conv 2's map in LDS as doubles -- and where the
// sign of a float64 pre-activation disagrees with the saved fp32 activation it rewrites THE SAVED COPY (x3, feat) with
// kink_value: the backward pass, which reads its masks as "saved > 0", then differentiates the exactly evaluated network.
// Runs after the Linear layer has read feat, so the latents stay the fp32 forward's bits.  One workgroup per frame.
__global__ __launch_bounds__(256) void encoder_kinks_kernel(const float* __restrict__ img, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, const float* __restrict__ w3,
                                                            const float* __restrict__ b3, float* __restrict__ feat,
                                                            float* __restrict__ x3) {
    extern __shared__ double d2[];                    // [32][24][24] conv-2 map after ReLU, float64
    const int n = blockIdx.x, tid = threadIdx.x;
    const float* im = img + (size_t)n * 3 * E_IN * E_IN;
    float* xs = x3 + (size_t)n * (E_Q * E_K3);
    for (int p = tid; p < E_S2 * E_S2; p += 256) {
        const int py = p / E_S2, px = p - py * E_S2;
        float px_in[3][4][4];
        load_patch(im, py, px, px_in);
        double acc[E_C2];
#pragma unroll
        for (int o = 0; o < E_C2; ++o) acc[o] = (double)b2[o];
        for (int c1 = 0; c1 < E_C1; ++c1) {
            double v[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) v[kk] = fmax(conv1_pre64(w1, b1, c1, kk >> 1, kk & 1, px_in), 0.0);
#pragma unroll
            for (int o = 0; o < E_C2; ++o) {
                const float* w = w2 + ((size_t)o * E_C1 + c1) * 4;
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[o] = fma((double)w[kk], v[kk], acc[o]);
            }
        }
        const int q = (py >> 1) * E_S3 + (px >> 1), kk = (py & 1) * 2 + (px & 1);
#pragma unroll
        for (int o = 0; o < E_C2; ++o) {
            d2[o * (E_S2 * E_S2) + p] = fmax(acc[o], 0.0);
            float* sv = xs + q * E_K3 + o * 4 + kk;
            const float a32 = *sv;
            if ((acc[o] > 0.0) != (a32 > 0.f)) *sv = kink_value(a32, acc[o] > 0.0);
        }
    }
    __syncthreads();
    float* f = feat + (size_t)n * E_FEAT;
    for (int idx = tid; idx < E_FEAT; idx += 256) {
        const int co = idx / E_Q, q = idx - co * E_Q;
        const int qy = q / E_S3, qx = q - qy * E_S3;
        double a = (double)b3[co];
        const float* w = w3 + (size_t)co * E_C2 * 4;
        for (int ci = 0; ci < E_C2; ++ci) {
            const double* sp = d2 + ci * (E_S2 * E_S2) + (2 * qy) * E_S2 + 2 * qx;
            a = fma((double)w[ci * 4 + 0], sp[0], a);
            a = fma((double)w[ci * 4 + 1], sp[1], a);
            a = fma((double)w[ci * 4 + 2], sp[E_S2], a);
            a = fma((double)w[ci * 4 + 3], sp[E_S2 + 1], a);
        }
        const float a32 = f[idx];
        if ((a > 0.0) != (a32 > 0.f)) f[idx] = kink_value(a32, a > 0.0);
    }
}

// conv-2 position of row r of a frame's 576 rows (r = q * 4 + kk)
__device__ __forceinline__ void row_pos(int r, int* py, int* px) {
    const int q = r >> 2, kk = r & 3, qy = q / E_S3, qx = q - qy * E_S3;
    *py = 2 * qy + (kk >> 1);
    *px = 2 * qx + (kk & 1);
}

// x2[row][c1*4 + ky*2 + kx] = ReLU(conv 1) recomputed from the frames (its sign from float64): one row per thread
__global__ __launch_bounds__(256) void enc_x2_kernel(const float* __restrict__ img, const float* __restrict__ w1,
                                                     const float* __restrict__ b1, long long rows, float* __restrict__ x2) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const long long n = row / (E_S2 * E_S2);
    int py, px;
    row_pos((int)(row - n * (E_S2 * E_S2)), &py, &px);
    float p[3][4][4];
    load_patch(img + (size_t)n * 3 * E_IN * E_IN, py, px, p);
    float4* out = reinterpret_cast<float4*>(x2 + (size_t)row * E_K2);
    for (int c1 = 0; c1 < E_C1; ++c1) {
        float v[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            v[kk] = conv1_at(w1, b1, c1, kk >> 1, kk & 1, p);
            v[kk] = kink_value(v[kk], conv1_pre64(w1, b1, c1, kk >> 1, kk & 1, p) > 0.0);     // the kink in float64 (encoder_kinks_kernel)
        }
        out[c1] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// dz3[n*144 + q][co] = dfeat[n][co*144 + q] where feat[n][co*144 + q] > 0: Flatten order -> channels-last rows, through LDS
__global__ __launch_bounds__(256) void enc_dz3_kernel(const float* __restrict__ dfeat, const float* __restrict__ feat,
                                                      float* __restrict__ dz3) {
    __shared__ float t[E_FEAT];
    const size_t base = (size_t)blockIdx.x * E_FEAT;
    for (int i = threadIdx.x; i < E_FEAT; i += 256) t[i] = feat[base + i] > 0.f ? dfeat[base + i] : 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < E_FEAT; i += 256) {
        const int q = i / E_C3, co = i - q * E_C3;
        dz3[base + i] = t[co * E_Q + q];
    }
}

// dz2[nq*4 + kk][ci] = dx3[nq][ci*4 + kk] where x3[nq][ci*4 + kk] > 0 (a permutation inside each 128-float row)
__global__ __launch_bounds__(256) void enc_dz2_kernel(const float* __restrict__ dx3, const float* __restrict__ x3, size_t total,
                                                      float* __restrict__ dz2) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int o = (int)(i & (E_K3 - 1)), kk = o >> 5, ci = o & 31;
    const size_t src = (i - o) + ci * 4 + kk;
    dz2[i] = x3[src] > 0.f ? dx3[src] : 0.f;
}

// conv 1's weight and bias gradient.  dz1[row][c1*4 + kk] = dx2[row][.] where x2[row][.] > 0 is the gradient at conv-1 position
// kk of the row's patch.  Workgroup = 4 waves x ENC_W1_ROWS rows; wave w owns channels 4 w .. 4 w + 3 and accumulates
// its 4 x 12 weights + 4 biases in registers over the workgroup's rows (lane l: rows l, l + 64, ... ascending), then adds the 64
// lanes by a butterfly.  part[workgroup][16*12 weights | 16 biases].
constexpr int ENC_W1_ROWS = 1024, ENC_W1_LD = E_C1 * 12 + E_C1;
__global__ __launch_bounds__(256) void enc_conv1_wgrad_kernel(const float* __restrict__ img, const float* __restrict__ dx2,
                                                              const float* __restrict__ x2, long long rows,
                                                              float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float acc[4][12], bacc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        bacc[a] = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) acc[a][k] = 0.f;
    }
    const long long r0 = (long long)blockIdx.x * ENC_W1_ROWS;
    for (int it = 0; it < ENC_W1_ROWS / 64; ++it) {
        const long long row = r0 + it * 64 + lane;
        if (row >= rows) break;
        const long long n = row / (E_S2 * E_S2);
        int py, px;
        row_pos((int)(row - n * (E_S2 * E_S2)), &py, &px);
        float p[3][4][4];
        load_patch(img + (size_t)n * 3 * E_IN * E_IN, py, px, p);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const size_t o = (size_t)row * E_K2 + (wave * 4 + a) * 4;
            const float4 g4 = *reinterpret_cast<const float4*>(dx2 + o), v4 = *reinterpret_cast<const float4*>(x2 + o);
            const float g[4] = {v4.x > 0.f ? g4.x : 0.f, v4.y > 0.f ? g4.y : 0.f, v4.z > 0.f ? g4.z : 0.f, v4.w > 0.f ? g4.w : 0.f};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                bacc[a] += g[kk];
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[a][c * 4 + j] = fmaf(g[kk], p[c][2 * (kk >> 1) + (j >> 1)][2 * (kk & 1) + (j & 1)], acc[a][c * 4 + j]);
            }
        }
    }
    float* out = part + (size_t)blockIdx.x * ENC_W1_LD;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
        for (int k = 0; k < 13; ++k) {
            float v = k < 12 ? acc[a][k] : bacc[a];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
            if (lane == 0) {
                if (k < 12) out[(wave * 4 + a) * 12 + k] = v;
                else out[E_C1 * 12 + wave * 4 + a] = v;
            }
        }
    }
}

// dst[c][r] = src[r][c]
__global__ void enc_add_kernel(const float* __restrict__ src, size_t n, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

inline unsigned blocks_of(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

hipError_t launch_encoder_train_convs(const float* img, const float* w1, const float* b1, const float* w2, const float* b2,
                                      const float* w3, const float* b3, float* feat, float* x3, int n_images, hipStream_t s) {
    if (n_images <= 0 || !img || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !feat || !x3) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * E_C2 * E_S2 * E_S2;
    if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(encoder_train_convs_kernel)); e != hipSuccess) return e;
    hipLaunchKernelGGL(encoder_train_convs_kernel, dim3(n_images), dim3(256), lds, s, img, w1, b1, w2, b2, w3, b3, feat, x3);
    return hipGetLastError();
}

hipError_t launch_encoder_kinks(const float* img, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* w3, const float* b3, float* feat, float* x3, int n_images, hipStream_t s) {
    if (n_images <= 0 || !img || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !feat || !x3) return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * E_C2 * E_S2 * E_S2;                // 147,456 bytes
    if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(encoder_kinks_kernel)); e != hipSuccess) return e;
    hipLaunchKernelGGL(encoder_kinks_kernel, dim3(n_images), dim3(256), lds, s, img, w1, b1, w2, b2, w3, b3, feat, x3);
    return hipGetLastError();
}

hipError_t launch_encoder_x2(const float* img, const float* w1, const float* b1, int n_images, float* x2, hipStream_t s) {
    if (n_images <= 0 || !img || !w1 || !b1 || !x2) return hipErrorInvalidValue;
    const long long rows = (long long)n_images * E_S2 * E_S2;
    hipLaunchKernelGGL(enc_x2_kernel, dim3(blocks_of((size_t)rows, 256)), dim3(256), 0, s, img, w1, b1, rows, x2);
    return hipGetLastError();
}

hipError_t launch_encoder_dz3(const float* dfeat, const float* feat, int n_images, float* dz3, hipStream_t s) {
    if (n_images <= 0 || !dfeat || !feat || !dz3) return hipErrorInvalidValue;
    hipLaunchKernelGGL(enc_dz3_kernel, dim3(n_images), dim3(256), 0, s, dfeat, feat, dz3);
    return hipGetLastError();
}

hipError_t launch_encoder_dz2(const float* dx3, const float* x3, int n_images, float* dz2, hipStream_t s) {
    if (n_images <= 0 || !dx3 || !x3 || !dz2) return hipErrorInvalidValue;
    const size_t total = (size_t)n_images * E_Q * E_K3;
    hipLaunchKernelGGL(enc_dz2_kernel, dim3(blocks_of(total, 256)), dim3(256), 0, s, dx3, x3, total, dz2);
    return hipGetLastError();
}

int encoder_conv1_wgrad_blocks(int n_images) {
    return (int)(((long long)n_images * E_S2 * E_S2 + ENC_W1_ROWS - 1) / ENC_W1_ROWS);
}

hipError_t launch_encoder_conv1_wgrad(const float* img, const float* dx2, const float* x2, int n_images, float* part,
                                      float* dw, float* db, hipStream_t s) {
    if (n_images <= 0 || !img || !dx2 || !x2 || !part || !dw || !db) return hipErrorInvalidValue;
    const long long rows = (long long)n_images * E_S2 * E_S2;
    const int nblk = encoder_conv1_wgrad_blocks(n_images);
    hipLaunchKernelGGL(enc_conv1_wgrad_kernel, dim3(nblk), dim3(256), 0, s, img, dx2, x2, rows, part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (hipError_t e = launch_colsum(part, ENC_W1_LD, nblk, E_C1 * 12, dw, s); e != hipSuccess) return e;
    return launch_colsum(part + E_C1 * 12, ENC_W1_LD, nblk, E_C1, db, s);
}

hipError_t launch_add(const float* src, size_t n, float* dst, hipStream_t s) {
    if (n == 0 || !src || !dst) return hipErrorInvalidValue;
    hipLaunchKernelGGL(enc_add_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, src, n, dst);
    return hipGetLastError();
}

}  // namespace spdm
