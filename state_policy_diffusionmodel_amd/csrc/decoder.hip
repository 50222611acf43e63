// decoder.hip -- the decoder of the observation autoencoder (models/encoder/autoencoder.py:23-32) and its reconstruction
// training (MSELoss(recon, batch), :48,55-58): Linear(128, 9216) Unflatten(64,12,12) ConvTranspose2d(64,32,2,2) ReLU
// ConvTranspose2d(32,16,2,2) ReLU ConvTranspose2d(16,3,2,2) Sigmoid.  DESIGN.md 8.7.
//
// The 2x2 stride-2 windows never overlap, so a transposed convolution is a GEMM per input pixel: a row of K channels gives
// 4 Cout outputs, column kk * Cout + co (kk = ky * 2 + kx).  Row orders, all channels-last:
//     h0 [n*144][64]    the Linear's output, its weight rows permuted at load from Flatten order c*144 + q to q*64 + c
//     a1 [n*576][32]    row r2 = (n*144 + q)*4 + kk1   = layer 2's [n*144][128] result with no data movement
//     a2 [n*2304][16]   row r3 = r2*4 + kk2            = layer 4's [n*576][64] result likewise
//     recon NCHW        pixel (8 qy + 4 ky1 + 2 ky2 + ky3, 8 qx + 4 kx1 + 2 kx2 + kx3)
// The Linear and the wide contractions of the backward pass go through the launchers training already has (spdm_api.hip:
// launch_gemm, launch_wgrad with its slab budget capped so that thin layers get long slabs); this file supplies
//   - the three transposed convolutions of a frame in one workgroup (VALU: K = 64 / 32 / 16 against wave-uniform weights from
//     scalar loads), a1 in LDS, a2 in registers; the training variant is the same template, statement for statement, and also
//     stores a1, a2 and the frame's sum of squared errors (float64);
//   - the loss: the per-frame sums added in a fixed order;
//   - layer 6 backwards: dz6 recomputed from recon and target, its weight / bias gradient in per-thread registers (a fixed
//     butterfly, one partial row per frame, then launch_colsum), and dz4 under a2's ReLU mask;
//   - layer 4's data gradient (K = 64 -> 32: below launch_gemm's 64-column tiles) under a1's ReLU mask;
//   - a two-level column sum for the bias gradients (thin matrices over very many rows) that also folds the four kk columns of
//     a channel, and the permutations back to torch layout.
//   - the saved maps' ReLU signs settled by a float64 evaluation of the pre-activations (decoder_kinks_kernel).
// ReLU masks are "saved value > 0" (PyTorch's convention at 0).  No float atomics: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"

namespace spdm {
namespace {

constexpr int D_Q = 144, D_C0 = 64, D_C1 = 32, D_C2 = 16, D_OUT = 96;
constexpr int D_P1 = 576;                       // positions of the 24 x 24 map (layer 2's output)
constexpr int D_S1 = D_C1 + 1;                  // LDS row of a1: 33 floats, so that lanes on consecutive positions hit distinct banks
constexpr int D_PIX = 3 * D_OUT * D_OUT;        // 27648 values per frame
constexpr int D_W6_LD = 16 * 12 + 16;           // partial row of layer 6: 192 weights (torch order) | 3 biases | padding

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// row r2 (within the frame) of position p = py * 24 + px of the 24 x 24 map
__device__ __forceinline__ int row_of_pos(int py, int px) { return ((py >> 1) * 12 + (px >> 1)) * 4 + (py & 1) * 2 + (px & 1); }

// One workgroup per frame.  Weights in kernel layout: w2 [64][4][32], w4 [32][4][16], w6 [16][4][3] = [ci][kk][co].
//   phase A  wave w computes window position kk1 = w of every q (lane = q): 32 channels from h0's 64, into LDS by map position
//   phase B  wave w takes ky2 = w & 1 of half w >> 1 of the 576 positions (lane = position, so a wave's stores run along pixel
//            rows), both kx2: 16 channels from a1's 32, then layer 6 and the sigmoid from registers: 4 x 4 pixels x 3 channels,
//            stored as float4 along x
template <bool TRAIN>
__global__ __launch_bounds__(256) void decoder_convs_kernel(const float* __restrict__ h0, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, const float* __restrict__ w4,
                                                            const float* __restrict__ b4, const float* __restrict__ w6,
                                                            const float* __restrict__ b6, float* __restrict__ recon,
                                                            const float* __restrict__ target, float* __restrict__ a1s,
                                                            float* __restrict__ a2s, double* __restrict__ sq) {
    extern __shared__ __align__(16) float s1[];       // [576][33] layer 2's map after ReLU, by position
    const size_t n = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = wave_id();
    {
        const int kk1 = wave;
        for (int q = lane; q < D_Q; q += 64) {
            const float4* hr = reinterpret_cast<const float4*>(h0 + (n * D_Q + q) * D_C0);
            float acc[D_C1];
#pragma unroll
            for (int co = 0; co < D_C1; ++co) acc[co] = b2[co];
            for (int c4 = 0; c4 < D_C0 / 4; ++c4) {
                const float4 v4 = hr[c4];
                const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* w = w2 + ((c4 * 4 + i) * 4 + kk1) * D_C1;
#pragma unroll
                    for (int co = 0; co < D_C1; ++co) acc[co] = fmaf(w[co], v[i], acc[co]);
                }
            }
#pragma unroll
            for (int co = 0; co < D_C1; ++co) acc[co] = fmaxf(acc[co], 0.f);
            const int qy = q / 12, qx = q - qy * 12;
            float* sp = s1 + ((2 * qy + (kk1 >> 1)) * 24 + 2 * qx + (kk1 & 1)) * D_S1;
#pragma unroll
            for (int co = 0; co < D_C1; ++co) sp[co] = acc[co];
            if constexpr (TRAIN) {
                float4* o = reinterpret_cast<float4*>(a1s + ((n * D_Q + q) * 4 + kk1) * D_C1);
#pragma unroll
                for (int c = 0; c < D_C1 / 4; ++c) o[c] = make_float4(acc[4 * c], acc[4 * c + 1], acc[4 * c + 2], acc[4 * c + 3]);
            }
        }
    }
    __syncthreads();
    const int ky2 = wave & 1, half = wave >> 1;
    double err = 0.0;
    for (int p = half * (D_P1 / 2) + lane; p < (half + 1) * (D_P1 / 2); p += 64) {
        const int py = p / 24, px = p - py * 24;
        float a[D_C1];
#pragma unroll
        for (int ci = 0; ci < D_C1; ++ci) a[ci] = s1[p * D_S1 + ci];
        float o[2][4][3];
#pragma unroll
        for (int kx2 = 0; kx2 < 2; ++kx2) {
            const int kk2 = ky2 * 2 + kx2;
            float c[D_C2];
#pragma unroll
            for (int co = 0; co < D_C2; ++co) c[co] = b4[co];
#pragma unroll
            for (int ci = 0; ci < D_C1; ++ci) {
                const float* w = w4 + (ci * 4 + kk2) * D_C2;
#pragma unroll
                for (int co = 0; co < D_C2; ++co) c[co] = fmaf(w[co], a[ci], c[co]);
            }
#pragma unroll
            for (int co = 0; co < D_C2; ++co) c[co] = fmaxf(c[co], 0.f);
            if constexpr (TRAIN) {
                float4* sv = reinterpret_cast<float4*>(a2s + ((n * D_P1 + row_of_pos(py, px)) * 4 + kk2) * D_C2);
#pragma unroll
                for (int k = 0; k < D_C2 / 4; ++k) sv[k] = make_float4(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]);
            }
#pragma unroll
            for (int kk3 = 0; kk3 < 4; ++kk3)
#pragma unroll
                for (int co = 0; co < 3; ++co) {
                    float z = b6[co];
#pragma unroll
                    for (int ci = 0; ci < D_C2; ++ci) z = fmaf(w6[(ci * 4 + kk3) * 3 + co], c[ci], z);
                    o[kx2][kk3][co] = 1.f / (1.f + expf(-z));
                }
        }
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int ky3 = 0; ky3 < 2; ++ky3) {
                const size_t at = ((n * 3 + co) * D_OUT + 4 * py + 2 * ky2 + ky3) * D_OUT + 4 * px;
                const float4 r = make_float4(o[0][ky3 * 2][co], o[0][ky3 * 2 + 1][co], o[1][ky3 * 2][co], o[1][ky3 * 2 + 1][co]);
                *reinterpret_cast<float4*>(recon + at) = r;
                if constexpr (TRAIN) {
                    const float4 t = *reinterpret_cast<const float4*>(target + at);
                    const float d0 = r.x - t.x, d1 = r.y - t.y, d2 = r.z - t.z, d3 = r.w - t.w;
                    err += (double)d0 * d0;
                    err += (double)d1 * d1;
                    err += (double)d2 * d2;
                    err += (double)d3 * d3;
                }
            }
    }
    if constexpr (TRAIN) {      // the frame's sum: a butterfly over the lanes, then the four waves in order
        __syncthreads();        // (s1 has been read: its first bytes carry the four wave sums; no static LDS beside the dynamic 76 KB)
        double* red = reinterpret_cast<double*>(s1);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) err += __shfl_xor(err, m, 64);
        if (lane == 0) red[wave] = err;
        __syncthreads();
        if (threadIdx.x == 0) sq[n] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// ReLU kinks decided in float64.  The fp32 forward rounds a pre-activation that lies within ~1e-8 of zero
// to either side, and a unit on the wrong side of its kink carries a whole unit's gradient: one such a1 unit among the 2.4
// million of 130 frames moved 0.weight / 2.weight / d loss / d latent by 2-4e-4 (torch's fp32 autograd misses float64 by the
// same amount on that input).  This kernel evaluates the Linear and the two ReLU layers again in float64 from the latents --
// every q of a frame is independent of the others, so a workgroup takes 16 of them -- and where the sign of a float64
// pre-activation disagrees with the SAVED fp32 activation it rewrites the saved copy (a1s, a2s): the smallest normal number
// where the exact unit is on, zero where it is off.  The backward pass, which reads its masks as "saved > 0", then
// differentiates the exactly evaluated network.  The reconstruction and the loss are the fp32 forward's, untouched.
constexpr int DK_Q = 16;                           // q per workgroup: 144 / 16 = 9 workgroups per frame
__device__ __forceinline__ float kink_value(float a32, bool on64) { return on64 ? fmaxf(a32, 1.17549435e-38f) : 0.f; }
__global__ __launch_bounds__(256) void decoder_kinks_kernel(const float* __restrict__ latent, const float* __restrict__ w0,
                                                            const float* __restrict__ b0, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, const float* __restrict__ w4,
                                                            const float* __restrict__ b4, float* __restrict__ a1s,
                                                            float* __restrict__ a2s) {
    __shared__ double zs[128];                     // the frame's latent
    __shared__ double hs[DK_Q][D_C0];              // h0 of the workgroup's q
    __shared__ double as[DK_Q * 4][D_C1];          // a1 after ReLU, position q_local*4 + kk1
    const size_t n = blockIdx.x;
    const int q0 = blockIdx.y * DK_Q, t = threadIdx.x;
    if (t < 128) zs[t] = (double)latent[n * 128 + t];
    __syncthreads();
    for (int o = t; o < DK_Q * D_C0; o += 256) {               // h0[q][c] = b0 + sum_k z[k] w0[q*64 + c][k]
        const int row = q0 * D_C0 + o;
        const float4* w = reinterpret_cast<const float4*>(w0 + (size_t)row * 128);
        double a = (double)b0[row];
        for (int k4 = 0; k4 < 32; ++k4) {
            const float4 v = w[k4];
            a = fma((double)v.x, zs[4 * k4], a);
            a = fma((double)v.y, zs[4 * k4 + 1], a);
            a = fma((double)v.z, zs[4 * k4 + 2], a);
            a = fma((double)v.w, zs[4 * k4 + 3], a);
        }
        hs[o / D_C0][o % D_C0] = a;
    }
    __syncthreads();
    {                                                          // layer 2: thread = (position, 8 of the 32 channels)
        const int pos = t >> 2, ql = pos >> 2, kk1 = pos & 3, c0 = (t & 3) * 8;
        double acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = (double)b2[c0 + j];
        for (int ci = 0; ci < D_C0; ++ci) {
            const double x = hs[ql][ci];
            const float* w = w2 + (ci * 4 + kk1) * D_C1 + c0;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fma((double)w[j], x, acc[j]);
        }
        float* sv = a1s + ((n * D_Q + q0 + ql) * 4 + kk1) * D_C1 + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            as[pos][c0 + j] = fmax(acc[j], 0.0);
            const float a32 = sv[j];
            if ((acc[j] > 0.0) != (a32 > 0.f)) sv[j] = kink_value(a32, acc[j] > 0.0);
        }
    }
    __syncthreads();
    {                                                          // layer 4: thread = (position, kk2), 16 channels
        const int pos = t >> 2, kk2 = t & 3;
        double acc[D_C2];
#pragma unroll
        for (int j = 0; j < D_C2; ++j) acc[j] = (double)b4[j];
        for (int ci = 0; ci < D_C1; ++ci) {
            const double x = as[pos][ci];
            const float* w = w4 + (ci * 4 + kk2) * D_C2;
#pragma unroll
            for (int j = 0; j < D_C2; ++j) acc[j] = fma((double)w[j], x, acc[j]);
        }
        float* sv = a2s + (((n * D_Q + q0) * 4 + pos) * 4 + kk2) * D_C2;        // row r3 = r2*4 + kk2, r2 = (n*144 + q)*4 + kk1
#pragma unroll
        for (int j = 0; j < D_C2; ++j) {
            const float a32 = sv[j];
            if ((acc[j] > 0.0) != (a32 > 0.f)) sv[j] = kink_value(a32, acc[j] > 0.0);
        }
    }
}

// loss = sum over frames (thread t: frames t, t + 256, ... ascending; then a fixed tree) / (n 27648)
__global__ __launch_bounds__(256) void decoder_loss_kernel(const double* __restrict__ sq, int n, float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += sq[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] / ((double)n * D_PIX));
}

// Layer 6 backwards, one workgroup per frame in phase B's thread mapping.  dz6 = scale (recon - target) recon (1 - recon),
// scale = 2 / (n 27648), recomputed from the saved reconstruction; per thread acc[ci][kk3*3 + co] += a2[ci] dz6[.] over its rows
// in a fixed order, dz4[r3][ci] = (a2 > 0) sum_j dz6[j] w6[ci][j].  part[frame]: 192 weights in torch order ci*12 + co*4 + kk3 | 3 biases.
__global__ __launch_bounds__(256) void decoder_bwd6_kernel(const float* __restrict__ recon, const float* __restrict__ target,
                                                           const float* __restrict__ a2s, const float* __restrict__ w6,
                                                           float scale, float* __restrict__ dz4, float* __restrict__ part) {
    __shared__ float red[4][D_C2 * 12 + 12];
    const size_t n = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int ky2 = wave & 1, half = wave >> 1;
    float acc[D_C2][12], dzs[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        dzs[j] = 0.f;
#pragma unroll
        for (int ci = 0; ci < D_C2; ++ci) acc[ci][j] = 0.f;
    }
    for (int p = half * (D_P1 / 2) + lane; p < (half + 1) * (D_P1 / 2); p += 64) {
        const int py = p / 24, px = p - py * 24;
        float g[2][12];                                // dz6 of the thread's two rows (kx2), column kk3*3 + co
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int ky3 = 0; ky3 < 2; ++ky3) {
                const size_t at = ((n * 3 + co) * D_OUT + 4 * py + 2 * ky2 + ky3) * D_OUT + 4 * px;
                const float4 r4 = *reinterpret_cast<const float4*>(recon + at), t4 = *reinterpret_cast<const float4*>(target + at);
                const float r[4] = {r4.x, r4.y, r4.z, r4.w}, t[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) g[i >> 1][(ky3 * 2 + (i & 1)) * 3 + co] = (scale * (r[i] - t[i])) * (r[i] * (1.f - r[i]));
            }
#pragma unroll
        for (int kx2 = 0; kx2 < 2; ++kx2) {
            const size_t r3 = (n * D_P1 + row_of_pos(py, px)) * 4 + ky2 * 2 + kx2;
            const float4* av = reinterpret_cast<const float4*>(a2s + r3 * D_C2);
            float a[D_C2];
#pragma unroll
            for (int k = 0; k < D_C2 / 4; ++k) {
                const float4 v = av[k];
                a[4 * k] = v.x; a[4 * k + 1] = v.y; a[4 * k + 2] = v.z; a[4 * k + 3] = v.w;
            }
            float da[D_C2];
#pragma unroll
            for (int ci = 0; ci < D_C2; ++ci) da[ci] = 0.f;
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                dzs[j] += g[kx2][j];
#pragma unroll
                for (int ci = 0; ci < D_C2; ++ci) {
                    acc[ci][j] = fmaf(a[ci], g[kx2][j], acc[ci][j]);
                    da[ci] = fmaf(w6[ci * 12 + j], g[kx2][j], da[ci]);
                }
            }
            float4* dv = reinterpret_cast<float4*>(dz4 + r3 * D_C2);
#pragma unroll
            for (int k = 0; k < D_C2 / 4; ++k)
                dv[k] = make_float4(a[4 * k] > 0.f ? da[4 * k] : 0.f, a[4 * k + 1] > 0.f ? da[4 * k + 1] : 0.f,
                                    a[4 * k + 2] > 0.f ? da[4 * k + 2] : 0.f, a[4 * k + 3] > 0.f ? da[4 * k + 3] : 0.f);
        }
    }
    // the 64 lanes by a butterfly, the four waves in order
#pragma unroll
    for (int j = 0; j < 12; ++j) {
#pragma unroll
        for (int ci = 0; ci <= D_C2; ++ci) {
            float v = ci < D_C2 ? acc[ci & (D_C2 - 1)][j] : dzs[j];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
            if (lane == 0) red[wave][ci * 12 + j] = v;
        }
    }
    __syncthreads();
    float* out = part + n * D_W6_LD;
    const int t = threadIdx.x;
    if (t < D_C2 * 12) {                               // torch index t = ci*12 + co*4 + kk3
        const int ci = t / 12, co = (t - ci * 12) >> 2, kk3 = t & 3, s = ci * 12 + kk3 * 3 + co;
        out[t] = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
    } else if (t < D_C2 * 12 + 3) {
        const int co = t - D_C2 * 12;
        float b = 0.f;
        for (int kk3 = 0; kk3 < 4; ++kk3) {
            const int s = D_C2 * 12 + kk3 * 3 + co;
            b += ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
        }
        out[t] = b;
    }
}

// Layer 4's data gradient under a1's ReLU mask: dz2[r2][ci] = (a1[r2][ci] > 0) sum_j dz4[r2][j] w4[ci][j], j = kk2*16 + co
// ascending.  One row per thread; the weights are wave-uniform scalar loads.
__global__ __launch_bounds__(256) void decoder_dgrad4_kernel(const float* __restrict__ dz4, const float* __restrict__ a1s,
                                                             const float* __restrict__ w4, long long rows,
                                                             float* __restrict__ dz2) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const float4* g = reinterpret_cast<const float4*>(dz4 + (size_t)row * 64);
    float acc[D_C1];
#pragma unroll
    for (int ci = 0; ci < D_C1; ++ci) acc[ci] = 0.f;
    for (int j4 = 0; j4 < 16; ++j4) {
        const float4 v4 = g[j4];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ci = 0; ci < D_C1; ++ci) acc[ci] = fmaf(w4[ci * 64 + j4 * 4 + i], v[i], acc[ci]);
    }
    const float4* av = reinterpret_cast<const float4*>(a1s + (size_t)row * D_C1);
    float4* out = reinterpret_cast<float4*>(dz2 + (size_t)row * D_C1);
#pragma unroll
    for (int k = 0; k < D_C1 / 4; ++k) {
        const float4 a = av[k];
        out[k] = make_float4(a.x > 0.f ? acc[4 * k] : 0.f, a.y > 0.f ? acc[4 * k + 1] : 0.f, a.z > 0.f ? acc[4 * k + 2] : 0.f,
                             a.w > 0.f ? acc[4 * k + 3] : 0.f);
    }
}

// Column sums of a thin matrix over very many rows, two levels.  Level 1: workgroup (slab, column group of 64) -- thread
// (rl = t >> 6, column t & 63) adds rows m0 + rl, m0 + rl + 4, ... of its slab in ascending order, the four partial rows then
// in order: part[slab][C].
__global__ __launch_bounds__(256) void decoder_colsum_part_kernel(const float* __restrict__ src, int C, long long M, int slab_rows,
                                                                  float* __restrict__ part) {
    __shared__ float red[4][64];
    const int col = blockIdx.y * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
    const long long m0 = (long long)blockIdx.x * slab_rows, m1 = min(M, m0 + slab_rows);
    float s = 0.f;
    for (long long m = m0 + rl; m < m1; m += 4) s += src[m * C + col];
    red[rl][threadIdx.x & 63] = s;
    __syncthreads();
    if (rl == 0) part[(size_t)blockIdx.x * C + col] = ((red[0][col & 63] + red[1][col & 63]) + red[2][col & 63]) + red[3][col & 63];
}
// Level 2, one thread per output: the slabs in ascending order, then
//   fold == 4  dst[co] = sum over kk (ascending) of column kk * n_out + co        (a transposed convolution's bias)
//   fold == 1  dst[c*144 + q] = column q*64 + c                                    (the Linear's bias, back in Flatten order)
__global__ void decoder_colsum_fold_kernel(const float* __restrict__ part, int nslab, int C, int n_out, int fold,
                                           float* __restrict__ dst) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_out) return;
    float total = 0.f;
    for (int f = 0; f < fold; ++f) {
        const int col = fold == 1 ? (o % D_Q) * D_C0 + o / D_Q : f * n_out + o;
        float s = 0.f;
        for (int b = 0; b < nslab; ++b) s += part[(size_t)b * C + col];
        total = f == 0 ? s : total + s;
    }
    dst[o] = total;
}

// weight gradients back in torch layout
//   a transposed convolution (cin, cout, 2, 2):  dst[ci][co*4 + kk] = src[ci][kk*cout + co]
__global__ void decoder_unperm_conv_kernel(const float* __restrict__ src, int cin, int cout, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cin * cout * 4) return;
    const int ci = i / (cout * 4), r = i - ci * cout * 4, co = r >> 2, kk = r & 3;
    dst[i] = src[ci * cout * 4 + kk * cout + co];
}
//   the Linear (9216, 128):  dst[c*144 + q][k] = src[q*64 + c][k]
__global__ void decoder_unperm_linear_kernel(const float* __restrict__ src, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D_Q * D_C0 * 128) return;
    const int row = i >> 7, k = i & 127, c = row / D_Q, q = row - c * D_Q;
    dst[i] = src[(q * D_C0 + c) * 128 + k];
}

inline unsigned blocks_of(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

}  // namespace

hipError_t launch_decoder_convs(const float* h0, const float* w2, const float* b2, const float* w4, const float* b4,
                                const float* w6, const float* b6, float* recon, int n_frames, hipStream_t s) {
    if (n_frames <= 0 || !h0 || !w2 || !b2 || !w4 || !b4 || !w6 || !b6 || !recon) return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * D_P1 * D_S1;                       // 76,032 bytes
    if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(decoder_convs_kernel<false>)); e != hipSuccess) return e;
    hipLaunchKernelGGL(decoder_convs_kernel<false>, dim3(n_frames), dim3(256), lds, s, h0, w2, b2, w4, b4, w6, b6, recon,
                       (const float*)nullptr, (float*)nullptr, (float*)nullptr, (double*)nullptr);
    return hipGetLastError();
}

hipError_t launch_decoder_train_convs(const float* h0, const float* w2, const float* b2, const float* w4, const float* b4,
                                      const float* w6, const float* b6, float* recon, const float* target, float* a1, float* a2,
                                      double* sq, int n_frames, hipStream_t s) {
    if (n_frames <= 0 || !h0 || !w2 || !b2 || !w4 || !b4 || !w6 || !b6 || !recon || !target || !a1 || !a2 || !sq)
        return hipErrorInvalidValue;
    const size_t lds = sizeof(float) * D_P1 * D_S1;
    if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(decoder_convs_kernel<true>)); e != hipSuccess) return e;
    hipLaunchKernelGGL(decoder_convs_kernel<true>, dim3(n_frames), dim3(256), lds, s, h0, w2, b2, w4, b4, w6, b6, recon, target,
                       a1, a2, sq);
    return hipGetLastError();
}

hipError_t launch_decoder_kinks(const float* latent, const float* w0, const float* b0, const float* w2, const float* b2,
                                const float* w4, const float* b4, float* a1, float* a2, int n_frames, hipStream_t s) {
    if (n_frames <= 0 || !latent || !w0 || !b0 || !w2 || !b2 || !w4 || !b4 || !a1 || !a2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_kinks_kernel, dim3(n_frames, D_Q / DK_Q), dim3(256), 0, s, latent, w0, b0, w2, b2, w4, b4, a1, a2);
    return hipGetLastError();
}

hipError_t launch_decoder_loss(const double* sq, int n_frames, float* loss, hipStream_t s) {
    if (n_frames <= 0 || !sq || !loss) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_loss_kernel, dim3(1), dim3(256), 0, s, sq, n_frames, loss);
    return hipGetLastError();
}

hipError_t launch_decoder_bwd6(const float* recon, const float* target, const float* a2, const float* w6, float scale,
                               int n_frames, float* dz4, float* part, float* dw, float* db, hipStream_t s) {
    if (n_frames <= 0 || !recon || !target || !a2 || !w6 || !dz4 || !part || !dw || !db) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_bwd6_kernel, dim3(n_frames), dim3(256), 0, s, recon, target, a2, w6, scale, dz4, part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (hipError_t e = launch_colsum(part, D_W6_LD, n_frames, D_C2 * 12, dw, s); e != hipSuccess) return e;
    return launch_colsum(part + D_C2 * 12, D_W6_LD, n_frames, 3, db, s);
}

hipError_t launch_decoder_dgrad4(const float* dz4, const float* a1, const float* w4, int n_frames, float* dz2, hipStream_t s) {
    if (n_frames <= 0 || !dz4 || !a1 || !w4 || !dz2) return hipErrorInvalidValue;
    const long long rows = (long long)n_frames * D_P1;
    hipLaunchKernelGGL(decoder_dgrad4_kernel, dim3(blocks_of((size_t)rows, 256)), dim3(256), 0, s, dz4, a1, w4, rows, dz2);
    return hipGetLastError();
}

int decoder_colsum_slab_rows(long long M) {               // <= 256 slabs of >= 64 rows
    const long long r = std::max<long long>(64, (M + 255) / 256);
    return (int)((r + 3) / 4 * 4);
}
int decoder_colsum_slabs(long long M) {
    const long long rows = decoder_colsum_slab_rows(M);
    return (int)((M + rows - 1) / rows);
}

hipError_t launch_decoder_colsum(const float* src, int C, long long M, int n_out, int fold, float* part, float* dst,
                                 hipStream_t s) {
    if (M <= 0 || !src || !part || !dst || C % 64 != 0 || !((fold == 4 && n_out * 4 == C) || (fold == 1 && n_out == C && C == D_Q * D_C0)))
        return hipErrorInvalidValue;
    const int rows = decoder_colsum_slab_rows(M), slabs = decoder_colsum_slabs(M);
    hipLaunchKernelGGL(decoder_colsum_part_kernel, dim3(slabs, C / 64), dim3(256), 0, s, src, C, M, rows, part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(decoder_colsum_fold_kernel, dim3(blocks_of((size_t)n_out, 256)), dim3(256), 0, s, (const float*)part, slabs, C,
                       n_out, fold, dst);
    return hipGetLastError();
}

hipError_t launch_decoder_unperm_conv(const float* src, int cin, int cout, float* dst, hipStream_t s) {
    if (!src || !dst || cin <= 0 || cout <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_unperm_conv_kernel, dim3(blocks_of((size_t)cin * cout * 4, 256)), dim3(256), 0, s, src, cin, cout, dst);
    return hipGetLastError();
}

hipError_t launch_decoder_unperm_linear(const float* src, float* dst, hipStream_t s) {
    if (!src || !dst) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decoder_unperm_linear_kernel, dim3(blocks_of((size_t)D_Q * D_C0 * 128, 256)), dim3(256), 0, s, src, dst);
    return hipGetLastError();
}

}  // namespace spdm
