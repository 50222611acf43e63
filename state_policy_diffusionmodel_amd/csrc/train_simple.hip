// train_simple.hip -- the kernels of the training-loss gradient of models/simple_Unet.py's UNet (SPDM_FLAG_TRAIN_SIMPLE,
// spdm_train_loss_grad).
//
// That network lives in channel-padded storage: real channels at the positions of a ChanMap, exact zeros
// elsewhere.  What the FiLM networks' kernels (train.hip) cannot do here: GroupNorm backward at storage widths that are not
// a power of two (64 .. 512, statistics over the REAL channel count), the residual DoubleConvolution's GELU(GN(y) + x), the
// block tail (+ time embedding, 32 appended conditioning channels), the dropout multiplier on pe[t] and the SiLU in front of
// cond_emb_layer.  A channel map reaches a kernel as its device array pos[i] = storage lane of real channel i.
// Every reduction runs in a fixed order: no float atomics, two calls give bit-identical results.
#include "device_utils.h"

namespace spdm {

static constexpr int TS_MAX_CH = 512;          // widest storage of the network (up1's doubleConv1: 320 + 192)

__device__ __forceinline__ float ts_gelu_grad(float v) {
    return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
}

// real[c] = 1 for the storage lanes of the map's real channels, 0 for padding (C lanes, 256 threads)
__device__ __forceinline__ void ts_lane_mask(const int* __restrict__ pos, int nreal, int C, unsigned char* real) {
    for (int c = threadIdx.x; c < C; c += 256) real[c] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < nreal; i += 256) real[pos[i]] = 1;
    __syncthreads();
}

// Backward of out = [GELU](GroupNorm(1, C_real)(y)) at storage width C (a multiple of 64, <= 512), one sample per workgroup
// of 256 threads: 64 channel lanes x 4 row lanes, each thread covering channels lane + 64 j.  g: the gradient of out.  With
// gg = g [* GELU'(gamma xh + beta)] * gamma and xh the normalised input, over the real lanes:
//   dy = rstd (gg - mean(gg) - xh mean(gg xh)), the means over HW * C_real values;
//   dgb[b][c] = {sum_p g' xh, sum_p g'} (per-sample partials of d gamma, d beta).
// Padded lanes of dy and dgb are written as exact zeros.
__global__ __launch_bounds__(256) void gn_bwd_mapped_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ g, int gelu,
                                                            int HW, int C, const int* __restrict__ pos, int nreal,
                                                            float* __restrict__ dy, float* __restrict__ dgb) {
    __shared__ unsigned char real[TS_MAX_CH];
    __shared__ double r1[256], r2[256];
    __shared__ float pa[4][TS_MAX_CH], pb[4][TS_MAX_CH];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, rl = tid >> 6, nch = C >> 6;
    ts_lane_mask(pos, nreal, C, real);
    const size_t base = (size_t)b * HW * C;
    const float mu = mean[b], rs = rstd[b];
    double s1 = 0.0, s2 = 0.0;
    float dga[TS_MAX_CH / 64], dbe[TS_MAX_CH / 64];
#pragma unroll
    for (int j = 0; j < TS_MAX_CH / 64; ++j) { dga[j] = 0.f; dbe[j] = 0.f; }
    for (int p = rl; p < HW; p += 4) {
#pragma unroll
        for (int j = 0; j < TS_MAX_CH / 64; ++j) {
            const int c = j * 64 + lane;
            if (j >= nch || !real[c]) continue;
            const size_t i = base + (size_t)p * C + c;
            const float ga = gamma[c], xh = (y[i] - mu) * rs;
            float gv = g[i];
            if (gelu) gv *= ts_gelu_grad(ga * xh + beta[c]);
            dga[j] += gv * xh;
            dbe[j] += gv;
            s1 += (double)(gv * ga);
            s2 += (double)(gv * ga) * xh;
        }
    }
#pragma unroll
    for (int j = 0; j < TS_MAX_CH / 64; ++j)
        if (j < nch) { pa[rl][j * 64 + lane] = dga[j]; pb[rl][j * 64 + lane] = dbe[j]; }
    r1[tid] = s1; r2[tid] = s2;
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const bool rc = real[c];
        dgb[((size_t)b * C + c) * 2] = rc ? ((pa[0][c] + pa[1][c]) + pa[2][c]) + pa[3][c] : 0.f;
        dgb[((size_t)b * C + c) * 2 + 1] = rc ? ((pb[0][c] + pb[1][c]) + pb[2][c]) + pb[3][c] : 0.f;
    }
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { r1[tid] += r1[tid + w]; r2[tid] += r2[tid + w]; }
        __syncthreads();
    }
    const double inv = 1.0 / ((double)HW * nreal);
    const float m1 = (float)(r1[0] * inv), m2 = (float)(r2[0] * inv);
    for (int p = rl; p < HW; p += 4) {
#pragma unroll
        for (int j = 0; j < TS_MAX_CH / 64; ++j) {
            const int c = j * 64 + lane;
            if (j >= nch) continue;
            const size_t i = base + (size_t)p * C + c;
            if (!real[c]) { dy[i] = 0.f; continue; }
            const float ga = gamma[c], xh = (y[i] - mu) * rs;
            float gv = g[i];
            if (gelu) gv *= ts_gelu_grad(ga * xh + beta[c]);
            dy[i] = rs * (gv * ga - m1 - xh * m2);
        }
    }
}

// dgamma[i] = sum_b p0[b][pos[i]][0] + sum_b p1[b][pos[i]][0], dbeta likewise: the ONE GroupNorm module of a DoubleConvolution
// serves both convolutions; written in torch layout (the real channels in order)
__global__ void gn_param_mapped_kernel(const float* __restrict__ p0, const float* __restrict__ p1, int B, int C,
                                       const int* __restrict__ pos, int nreal, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nreal) return;
    const int c = pos[i];
    float a = 0.f, bb = 0.f;
    for (int b = 0; b < B; ++b) { a += p0[((size_t)b * C + c) * 2]; bb += p0[((size_t)b * C + c) * 2 + 1]; }
    for (int b = 0; b < B; ++b) { a += p1[((size_t)b * C + c) * 2]; bb += p1[((size_t)b * C + c) * 2 + 1]; }
    dgamma[i] = a;
    dbeta[i] = bb;
}

// End of a residual DoubleConvolution (simple_Unet.py:117-119): pre = GN(y) + res, out = GELU(pre).  pre is what the backward
// pass differentiates GELU at.
__global__ void gn_res_kernel(const float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ rstd,
                              const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ res,
                              int HW, int C, size_t n, float* __restrict__ pre, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int b = (int)(i / ((size_t)HW * C));
    const float v = (gamma[c] * ((y[i] - mean[b]) * rstd[b]) + beta[c]) + res[i];
    pre[i] = v;
    out[i] = gelu_erf(v);
}

// Block tail (simple_Unet.py:160-176, :209-224) on the saved raw output y (width Cz) of the block's last convolution:
//   out[:, 0:Cr]       = GELU(GN(y)) + temb[b]          (Linear(SiLU(pe[t_b] * scale_b)) of the call)
//   out[:, Cr:Cr + 32] = cemb[b]                        (Linear(SiLU(cond)) of this block)
//   out[:, Cr + 32:Co] = 0                              (storage padding)
__global__ void simple_tail_fwd_kernel(const float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ rstd,
                                       const float* __restrict__ gamma, const float* __restrict__ beta, int Cz, int Cr,
                                       const float* __restrict__ temb, int temb_ld, const float* __restrict__ cemb, int cemb_ld,
                                       int HW, int Co, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % Co);
    const size_t m = i / Co;
    const int b = (int)(m / HW);
    float v = 0.f;
    if (c < Cr) v = gelu_erf(gamma[c] * ((y[m * Cz + c] - mean[b]) * rstd[b]) + beta[c]) + temb[(size_t)b * temb_ld + c];
    else if (c < Cr + 32) v = cemb[(size_t)b * cemb_ld + (c - Cr)];
    out[i] = v;
}

// Backward of the block tail, one sample per workgroup (64 channel lanes x 4 row lanes), dout [B][HW][Co]:
//   dz[b][p][c] = dout[b][p][c] for c < Cr, 0 for Cr <= c < Cz  (the gradient of GELU(GN(y)), width Cz);
//   dtemb[b][c] = sum_p dout[b][p][c] (c < Cr, rows of Cr);  dcemb[b][j] = sum_p dout[b][p][Cr + j] (j < 32, rows of cemb_ld).
__global__ __launch_bounds__(256) void simple_tail_bwd_kernel(const float* __restrict__ dout, int HW, int Co, int Cr, int Cz,
                                                              float* __restrict__ dz, float* __restrict__ dtemb,
                                                              float* __restrict__ dcemb, int cemb_ld) {
    __shared__ float ps[4][TS_MAX_CH];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, rl = tid >> 6, nch = Co >> 6;
    float acc[TS_MAX_CH / 64];
#pragma unroll
    for (int j = 0; j < TS_MAX_CH / 64; ++j) acc[j] = 0.f;
    for (int p = rl; p < HW; p += 4) {
        const size_t row = (size_t)b * HW + p;
#pragma unroll
        for (int j = 0; j < TS_MAX_CH / 64; ++j) {
            const int c = j * 64 + lane;
            if (j >= nch) continue;
            const float d = dout[row * Co + c];
            acc[j] += d;
            if (c < Cz) dz[row * Cz + c] = c < Cr ? d : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < TS_MAX_CH / 64; ++j)
        if (j < nch) ps[rl][j * 64 + lane] = acc[j];
    __syncthreads();
    for (int c = tid; c < Cr + 32; c += 256) {
        const float s = ((ps[0][c] + ps[1][c]) + ps[2][c]) + ps[3][c];
        if (c < Cr) dtemb[(size_t)b * Cr + c] = s;
        else dcemb[(size_t)b * cemb_ld + (c - Cr)] = s;
    }
}

// tsilu[b][i] = SiLU(pe[t_b][i] * scale[b][i]): the rows the six emb_layer Linears read under PositionalEncoding's dropout
// (scale = the caller's mask / (1 - p))
__global__ void time_rows_scaled_kernel(const float* __restrict__ pe, const int* __restrict__ t_dev, int t_count,
                                        const float* __restrict__ scale, int B, int n, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * n) return;
    const int b = i / n;
    const float v = pe[(size_t)t_dev[t_count == 1 ? 0 : b] * n + (i - b * n)] * scale[i];
    out[i] = v / (1.0f + expf(-v));
}

// grad_cond[b][j] = SiLU'(cond[b][j]) ds[b][j], ds rows of ld floats (d SiLU(cond), the six cond_emb_layer projections summed
// by one GEMM over their stacked weights)
__global__ void silu_bwd_kernel(const float* __restrict__ ds, int ld, const float* __restrict__ cond, int B, int cond_dim,
                                float* __restrict__ grad_cond) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * cond_dim) return;
    const int b = i / cond_dim, j = i - b * cond_dim;
    const float x = cond[i];
    const float sg = 1.f / (1.f + expf(-x));
    grad_cond[i] = ds[(size_t)b * ld + j] * (sg * (1.f + x * (1.f - sg)));
}

static inline unsigned ts_blocks(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

hipError_t launch_gn_bwd_mapped(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                const float* g, int gelu, int B, int HW, int C, const int* pos, int nreal, float* dy, float* dgb,
                                hipStream_t s) {
    if (C % 64 != 0 || C < 64 || C > TS_MAX_CH || nreal < 1 || nreal > C || !pos) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_bwd_mapped_kernel, dim3(B), dim3(256), 0, s, y, mean, rstd, gamma, beta, g, gelu, HW, C, pos, nreal, dy,
                       dgb);
    return hipGetLastError();
}

hipError_t launch_gn_param_mapped(const float* p0, const float* p1, int B, int C, const int* pos, int nreal, float* dgamma,
                                  float* dbeta, hipStream_t s) {
    hipLaunchKernelGGL(gn_param_mapped_kernel, dim3(ts_blocks(nreal, 256)), dim3(256), 0, s, p0, p1, B, C, pos, nreal, dgamma, dbeta);
    return hipGetLastError();
}

hipError_t launch_gn_res(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* res, int B, int HW, int C, float* pre, float* out, hipStream_t s) {
    const size_t n = (size_t)B * HW * C;
    hipLaunchKernelGGL(gn_res_kernel, dim3(ts_blocks(n, 256)), dim3(256), 0, s, y, mean, rstd, gamma, beta, res, HW, C, n, pre, out);
    return hipGetLastError();
}

hipError_t launch_simple_tail_fwd(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                  int Cz, int Cr, const float* temb, int temb_ld, const float* cemb, int cemb_ld, int B, int HW,
                                  int Co, float* out, hipStream_t s) {
    if (Cr > Cz || Cr + 32 > Co) return hipErrorInvalidValue;
    const size_t n = (size_t)B * HW * Co;
    hipLaunchKernelGGL(simple_tail_fwd_kernel, dim3(ts_blocks(n, 256)), dim3(256), 0, s, y, mean, rstd, gamma, beta, Cz, Cr, temb,
                       temb_ld, cemb, cemb_ld, HW, Co, n, out);
    return hipGetLastError();
}

hipError_t launch_simple_tail_bwd(const float* dout, int B, int HW, int Co, int Cr, int Cz, float* dz, float* dtemb, float* dcemb,
                                  int cemb_ld, hipStream_t s) {
    if (Co % 64 != 0 || Co > TS_MAX_CH || Cr > Cz || Cz > Co || Cr + 32 > Co) return hipErrorInvalidValue;
    hipLaunchKernelGGL(simple_tail_bwd_kernel, dim3(B), dim3(256), 0, s, dout, HW, Co, Cr, Cz, dz, dtemb, dcemb, cemb_ld);
    return hipGetLastError();
}

hipError_t launch_time_rows_scaled(const float* pe, const int* t_dev, int t_count, const float* scale, int B, int n, float* out,
                                   hipStream_t s) {
    hipLaunchKernelGGL(time_rows_scaled_kernel, dim3(ts_blocks((size_t)B * n, 256)), dim3(256), 0, s, pe, t_dev, t_count, scale, B,
                       n, out);
    return hipGetLastError();
}

hipError_t launch_silu_bwd(const float* ds, int ld, const float* cond, int B, int cond_dim, float* grad_cond, hipStream_t s) {
    hipLaunchKernelGGL(silu_bwd_kernel, dim3(ts_blocks((size_t)B * cond_dim, 256)), dim3(256), 0, s, ds, ld, cond, B, cond_dim,
                       grad_cond);
    return hipGetLastError();
}

}  // namespace spdm
