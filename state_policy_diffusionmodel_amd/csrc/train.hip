// train.hip -- the kernels of the training-loss gradient (spdm_train_loss_grad) of UNet_Film_noAttention
// (models/Unet_FiLmLayer_noAttention.py; training_step -> process_single_batch, models/diffusion_ddpm.py:128-173).
//
// The forward half of a training step runs the plan's own implicit-GEMM kernels on MATERIALISED inputs; these kernels
// supply what those launches do not: the GroupNorm statistics and finishing pass, the Cin = 1 first convolution, the 1x1
// out convolution + MSE loss, and every backward op.  The backward contractions are
//   - data gradients of 3x3 convolutions and Linear layers: the forward GEMM kernels (spdm_api.hip, exact fp32 path) on
//     flipped / transposed weight copies;
//   - weight gradients: wgrad_partial_kernel below, fp32 MFMA (v_mfma_f32_16x16x4_f32), rows split over workgroups into
//     partial slabs that wgrad_combine_kernel adds in a fixed order -- no float atomics, so a gradient is bit-reproducible.
// Every reduction here runs in a fixed order for the same reason.
#include <algorithm>

#include "device_utils.h"

namespace spdm {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// source row of output row m under tap `tap` of a same-padded 3x3 (taps 9), vertical 3x1 (taps 3, W == 1) or 1x1 (taps 1)
// convolution on H x W maps; -1: zero padding
__device__ __forceinline__ long long tap_src(long long m, int tap, int taps, int H, int W, int HW) {
    if (taps == 1) return m;
    const long long b = m / HW;
    const int p = (int)(m - b * HW);
    const int y = p / W, x = p - (p / W) * W;
    const int dy = (taps == 9 ? tap / 3 : tap) - 1, dx = (taps == 9 ? tap % 3 : 1) - 1;
    const int ys = y + dy, xs = x + dx;
    if (ys < 0 || ys >= H || xs < 0 || xs >= W) return -1;
    return b * HW + (long long)ys * W + xs;
}

// partial[chunk][tap][co][ci] = sum over rows m of chunk: dy[m][co] * x[tap_src(m)][ci].  Workgroup = 4 waves = a 64 (co) x 64
// (ci) tile of one tap; wave = 32 x 32 as 2 x 2 MFMA 16x16x4 tiles.  Operands straight from global memory: each k-step of an
// MFMA is 4 rows, lanes l & 15 read 16 consecutive channels of row l >> 4.
__global__ __launch_bounds__(256) void wgrad_partial_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x,
                                                            int ldx, long long M, int H, int W, int HW, int taps, int Co,
                                                            int Ci, int rows, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ci_tiles = (Ci + 63) / 64;
    const int co0 = (blockIdx.x / ci_tiles) * 64 + (wave >> 1) * 32;
    const int ci0 = (blockIdx.x % ci_tiles) * 64 + (wave & 1) * 32;
    const int tap = blockIdx.y, chunk = blockIdx.z;
    const long long m0 = (long long)chunk * rows, m1 = min(M, m0 + rows);
    const int r = lane & 15, k = lane >> 4;
    f32x4_t acc[2][2];
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (long long m = m0; m < m1; m += 4) {
        const long long row = m + k;
        float a[2] = {0.f, 0.f}, bv[2] = {0.f, 0.f};
        if (row < m1) {
            const long long src = tap_src(row, tap, taps, H, W, HW);
            for (int i = 0; i < 2; ++i) {
                const int co = co0 + 16 * i + r;
                if (co < Co) a[i] = dy[row * ldy + co];
            }
            if (src >= 0)
                for (int j = 0; j < 2; ++j) {
                    const int ci = ci0 + 16 * j + r;
                    if (ci < Ci) bv[j] = x[src * ldx + ci];
                }
        }
        for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv[j], acc[i][j], 0, 0, 0);
    }
    float* out = partial + ((size_t)chunk * taps + tap) * (size_t)Co * Ci;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            for (int q = 0; q < 4; ++q) {
                const int co = co0 + 16 * i + 4 * k + q, ci = ci0 + 16 * j + r;     // C/D: row (lane >> 4) * 4 + reg, col lane & 15
                if (co < Co && ci < Ci) out[(size_t)co * Ci + ci] = acc[i][j][q];
            }
}

// dst = sum over chunks (ascending) of partial, in torch layout: conv9 -> (Co, Ci, 3, 3) (taps 3: the centre column, the side
// columns exact zeros), else (Co, Ci)
__global__ void wgrad_combine_kernel(const float* __restrict__ partial, int nchunks, int taps, int Co, int Ci, int conv9,
                                     float* __restrict__ dst) {
    const int T = conv9 ? 9 : 1;
    const size_t n = (size_t)Co * Ci * T;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t9 = (int)(i % T);
    const size_t oc = i / T;                  // co * Ci + ci
    int tap = t9;
    if (conv9 && taps == 3) tap = (t9 % 3 == 1) ? t9 / 3 : -1;
    float s = 0.f;
    if (tap >= 0) {
        const size_t slab = (size_t)taps * Co * Ci;
        const float* p = partial + (size_t)tap * Co * Ci + oc;
        for (int c = 0; c < nchunks; ++c) s += p[(size_t)c * slab];
    }
    dst[i] = s;
}

// The same sum for a channel-padded layer (models/simple_Unet.py): partials at storage widths Co x Ci, dst (no, ni, 3, 3) in torch
// layout gathered through the maps' device arrays pos_o / pos_i (storage lane of each real channel)
__global__ void wgrad_combine_mapped_kernel(const float* __restrict__ partial, int nchunks, int taps, int Co, int Ci,
                                            const int* __restrict__ pos_o, int no, const int* __restrict__ pos_i, int ni,
                                            float* __restrict__ dst) {
    const size_t n = (size_t)no * ni * 9;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int t9 = (int)(i % 9);
    const size_t oc = i / 9;                  // co_real * ni + ci_real
    const int co = pos_o[oc / ni], ci = pos_i[oc % ni];
    int tap = t9;
    if (taps == 3) tap = (t9 % 3 == 1) ? t9 / 3 : -1;
    float s = 0.f;
    if (tap >= 0) {
        const size_t slab = (size_t)taps * Co * Ci;
        const float* p = partial + ((size_t)tap * Co + co) * Ci + ci;
        for (int c = 0; c < nchunks; ++c) s += p[(size_t)c * slab];
    }
    dst[i] = s;
}

// dst[c] = sum_m src[m * ld + c] (bias gradients): one workgroup per column, fixed-order tree
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ src, int ld, long long M, float* __restrict__ dst) {
    __shared__ float red[256];
    const int c = blockIdx.x;
    float s = 0.f;
    for (long long m = threadIdx.x; m < M; m += 256) s += src[m * ld + c];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) dst[c] = red[0];
}

// per-sample mean and 1 / sqrt(var + eps) of GroupNorm(1, C) over the n = HW * C values of a sample (fp64 sums, fixed-order
// tree), divided by cnt: n, or HW * C_real for channel-padded storage whose padded lanes hold zeros
__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ y, int n, int cnt, float* __restrict__ mean,
                                                       float* __restrict__ rstd) {
    __shared__ double s1[256], s2[256];
    const int b = blockIdx.x;
    const float* p = y + (size_t)b * n;
    double a = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { const double v = p[i]; a += v; q += v * v; }
    s1[threadIdx.x] = a; s2[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { s1[threadIdx.x] += s1[threadIdx.x + w]; s2[threadIdx.x] += s2[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mu = s1[0] / cnt, var = fmax(s2[0] / cnt - mu * mu, 0.0);
        mean[b] = (float)mu;
        rstd[b] = (float)(1.0 / sqrt(var + 1e-5));
    }
}

// out = [GELU](gamma_c (y - mean_b) rstd_b + beta_c)
__global__ void gn_act_kernel(const float* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ rstd,
                              const float* __restrict__ gamma, const float* __restrict__ beta, int HW, int C, int gelu,
                              size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const int b = (int)(i / ((size_t)HW * C));
    float v = gamma[c] * ((y[i] - mean[b]) * rstd[b]) + beta[c];
    out[i] = gelu ? gelu_erf(v) : v;
}

__device__ __forceinline__ float gelu_grad(float v) {
    return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * 0.39894228040143268f * expf(-0.5f * v * v);
}

// Backward of out = [GELU](GroupNorm(1, C)(y)) for one sample per workgroup (blockDim = max(256, C), a multiple of C).
// g: the gradient of out.  With gg = g [* GELU'(n)] * gamma and xh the normalised input:
//   dy = rstd (gg - mean(gg) - xh mean(gg xh));  per-sample partials dgb[b][c] = {sum g' xh, sum g'} for dgamma, dbeta.
__global__ __launch_bounds__(512) void gn_bwd_kernel(const float* __restrict__ y, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ g, int gelu,
                                                     int HW, int C, float* __restrict__ dy, float* __restrict__ dgb) {
    __shared__ double r1[512], r2[512];
    __shared__ float cg[512], cb[512];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int c = tid % C, p0 = tid / C, pstep = nt / C;
    const size_t base = (size_t)b * HW * C;
    const float mu = mean[b], rs = rstd[b], ga = gamma[c], be = beta[c];
    double s1 = 0.0, s2 = 0.0;
    float dga = 0.f, dbe = 0.f;
    for (int p = p0; p < HW; p += pstep) {
        const size_t i = base + (size_t)p * C + c;
        const float xh = (y[i] - mu) * rs;
        float gv = g[i];
        if (gelu) gv *= gelu_grad(ga * xh + be);
        dga += gv * xh;
        dbe += gv;
        s1 += (double)(gv * ga);
        s2 += (double)(gv * ga) * xh;
    }
    r1[tid] = s1; r2[tid] = s2; cg[tid] = dga; cb[tid] = dbe;
    __syncthreads();
    if (tid < C) {
        float a = 0.f, bb = 0.f;
        for (int t = tid; t < nt; t += C) { a += cg[t]; bb += cb[t]; }
        dgb[((size_t)b * C + tid) * 2] = a;
        dgb[((size_t)b * C + tid) * 2 + 1] = bb;
    }
    for (int w = nt >> 1; w > 0; w >>= 1) {
        if (tid < w) { r1[tid] += r1[tid + w]; r2[tid] += r2[tid + w]; }
        __syncthreads();
    }
    const double inv = 1.0 / ((double)HW * C);
    const float m1 = (float)(r1[0] * inv), m2 = (float)(r2[0] * inv);
    for (int p = p0; p < HW; p += pstep) {
        const size_t i = base + (size_t)p * C + c;
        const float xh = (y[i] - mu) * rs;
        float gv = g[i];
        if (gelu) gv *= gelu_grad(ga * xh + be);
        dy[i] = rs * (gv * ga - m1 - xh * m2);
    }
}

// dgamma[c] (+)= sum_b (p0[b][c][0] + p1[b][c][0]), dbeta likewise: the two GroupNorms of a DoubleConvolution share the affine
__global__ void gn_param_kernel(const float* __restrict__ p0, const float* __restrict__ p1, int B, int C,
                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float a = 0.f, bb = 0.f;
    for (int b = 0; b < B; ++b) { a += p0[((size_t)b * C + c) * 2]; bb += p0[((size_t)b * C + c) * 2 + 1]; }
    for (int b = 0; b < B; ++b) { a += p1[((size_t)b * C + c) * 2]; bb += p1[((size_t)b * C + c) * 2 + 1]; }
    dgamma[c] = a;
    dbeta[c] = bb;
}

// Backward of out = s (z + e) + f (FiLM; film null: out = z + e), one sample per workgroup (blockDim = max(256, C)):
// dz = s dout;  de = s sum_p dout;  ds = sum_p dout (z + e);  df = sum_p dout.  e = temb_table[t_b].
__global__ __launch_bounds__(512) void film_bwd_kernel(const float* __restrict__ z, const float* __restrict__ temb,
                                                       const int* __restrict__ t_dev, int t_count,
                                                       const float* __restrict__ film, const float* __restrict__ dout, int HW,
                                                       int C, float* __restrict__ dz, float* __restrict__ de,
                                                       float* __restrict__ dfilm) {
    __shared__ float a1[512], a2[512];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int c = tid % C, p0 = tid / C, pstep = nt / C;
    const size_t base = (size_t)b * HW * C;
    const float e = temb[(size_t)t_dev[t_count == 1 ? 0 : b] * C + c];
    const float sc = film ? film[(size_t)b * 2 * C + c] : 1.f;
    float sd = 0.f, sdx = 0.f;
    for (int p = p0; p < HW; p += pstep) {
        const size_t i = base + (size_t)p * C + c;
        const float d = dout[i];
        sd += d;
        sdx += d * (z[i] + e);
        dz[i] = sc * d;
    }
    a1[tid] = sd; a2[tid] = sdx;
    __syncthreads();
    if (tid < C) {
        float s = 0.f, sx = 0.f;
        for (int t = tid; t < nt; t += C) { s += a1[t]; sx += a2[t]; }
        de[(size_t)b * C + tid] = sc * s;
        if (dfilm) {
            dfilm[(size_t)b * 2 * C + tid] = sx;
            dfilm[(size_t)b * 2 * C + C + tid] = s;
        }
    }
}

// out[b][i] = table[t_b][i] (the SiLU(pos_encoding) rows the time-embedding Linears of the call read)
__global__ void gather_rows_kernel(const float* __restrict__ table, const int* __restrict__ t_dev, int t_count, int B, int n,
                                   float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * n) return;
    const int b = i / n;
    out[i] = table[(size_t)t_dev[t_count == 1 ? 0 : b] * n + (i - b * n)];
}

// xp[b][y * Wp + x] = pad_to(x, 8) (models/Unet_FiLmLayer.py:15-28)
__global__ void pad_kernel(const float* __restrict__ x, int B, int H0, int D, int Hp, int Wp, int lh, int lw,
                           float* __restrict__ xp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * Hp * Wp) return;
    const int b = i / (Hp * Wp), p = i - b * Hp * Wp;
    const int h0 = p / Wp - lh, d = p % Wp - lw;
    xp[i] = (h0 >= 0 && h0 < H0 && d >= 0 && d < D) ? x[((size_t)b * H0 + h0) * D + d] : 0.f;
}

// inc.first, Conv2d(1, 64, 3, padding=1, bias=False) on the padded map: out[m][co] = sum_tap w[tap][co] xp[tap_src(m)]
__global__ void conv_in_plain_kernel(const float* __restrict__ xp, const float* __restrict__ w, long long M, int H, int W,
                                     float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * 64) return;
    const long long m = i >> 6;
    const int co = (int)(i & 63);
    float s = 0.f;
    for (int t = 0; t < 9; ++t) {
        const long long src = tap_src(m, t, 9, H, W, H * W);
        if (src >= 0) s += w[t * 64 + co] * xp[src];
    }
    out[i] = s;
}

// outc, Conv2d(64, 1, 1): out[m] = sum_c u[m][c] w[c] + bias
__global__ void outc_kernel(const float* __restrict__ u, const float* __restrict__ w, float bias, long long M,
                            float* __restrict__ out) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float s = 0.f;
    for (int c = 0; c < 64; ++c) s += u[m * 64 + c] * w[c];
    out[m] = s + bias;
}

// du[m][c] = deps[m] w[c]
__global__ void outc_bwd_kernel(const float* __restrict__ deps, const float* __restrict__ w, long long M,
                                float* __restrict__ du) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * 64) return;
    du[i] = deps[i >> 6] * w[i & 63];
}

// loss = mean over the unpadded lanes of (noise - eps)^2; deps_pad = d loss / d eps on the padded map (exact zeros on the
// padded lanes); eps_out (optional) = the unpadded eps.  One workgroup, fixed-order fp64 tree.
__global__ __launch_bounds__(1024) void mse_kernel(const float* __restrict__ eps_pad, const float* __restrict__ noise, int B,
                                                   int H0, int D, int Hp, int Wp, int lh, int lw, float* __restrict__ loss,
                                                   float* __restrict__ deps_pad, float* __restrict__ eps_out) {
    __shared__ double red[1024];
    const int n = B * H0 * D, np = B * Hp * Wp;
    const float k = 2.f / (float)n;
    double s = 0.0;
    for (int i = threadIdx.x; i < np; i += 1024) {
        const int b = i / (Hp * Wp), p = i - b * Hp * Wp;
        const int h0 = p / Wp - lh, d = p % Wp - lw;
        float g = 0.f;
        if (h0 >= 0 && h0 < H0 && d >= 0 && d < D) {
            const size_t j = ((size_t)b * H0 + h0) * D + d;
            const float e = eps_pad[i], diff = e - noise[j];
            s += (double)diff * diff;
            g = k * diff;
            if (eps_out) eps_out[j] = e;
        }
        deps_pad[i] = g;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(red[0] / n);
}

// Backward of MaxPool2d(2) as a gather: d_in[b][p][c] += d_out[window of p][c] where p is the window's FIRST maximum in scan
// order (torch's choice), fine map H x W
__global__ void pool_bwd_kernel(const float* __restrict__ in, const float* __restrict__ dout, int B, int H, int W, int C,
                                float* __restrict__ din) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * H * W * C) return;
    const int c = (int)(i % C);
    const size_t bp = i / C;
    const int b = (int)(bp / ((size_t)H * W)), p = (int)(bp - (size_t)b * H * W);
    const int y = p / W, x = p % W, yc = y >> 1, xc = x >> 1;
    const float* s = in + (size_t)b * H * W * C + c;
    int best = -1;
    float mx = 0.f;
    for (int q = 0; q < 4; ++q) {
        const int pp = (2 * yc + (q >> 1)) * W + 2 * xc + (q & 1);
        const float v = s[(size_t)pp * C];
        if (best < 0 || v > mx) { mx = v; best = pp; }
    }
    if (best == p) din[i] += dout[((size_t)b * (H / 2) * (W / 2) + (size_t)yc * (W / 2) + xc) * C + c];
}

// weight of output index o on input index i of a bilinear x2, align_corners=True resampling of n_in -> 2 n_in
__device__ __forceinline__ float up_weight(int o, int i, int n_in) {
    const int n_out = 2 * n_in;
    const float scale = n_in > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f;
    const float src = scale * o;
    const int i0 = (int)src, i1 = min(i0 + 1, n_in - 1);
    const float l1 = src - (float)i0, l0 = 1.f - l1;
    return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// Backward of the bilinear x2 half of upsample + concat, as a gather over the output pixels that read each input pixel:
// d_x[b][iy, ix][c] += sum_{oy, ox} wy(oy, iy) wx(ox, ix) d_cat[b][oy, ox][c]   (d_cat: [B][4 h w][ld], channels [0, C))
__global__ void up_bwd_kernel(const float* __restrict__ dcat, int ld, int B, int h, int w, int C, float* __restrict__ dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * h * w * C) return;
    const int c = (int)(i % C);
    const size_t bp = i / C;
    const int b = (int)(bp / ((size_t)h * w)), p = (int)(bp - (size_t)b * h * w);
    const int iy = p / w, ix = p % w, H = 2 * h, W = 2 * w;
    // outputs of input index i lie where |scale o - i| < 1, scale = (n-1)/(2n-1) > 1/3: |o - i / scale| < 3
    auto lo_hi = [](int ii, int n_in, int* lo, int* hi) {
        if (n_in == 1) { *lo = 0; *hi = 2; return; }          // both outputs read the one input
        const float inv = (float)(2 * n_in - 1) / (float)(n_in - 1);
        *lo = max(0, (int)floorf((ii - 1) * inv) - 1);
        *hi = min(2 * n_in, (int)ceilf((ii + 1) * inv) + 2);
    };
    int y0, y1, x0, x1;
    lo_hi(iy, h, &y0, &y1);
    lo_hi(ix, w, &x0, &x1);
    float s = 0.f;
    for (int oy = y0; oy < y1; ++oy) {
        const float wy = up_weight(oy, iy, h);
        if (wy == 0.f) continue;
        float r = 0.f;
        for (int ox = x0; ox < x1; ++ox) {
            const float wx = up_weight(ox, ix, w);
            if (wx != 0.f) r += wx * dcat[((size_t)b * H * W + (size_t)oy * W + ox) * ld + c];
        }
        s += wy * r;
    }
    dx[i] += s;
}

// dst[m][c] += src[m * ld + c0 + c] (the skip half of a concat's gradient)
__global__ void add_cols_kernel(const float* __restrict__ src, int ld, int c0, long long M, int C, float* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * C) return;
    const long long m = i / C;
    dst[i] += src[m * ld + c0 + (i - m * C)];
}

// grad_cond[b][j] = Mish'(cond[b][j]) sum_k dm[k][b][j] (k = 0..nblk-1 ascending; dm rows of ld floats)
__global__ void mish_bwd_kernel(const float* __restrict__ dm, int nblk, int B, int ld, const float* __restrict__ cond,
                                int cond_dim, float* __restrict__ grad_cond) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * cond_dim) return;
    const int b = i / cond_dim, j = i - b * cond_dim;
    float s = 0.f;
    for (int k = 0; k < nblk; ++k) s += dm[((size_t)k * B + b) * ld + j];
    const float x = cond[i];
    const float sp = x > 20.f ? x : log1pf(expf(x));
    const float th = tanhf(sp), sg = 1.f / (1.f + expf(-x));
    grad_cond[i] = s * (th + x * (1.f - th * th) * sg);
}

static inline unsigned nblocks(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

int wgrad_chunks(long long M, int taps, int Co, int Ci, size_t budget_floats) {
    const long long tiles = (long long)((Co + 63) / 64) * ((Ci + 63) / 64) * taps;
    long long n = std::max<long long>(1, 2048 / tiles);                      // ~2048 workgroups
    n = std::min<long long>(n, std::max<long long>(1, M / 64));              // >= 64 rows per chunk
    n = std::min<long long>(n, std::max<long long>(1, (long long)(budget_floats / ((size_t)taps * Co * Ci))));
    return (int)n;
}

// the partial slabs of a weight gradient: returns their count, 0 if they do not fit the budget
static int wgrad_partials(const float* dy, int ldy, const float* x, int ldx, long long M, int H, int W, int taps, int Co, int Ci,
                          float* partial, size_t budget_floats, hipStream_t s) {
    const int nch = wgrad_chunks(M, taps, Co, Ci, budget_floats);
    if ((size_t)nch * taps * Co * Ci > budget_floats) return 0;
    long long rows = (M + nch - 1) / nch;
    rows = (rows + 3) / 4 * 4;
    const int tiles = ((Co + 63) / 64) * ((Ci + 63) / 64);
    hipLaunchKernelGGL(wgrad_partial_kernel, dim3(tiles, taps, nch), dim3(256), 0, s, dy, ldy, x, ldx, M, H, W, H * W, taps, Co,
                       Ci, (int)rows, partial);
    return nch;
}

hipError_t launch_wgrad(const float* dy, int ldy, const float* x, int ldx, long long M, int H, int W, int taps, int Co, int Ci,
                        int conv9, float* partial, size_t budget_floats, float* dst, hipStream_t s) {
    const int nch = wgrad_partials(dy, ldy, x, ldx, M, H, W, taps, Co, Ci, partial, budget_floats, s);
    if (nch == 0) return hipErrorInvalidValue;
    const size_t n = (size_t)Co * Ci * (conv9 ? 9 : 1);
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, (const float*)partial, nch, taps, Co, Ci,
                       conv9, dst);
    return hipGetLastError();
}

hipError_t launch_wgrad_mapped(const float* dy, const float* x, long long M, int H, int W, int taps, int Co, int Ci,
                               const int* pos_o, int no, const int* pos_i, int ni, float* partial, size_t budget_floats, float* dst,
                               hipStream_t s) {
    if (taps != 9 && taps != 3) return hipErrorInvalidValue;
    const int nch = wgrad_partials(dy, Co, x, Ci, M, H, W, taps, Co, Ci, partial, budget_floats, s);
    if (nch == 0) return hipErrorInvalidValue;
    const size_t n = (size_t)no * ni * 9;
    hipLaunchKernelGGL(wgrad_combine_mapped_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, (const float*)partial, nch, taps, Co, Ci,
                       pos_o, no, pos_i, ni, dst);
    return hipGetLastError();
}

hipError_t launch_colsum(const float* src, int ld, long long M, int C, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(colsum_kernel, dim3(C), dim3(256), 0, s, src, ld, M, dst);
    return hipGetLastError();
}

hipError_t launch_gn_stats(const float* y, int B, int n, float* mean, float* rstd, hipStream_t s) {
    hipLaunchKernelGGL(gn_stats_kernel, dim3(B), dim3(256), 0, s, y, n, n, mean, rstd);
    return hipGetLastError();
}

hipError_t launch_gn_stats_real(const float* y, int B, int n, int cnt, float* mean, float* rstd, hipStream_t s) {
    if (cnt < 1 || cnt > n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(B), dim3(256), 0, s, y, n, cnt, mean, rstd);
    return hipGetLastError();
}

hipError_t launch_gn_act(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int B,
                         int HW, int C, int gelu, float* out, hipStream_t s) {
    const size_t n = (size_t)B * HW * C;
    hipLaunchKernelGGL(gn_act_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, y, mean, rstd, gamma, beta, HW, C, gelu, n, out);
    return hipGetLastError();
}

static inline int per_channel_threads(int C) { return C > 256 ? C : 256; }

hipError_t launch_gn_bwd(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* g, int gelu, int B, int HW, int C, float* dy, float* dgb, hipStream_t s) {
    const int nt = per_channel_threads(C);
    if (C > 512 || nt % C != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gn_bwd_kernel, dim3(B), dim3(nt), 0, s, y, mean, rstd, gamma, beta, g, gelu, HW, C, dy, dgb);
    return hipGetLastError();
}

hipError_t launch_gn_param(const float* p0, const float* p1, int B, int C, float* dgamma, float* dbeta, hipStream_t s) {
    hipLaunchKernelGGL(gn_param_kernel, dim3(nblocks(C, 256)), dim3(256), 0, s, p0, p1, B, C, dgamma, dbeta);
    return hipGetLastError();
}

hipError_t launch_film_bwd(const float* z, const float* temb, const int* t_dev, int t_count, const float* film,
                           const float* dout, int B, int HW, int C, float* dz, float* de, float* dfilm, hipStream_t s) {
    const int nt = per_channel_threads(C);
    if (C > 512 || nt % C != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(film_bwd_kernel, dim3(B), dim3(nt), 0, s, z, temb, t_dev, t_count, film, dout, HW, C, dz, de, dfilm);
    return hipGetLastError();
}

hipError_t launch_gather_rows(const float* table, const int* t_dev, int t_count, int B, int n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3(nblocks((size_t)B * n, 256)), dim3(256), 0, s, table, t_dev, t_count, B, n, out);
    return hipGetLastError();
}

hipError_t launch_pad(const float* x, int B, int H0, int D, int Hp, int Wp, int lh, int lw, float* xp, hipStream_t s) {
    hipLaunchKernelGGL(pad_kernel, dim3(nblocks((size_t)B * Hp * Wp, 256)), dim3(256), 0, s, x, B, H0, D, Hp, Wp, lh, lw, xp);
    return hipGetLastError();
}

hipError_t launch_conv_in_plain(const float* xp, const float* w, int B, int H, int W, float* out, hipStream_t s) {
    const long long M = (long long)B * H * W;
    hipLaunchKernelGGL(conv_in_plain_kernel, dim3(nblocks((size_t)M * 64, 256)), dim3(256), 0, s, xp, w, M, H, W, out);
    return hipGetLastError();
}

hipError_t launch_outc(const float* u, const float* w, float bias, long long M, float* out, hipStream_t s) {
    hipLaunchKernelGGL(outc_kernel, dim3(nblocks((size_t)M, 256)), dim3(256), 0, s, u, w, bias, M, out);
    return hipGetLastError();
}

hipError_t launch_outc_bwd(const float* deps, const float* w, long long M, float* du, hipStream_t s) {
    hipLaunchKernelGGL(outc_bwd_kernel, dim3(nblocks((size_t)M * 64, 256)), dim3(256), 0, s, deps, w, M, du);
    return hipGetLastError();
}

hipError_t launch_mse(const float* eps_pad, const float* noise, int B, int H0, int D, int Hp, int Wp, int lh, int lw,
                      float* loss, float* deps_pad, float* eps_out, hipStream_t s) {
    hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(1024), 0, s, eps_pad, noise, B, H0, D, Hp, Wp, lh, lw, loss, deps_pad, eps_out);
    return hipGetLastError();
}

hipError_t launch_pool_bwd(const float* in, const float* dout, int B, int H, int W, int C, float* din, hipStream_t s) {
    hipLaunchKernelGGL(pool_bwd_kernel, dim3(nblocks((size_t)B * H * W * C, 256)), dim3(256), 0, s, in, dout, B, H, W, C, din);
    return hipGetLastError();
}

hipError_t launch_up_bwd(const float* dcat, int ld, int B, int h, int w, int C, float* dx, hipStream_t s) {
    hipLaunchKernelGGL(up_bwd_kernel, dim3(nblocks((size_t)B * h * w * C, 256)), dim3(256), 0, s, dcat, ld, B, h, w, C, dx);
    return hipGetLastError();
}

hipError_t launch_add_cols(const float* src, int ld, int c0, long long M, int C, float* dst, hipStream_t s) {
    hipLaunchKernelGGL(add_cols_kernel, dim3(nblocks((size_t)M * C, 256)), dim3(256), 0, s, src, ld, c0, M, C, dst);
    return hipGetLastError();
}

hipError_t launch_mish_bwd(const float* dm, int nblk, int B, int ld, const float* cond, int cond_dim, float* grad_cond,
                           hipStream_t s) {
    hipLaunchKernelGGL(mish_bwd_kernel, dim3(nblocks((size_t)B * cond_dim, 256)), dim3(256), 0, s, dm, nblk, B, ld, cond,
                       cond_dim, grad_cond);
    return hipGetLastError();
}

}  // namespace spdm
