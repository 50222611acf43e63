// train_attn.hip -- the SelfAttention kernels of the training-loss gradient of UNet_Film (spdm_train_loss_grad on a handle
// created with SPDM_FLAG_TRAIN_ATTENTION; SelfAttention.forward, models/Unet_FiLmLayer.py:71-82).
//
// The block's four Linear layers run on the forward GEMM kernels (spdm_api.hip, exact fp32 path, transposed weight copies for
// the data gradients; launch_wgrad / launch_colsum for the weight and bias gradients).  This file supplies the rest, all exact
// fp32 on the VALU:
//   - LayerNorm forward with its per-row mean and 1 / std kept, and its backward (the residual gradient added in the same pass;
//     the affine gradients as per-workgroup partials that launch_colsum adds in a fixed order);
//   - the backward of the exact erf GELU;
//   - the attention core forward with the per-(sample, head, query) log-sum-exp of the scaled scores, and its backward, which
//     recomputes P = exp(q k^T / sqrt(d) - lse) instead of storing L x L per head.
// No float atomics and every reduction in a fixed order: two calls with the same inputs give the same bits.
#include <algorithm>

#include "device_utils.h"

namespace spdm {

__device__ __forceinline__ float ta_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- LayerNorm(C) over rows of C = 64 CPL channels: one wave per row, lane l owns channels l + 64 k ------------------------
template <int CPL>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                     const float* __restrict__ b, float* __restrict__ y, float* __restrict__ mean,
                                                     float* __restrict__ rstd, long long rows) {
    constexpr int C = 64 * CPL;
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * C;
    float v[CPL];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { v[k] = xr[lane + 64 * k]; s += v[k]; }
    const float mu = ta_wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) { const float d = v[k] - mu; q += d * d; }
    const float rs = 1.0f / sqrtf(ta_wave_sum(q) / (float)C + 1e-5f);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int c = lane + 64 * k;
        y[r * C + c] = (v[k] - mu) * rs * g[c] + b[c];
    }
    if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
}

// dx = rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat)) (+ add); per workgroup of rpb rows: part[blk] = [sum g xhat | sum g]
template <int CPL>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                     const float* __restrict__ gy, const float* __restrict__ add,
                                                     float* __restrict__ dx, float* __restrict__ part, long long rows, int rpb) {
    constexpr int C = 64 * CPL;
    __shared__ float red[4][2 * C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float dg[CPL], db[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) { dg[k] = 0.f; db[k] = 0.f; }
    const long long r0 = (long long)blockIdx.x * rpb;
    const long long r1 = std::min<long long>(r0 + rpb, rows);
    for (long long r = r0 + wave; r < r1; r += 4) {
        const float mu = mean[r], rs = rstd[r];
        float xh[CPL], gg[CPL];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lane + 64 * k;
            xh[k] = (x[r * C + c] - mu) * rs;
            const float gv = gy[r * C + c];
            gg[k] = gv * gamma[c];
            s1 += gg[k];
            s2 += gg[k] * xh[k];
            dg[k] += gv * xh[k];
            db[k] += gv;
        }
        s1 = ta_wave_sum(s1) / (float)C;
        s2 = ta_wave_sum(s2) / (float)C;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lane + 64 * k;
            float v = rs * (gg[k] - s1 - xh[k] * s2);
            if (add) v += add[r * C + c];
            dx[r * C + c] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) { red[wave][lane + 64 * k] = dg[k]; red[wave][C + lane + 64 * k] = db[k]; }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * C; i += 256)
        part[(size_t)blockIdx.x * 2 * C + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

int ln_bwd_blocks(long long rows) { return (int)((rows + LN_BWD_ROWS - 1) / LN_BWD_ROWS); }

hipError_t launch_ln_fwd(const float* x, const float* g, const float* b, long long rows, int C, float* y, float* mean, float* rstd,
                         hipStream_t s) {
    if (rows <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch (C) {
        case 64: hipLaunchKernelGGL(ln_fwd_kernel<1>, grid, block, 0, s, x, g, b, y, mean, rstd, rows); break;
        case 128: hipLaunchKernelGGL(ln_fwd_kernel<2>, grid, block, 0, s, x, g, b, y, mean, rstd, rows); break;
        case 256: hipLaunchKernelGGL(ln_fwd_kernel<4>, grid, block, 0, s, x, g, b, y, mean, rstd, rows); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ln_bwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* gy,
                         const float* add, long long rows, int C, float* dx, float* part, hipStream_t s) {
    if (rows <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)ln_bwd_blocks(rows)), block(256);
    switch (C) {
        case 64: hipLaunchKernelGGL(ln_bwd_kernel<1>, grid, block, 0, s, x, mean, rstd, gamma, gy, add, dx, part, rows, LN_BWD_ROWS); break;
        case 128: hipLaunchKernelGGL(ln_bwd_kernel<2>, grid, block, 0, s, x, mean, rstd, gamma, gy, add, dx, part, rows, LN_BWD_ROWS); break;
        case 256: hipLaunchKernelGGL(ln_bwd_kernel<4>, grid, block, 0, s, x, mean, rstd, gamma, gy, add, dx, part, rows, LN_BWD_ROWS); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- GELU (erf) backward: du = dh (Phi(u) + u phi(u)) ---------------------------------------------------------------------
__global__ void gelu_bwd_kernel(const float* __restrict__ u, const float* __restrict__ dh, float* __restrict__ du, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = u[i];
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * expf(-0.5f * v * v);
    du[i] = dh[i] * (cdf + v * pdf);
}

hipError_t launch_gelu_bwd(const float* u, const float* dh, size_t n, float* du, hipStream_t s) {
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, u, dh, du, n);
    return hipGetLastError();
}

// ---- attention core ---------------------------------------------------------------------------------------------------------
// One workgroup per (sample, head); one thread per query (or key) row, looping when L exceeds the workgroup.  The rows of the
// head staged in LDS are read by every lane of a wave at the same address (broadcast).  qkv [B L][3C] in in_proj's packed
// layout (q | k | v, head hd at columns hd d of each third), out / dout [B L][C], lse [B heads][L].
template <int D>
__device__ __forceinline__ float ta_dot(const float* a, const float* __restrict__ b) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int k = 0; k < D; k += 4) { s0 += a[k] * b[k]; s1 += a[k + 1] * b[k + 1]; s2 += a[k + 2] * b[k + 2]; s3 += a[k + 3] * b[k + 3]; }
    return (s0 + s1) + (s2 + s3);
}

template <int D>
__global__ __launch_bounds__(256) void attn_fwd_lse_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                           float* __restrict__ lse, int L, int C, int heads) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // K [L][D], V [L][D]
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int bh = blockIdx.x, b = bh / heads, hd = bh - b * heads;
    const size_t ld = (size_t)3 * C;
    const float* base = qkv + (size_t)b * L * ld + hd * D;
    float* Ks = sm;
    float* Vs = sm + (size_t)L * D;
    for (int i = tid; i < L * D; i += nthr) {
        const int j = i / D, k = i - j * D;
        Ks[i] = base[j * ld + C + k];
        Vs[i] = base[j * ld + 2 * C + k];
    }
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)D);
    for (int qi = tid; qi < L; qi += nthr) {
        float q[D], o[D];
#pragma unroll
        for (int k = 0; k < D; ++k) { q[k] = base[(size_t)qi * ld + k] * scale; o[k] = 0.f; }
        float m = -INFINITY;
        for (int j = 0; j < L; ++j) m = fmaxf(m, ta_dot<D>(q, Ks + j * D));
        float l = 0.f;
        for (int j = 0; j < L; ++j) {
            const float p = expf(ta_dot<D>(q, Ks + j * D) - m);
            l += p;
            const float* vr = Vs + j * D;
#pragma unroll
            for (int k = 0; k < D; ++k) o[k] += p * vr[k];
        }
        const float inv = 1.0f / l;
        float* orow = out + ((size_t)b * L + qi) * C + hd * D;
#pragma unroll
        for (int k = 0; k < D; ++k) orow[k] = o[k] * inv;
        lse[(size_t)bh * L + qi] = m + logf(l);
    }
}

// dqkv: dQ = dS K / sqrt(d), dK = dS^T Q / sqrt(d), dV = P^T dO with dS = P o (dO V^T - rowsum(dO o O)).  dQ by query rows,
// dK and dV by key rows: each sum runs inside one thread, in key (query) order.
template <int D>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                       const float* __restrict__ dout, const float* __restrict__ lse,
                                                       float* __restrict__ dqkv, int L, int C, int heads) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // Q / sqrt(d), K, V, dO [L][D] each; lse [L]; Di [L]
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int bh = blockIdx.x, b = bh / heads, hd = bh - b * heads;
    const size_t ld = (size_t)3 * C;
    const float* base = qkv + (size_t)b * L * ld + hd * D;
    const size_t row0 = (size_t)b * L;
    float* Qs = sm;
    float* Ks = Qs + (size_t)L * D;
    float* Vs = Ks + (size_t)L * D;
    float* dOs = Vs + (size_t)L * D;
    float* Ls = dOs + (size_t)L * D;
    float* Ds = Ls + L;
    const float scale = 1.0f / sqrtf((float)D);
    for (int i = tid; i < L * D; i += nthr) {
        const int j = i / D, k = i - j * D;
        Qs[i] = base[j * ld + k] * scale;
        Ks[i] = base[j * ld + C + k];
        Vs[i] = base[j * ld + 2 * C + k];
        dOs[i] = dout[(row0 + j) * C + hd * D + k];
    }
    for (int i = tid; i < L; i += nthr) {
        const float* orow = o + (row0 + i) * C + hd * D;
        const float* grow = dout + (row0 + i) * C + hd * D;
        float s = 0.f;
        for (int k = 0; k < D; ++k) s += grow[k] * orow[k];
        Ds[i] = s;
        Ls[i] = lse[(size_t)bh * L + i];
    }
    __syncthreads();
    for (int qi = tid; qi < L; qi += nthr) {
        float q[D], g[D], dq[D];
#pragma unroll
        for (int k = 0; k < D; ++k) { q[k] = Qs[qi * D + k]; g[k] = dOs[qi * D + k]; dq[k] = 0.f; }
        const float li = Ls[qi], di = Ds[qi];
        for (int j = 0; j < L; ++j) {
            const float* kr = Ks + j * D;
            const float p = expf(ta_dot<D>(q, kr) - li);
            const float ds = p * (ta_dot<D>(g, Vs + j * D) - di);
#pragma unroll
            for (int k = 0; k < D; ++k) dq[k] += ds * kr[k];
        }
        float* dst = dqkv + (row0 + qi) * ld + hd * D;
#pragma unroll
        for (int k = 0; k < D; ++k) dst[k] = dq[k] * scale;
    }
    for (int kj = tid; kj < L; kj += nthr) {
        float kk[D], vv[D], dk[D], dv[D];
#pragma unroll
        for (int k = 0; k < D; ++k) { kk[k] = Ks[kj * D + k]; vv[k] = Vs[kj * D + k]; dk[k] = 0.f; dv[k] = 0.f; }
        for (int i = 0; i < L; ++i) {
            const float* qr = Qs + i * D;
            const float* gr = dOs + i * D;
            const float p = expf(ta_dot<D>(qr, kk) - Ls[i]);
            const float ds = p * (ta_dot<D>(gr, vv) - Ds[i]);
#pragma unroll
            for (int k = 0; k < D; ++k) { dk[k] += ds * qr[k]; dv[k] += p * gr[k]; }
        }
        float* dst = dqkv + (row0 + kj) * ld + hd * D;
#pragma unroll
        for (int k = 0; k < D; ++k) { dst[C + k] = dk[k]; dst[2 * C + k] = dv[k]; }
    }
}

static int ta_threads(int L) { return std::min(256, (L + 63) / 64 * 64); }

size_t attn_train_lds_bytes(int L, int C, int heads) {
    const size_t d = (size_t)C / heads;
    return sizeof(float) * (4 * (size_t)L * d + 2 * (size_t)L);       // the backward kernel's (the forward stages half of it)
}

bool attn_train_supported(int L, int C, int heads) {
    if (L < 1 || L > 512 || heads < 1 || C % heads != 0) return false;
    const int d = C / heads;
    return (d == 16 || d == 32 || d == 64) && attn_train_lds_bytes(L, C, heads) <= 160 * 1024;
}

hipError_t launch_attn_fwd_lse(const float* qkv, float* out, float* lse, int B, int L, int C, int heads, hipStream_t s) {
    if (B <= 0 || !attn_train_supported(L, C, heads)) return hipErrorInvalidValue;
    const int d = C / heads;
    const size_t lds = sizeof(float) * 2 * (size_t)L * d;
    const dim3 grid(B * heads), block(ta_threads(L));
#define SPDM_TA(DD)                                                                                           \
    {                                                                                                         \
        auto kern = attn_fwd_lse_kernel<DD>;                                                                  \
        if (lds > 64 * 1024)                                                                                  \
            if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern)); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, s, qkv, out, lse, L, C, heads);                            \
    }
    switch (d) {
        case 16: SPDM_TA(16) break;
        case 32: SPDM_TA(32) break;
        case 64: SPDM_TA(64) break;
        default: return hipErrorInvalidValue;
    }
#undef SPDM_TA
    return hipGetLastError();
}

hipError_t launch_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int L,
                           int C, int heads, hipStream_t s) {
    if (B <= 0 || !attn_train_supported(L, C, heads)) return hipErrorInvalidValue;
    const int d = C / heads;
    const size_t lds = attn_train_lds_bytes(L, C, heads);
    const dim3 grid(B * heads), block(ta_threads(L));
#define SPDM_TA(DD)                                                                                           \
    {                                                                                                         \
        auto kern = attn_bwd_kernel<DD>;                                                                      \
        if (lds > 64 * 1024)                                                                                  \
            if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern)); e != hipSuccess) return e; \
        hipLaunchKernelGGL(kern, grid, block, lds, s, qkv, out, dout, lse, dqkv, L, C, heads);                \
    }
    switch (d) {
        case 16: SPDM_TA(16) break;
        case 32: SPDM_TA(32) break;
        case 64: SPDM_TA(64) break;
        default: return hipErrorInvalidValue;
    }
#undef SPDM_TA
    return hipGetLastError();
}

}  // namespace spdm
