// optim.hip -- gradient clipping + Adam on the device (spdm_adam_step), and the exponential moving average of
// the weights on the same partition (spdm_ema_step, ema_apply_kernel below).
//
// Replaces: torch.nn.utils.clip_grad_norm_ (Lightning's gradient_clip_val, train.py) followed by torch.optim.Adam.step()
// (configure_optimizers, models/diffusion_ddpm.py:114-124; models/encoder/autoencoder.py:73-74) over up to four flat fp32
// segments (the U-Net blob, the encoder blob, the decoder blob).
//
// Two launches of ADAM_GRID workgroups, no atomics, no grid synchronisation:
//   grad_sumsq_kernel   partial[wg] = sum g^2 over the workgroup's range, in fp64 (skipped without clipping)
//   adam_apply_kernel   every workgroup adds partial[0 .. ADAM_GRID) in index order -- so all hold the same bits --, takes
//                       coef = min(1, max_norm / (sqrt(sum) + 1e-6)) and applies Adam to its range in fp32.
// The ranges: segment i is cut into quads of 4 floats (the last one may be short: the scalar tail), the quads of all segments
// are concatenated, and workgroup w owns quads [w per, (w + 1) per) with per = ceil(quads / ADAM_GRID).  Inside a range thread t
// takes the quads t, t + 256, ... of each segment's part in turn.  Both are pure functions of the segment sizes, so the fp64
// summation order is too: two calls on the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace spdm {

namespace {

constexpr int THREADS = 256;
typedef unsigned long long u64;

// the part of segment s (quads [base, base + nq) of the concatenation) inside the workgroup's range [lo, hi), segment-local
// (Seg: OptimSeg or EmaSeg -- only its n is read)
struct Part { u64 b, e, full; bool any; };
template <class Seg>
__device__ inline Part part_of(const Seg& sg, u64 base, u64 lo, u64 hi) {
    const u64 nq = (sg.n + 3) >> 2;
    Part p;
    p.full = sg.n >> 2;                                  // whole quads; quad `full` (if nq > full) holds the n & 3 tail floats
    const u64 b = lo > base ? lo : base, e = hi < base + nq ? hi : base + nq;
    p.any = b < e;
    p.b = p.any ? b - base : 0;
    p.e = p.any ? e - base : 0;
    return p;
}
// does this thread own the segment's short last quad?  (it is quad `full` of the thread order b + t, b + t + 256, ...)
template <class Seg>
__device__ inline bool owns_tail(const Part& p, const Seg& sg) {
    return (sg.n & 3) != 0 && p.any && p.full >= p.b && p.full < p.e && ((p.full - p.b) & (THREADS - 1)) == threadIdx.x;
}

__device__ inline double sq4(double acc, const float4 g) {
    acc += (double)g.x * (double)g.x;
    acc += (double)g.y * (double)g.y;
    acc += (double)g.z * (double)g.z;
    acc += (double)g.w * (double)g.w;
    return acc;
}

__global__ __launch_bounds__(THREADS) void grad_sumsq_kernel(const OptimArgs a, double* __restrict__ partial) {
    const u64 lo = (u64)blockIdx.x * a.per, hi = lo + a.per < a.quads ? lo + a.per : a.quads;
    double acc = 0.0;                                    // this thread's chain, in the order of the loops below
    u64 base = 0;
#pragma unroll
    for (int s = 0; s < OPTIM_MAX_SEGMENTS; ++s) {
        if (s >= a.nseg) break;
        const OptimSeg& sg = a.seg[s];
        const Part p = part_of(sg, base, lo, hi);
        base += (sg.n + 3) >> 2;
        if (!p.any) continue;
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(sg.g);
        const u64 ef = p.e < p.full ? p.e : p.full;
        u64 q = p.b + threadIdx.x;
        for (; q + 3 * THREADS < ef; q += 4 * THREADS) {      // four 16-byte loads in flight
            const float4 g0 = g4[q], g1 = g4[q + THREADS], g2 = g4[q + 2 * THREADS], g3 = g4[q + 3 * THREADS];
            acc = sq4(sq4(sq4(sq4(acc, g0), g1), g2), g3);
        }
        for (; q < ef; q += THREADS) acc = sq4(acc, g4[q]);
        if (owns_tail(p, sg))
            for (u64 i = p.full * 4; i < sg.n; ++i) acc += (double)sg.g[i] * (double)sg.g[i];
    }
    // fixed-order reduction: lanes of a wave by halving strides, then the four waves in order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double wave_sum[THREADS / 64];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wave_sum[0];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) t += wave_sum[w];
        partial[blockIdx.x] = t;                         // a workgroup without elements writes 0.0
    }
}

// torch's Adam (amsgrad = False, weight_decay = 0) on one element in fp32.  The operation sequence is pinned (no compiler
// contraction): the accumulations are explicit fused multiply-adds, the division and the square root the correctly rounded ones.
// A beta is carried as hi + lo (lo = the rounding error of the fp32 beta): 0.9f alone is 2.6e-8 low, a bias of 0.44 x 2^-24 per
// step that does not average out over the steps (measured: it doubles how often a moment ends more than one rounding away
// from float64 after five steps).  g = m = v = 0 gives m = v = 0 and p - step_size * (0 / eps) = p, bit for bit.
__device__ inline void adam1(float& p, const float g, float& m, float& v, const OptimArgs& a, const float coef) {
#pragma clang fp contract(off)
    const float gc = g * coef;
    m = fmaf(a.beta1, m, fmaf(a.beta1_lo, m, a.one_minus_beta1 * gc));
    v = fmaf(a.beta2, v, fmaf(a.beta2_lo, v, a.one_minus_beta2 * (gc * gc)));
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = fmaf(-a.step_size, m / denom, p);
}
__device__ inline void adam4(float4& p, const float4 g, float4& m, float4& v, const OptimArgs& a, const float coef) {
    adam1(p.x, g.x, m.x, v.x, a, coef);
    adam1(p.y, g.y, m.y, v.y, a, coef);
    adam1(p.z, g.z, m.z, v.z, a, coef);
    adam1(p.w, g.w, m.w, v.w, a, coef);
}

__global__ __launch_bounds__(THREADS) void adam_apply_kernel(const OptimArgs a, const double* __restrict__ partial,
                                                            double* __restrict__ norm_out) {
    float coef = 1.0f;
    if (a.clip) {
        double sum = 0.0;                                // index order, in every thread: the same bits everywhere
#pragma unroll 8
        for (int i = 0; i < ADAM_GRID; ++i) sum += partial[i];
        const double norm = sqrt(sum);
        double c = (double)a.max_norm / (norm + 1e-6);   // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
        if (c > 1.0) c = 1.0;                            // (a NaN stays a NaN and propagates, as in torch)
        coef = (float)c;
        if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = norm;
    }
    const u64 lo = (u64)blockIdx.x * a.per, hi = lo + a.per < a.quads ? lo + a.per : a.quads;
    u64 base = 0;
#pragma unroll
    for (int s = 0; s < OPTIM_MAX_SEGMENTS; ++s) {
        if (s >= a.nseg) break;
        const OptimSeg& sg = a.seg[s];
        const Part pt = part_of(sg, base, lo, hi);
        base += (sg.n + 3) >> 2;
        if (!pt.any) continue;
        float4* p4 = reinterpret_cast<float4*>(sg.p);
        const float4* g4 = reinterpret_cast<const float4*>(sg.g);
        float4* m4 = reinterpret_cast<float4*>(sg.m);
        float4* v4 = reinterpret_cast<float4*>(sg.v);
        const u64 ef = pt.e < pt.full ? pt.e : pt.full;
        u64 q = pt.b + threadIdx.x;
        for (; q + THREADS < ef; q += 2 * THREADS) {          // eight 16-byte loads in flight, then the stores
            const u64 r = q + THREADS;
            float4 p0 = p4[q], m0 = m4[q], v0 = v4[q], p1 = p4[r], m1 = m4[r], v1 = v4[r];
            const float4 g0 = g4[q], g1 = g4[r];
            adam4(p0, g0, m0, v0, a, coef);
            adam4(p1, g1, m1, v1, a, coef);
            p4[q] = p0; m4[q] = m0; v4[q] = v0;
            p4[r] = p1; m4[r] = m1; v4[r] = v1;
        }
        for (; q < ef; q += THREADS) {
            float4 p0 = p4[q], m0 = m4[q], v0 = v4[q];
            adam4(p0, g4[q], m0, v0, a, coef);
            p4[q] = p0; m4[q] = m0; v4[q] = v0;
        }
        if (owns_tail(pt, sg))
            for (u64 i = pt.full * 4; i < sg.n; ++i) adam1(sg.p[i], sg.g[i], sg.m[i], sg.v[i], a, coef);
    }
}

// One EMA update of one element: ema - omd (ema - p), the recipe s.sub_(one_minus_decay * (s - p)) of diffusion-policy code
// bases, as torch evaluates it: a subtraction, a multiplication and a subtraction, each rounded on its own (no contraction:
// fma(-omd, ema - p, ema) differs from it on about one element in a hundred at decay 0.4 .. 0.9).  NOT torch.lerp_, which
// rounds differently.  omd = 0 returns ema's bits; a NaN or an infinity in p reaches this element alone.
__device__ inline float ema1(const float e, const float p, const float omd) {
#pragma clang fp contract(off)
    const float d = e - p;
    const float s = omd * d;
    return e - s;
}
__device__ inline float4 ema4(const float4 e, const float4 p, const float omd) {
    return make_float4(ema1(e.x, p.x, omd), ema1(e.y, p.y, omd), ema1(e.z, p.z, omd), ema1(e.w, p.w, omd));
}

// adam_apply_kernel's partition over (ema, p) pairs: every element is read and written by exactly one thread, which loads its
// ema before it stores it.  Nothing is reduced, so the result does not depend on the partition at all.
__global__ __launch_bounds__(THREADS) void ema_apply_kernel(const EmaArgs a) {
    const u64 lo = (u64)blockIdx.x * a.per, hi = lo + a.per < a.quads ? lo + a.per : a.quads;
    u64 base = 0;
#pragma unroll
    for (int s = 0; s < OPTIM_MAX_SEGMENTS; ++s) {
        if (s >= a.nseg) break;
        const EmaSeg& sg = a.seg[s];
        const Part pt = part_of(sg, base, lo, hi);
        base += (sg.n + 3) >> 2;
        if (!pt.any) continue;
        float4* e4 = reinterpret_cast<float4*>(sg.ema);
        const float4* p4 = reinterpret_cast<const float4*>(sg.p);
        const u64 ef = pt.e < pt.full ? pt.e : pt.full;
        u64 q = pt.b + threadIdx.x;
        for (; q + 3 * THREADS < ef; q += 4 * THREADS) {      // eight 16-byte loads in flight, then the stores
            const u64 r1 = q + THREADS, r2 = q + 2 * THREADS, r3 = q + 3 * THREADS;
            const float4 e0 = e4[q], e1 = e4[r1], e2 = e4[r2], e3 = e4[r3];
            const float4 p0 = p4[q], p1 = p4[r1], p2 = p4[r2], p3 = p4[r3];
            e4[q] = ema4(e0, p0, a.omd);
            e4[r1] = ema4(e1, p1, a.omd);
            e4[r2] = ema4(e2, p2, a.omd);
            e4[r3] = ema4(e3, p3, a.omd);
        }
        for (; q < ef; q += THREADS) e4[q] = ema4(e4[q], p4[q], a.omd);
        if (owns_tail(pt, sg))
            for (u64 i = pt.full * 4; i < sg.n; ++i) sg.ema[i] = ema1(sg.ema[i], sg.p[i], a.omd);
    }
}

}  // namespace

hipError_t launch_ema_step(EmaArgs a, hipStream_t s) {
    a.quads = 0;
    for (int i = 0; i < a.nseg; ++i) a.quads += (a.seg[i].n + 3) >> 2;
    a.per = (a.quads + ADAM_GRID - 1) / ADAM_GRID;
    hipLaunchKernelGGL(ema_apply_kernel, dim3(ADAM_GRID), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_adam_step(OptimArgs a, double* workspace, hipStream_t s) {
    a.quads = 0;
    for (int i = 0; i < a.nseg; ++i) a.quads += (a.seg[i].n + 3) >> 2;
    a.per = (a.quads + ADAM_GRID - 1) / ADAM_GRID;
    if (a.clip) hipLaunchKernelGGL(grad_sumsq_kernel, dim3(ADAM_GRID), dim3(THREADS), 0, s, a, workspace);
    hipLaunchKernelGGL(adam_apply_kernel, dim3(ADAM_GRID), dim3(THREADS), 0, s, a, workspace, workspace + ADAM_GRID);
    return hipGetLastError();
}

}  // namespace spdm
