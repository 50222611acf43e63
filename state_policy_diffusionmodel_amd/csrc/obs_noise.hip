// obs_noise.hip -- uniform noise added to the observations of a batch of windows on the device (spdm_obs_noise).
//
// Replaces: the head of the loop of evaluation/eval_robustness.py:174-190 -- four times
// batch[k] = batch[k] + torch.rand_like(batch[k]) * scaling_factor, for the frames, the position, the velocity and the action.
//
// ONE launch for up to four tensors:  dst[row][e] = src[row][e] + alpha * u(row_offset + row, e)  for e < inner, rows strided on
// both sides, in place or out of place.  Randomness is Philox4x32-10 with key = (seed lo, seed hi) and counter
// (q, row_offset + row, draw, 4 + tensor): q = e / 4 and element e takes word e % 4 -- ONE Philox per four elements, as in
// train_noise.hip, whose purposes 0 .. 3 these streams stay apart from.  u = (float)(w >> 8) * 2^-24 is exact, in [0, 1).
// The product and the sum are two float32 roundings (FMA contraction is off for the whole file), so
// tests/obs_noise_ref.py gives the same bits from numpy.
//
// Work: a work item is one quad of one row.  A workgroup takes OBS_NOISE_ITEMS quads: of a long row (the frames) one chunk, so
// a row is spread over many workgroups; of short rows (position, velocity, action) as many whole rows as fit.  Where the
// pointers, the strides and inner are multiples of four floats a quad is one 16-byte load and one 16-byte store; otherwise
// its elements move one by one, which also finishes a last quad of 1 .. 3 elements.  Both paths give element e word e % 4 of
// quad e / 4: alignment never changes a value.
//
// Elementwise: no LDS, no barrier, no atomics; an element is read and written by the same thread, so dst == src is safe.
// Safety: every index is built from scalars the host entry point has validated (include/spdm.h); nothing read from device
// memory is used as an index, and elements at or beyond inner are neither read nor written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

#pragma clang fp contract(off)

namespace spdm {

namespace {

constexpr int THREADS = 256;
constexpr int QUADS = OBS_NOISE_ITEMS / THREADS;         // quads per thread, their loads issued before the first Philox

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// (w >> 8) 2^-24: a 24-bit integer converts exactly and the scaling is a change of exponent, so u is exact, in [0, 1)
__device__ __forceinline__ float u01(unsigned w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }

__device__ __forceinline__ float perturb(float x, float alpha, unsigned w) {
    const float p = alpha * u01(w);                      // rounded ...
    return x + p;                                        // ... and rounded again
}

__global__ __launch_bounds__(THREADS) void obs_noise_kernel(const ObsNoiseArgs a) {
    int t = 0;                                           // the tensor of this workgroup: uniform
#pragma unroll
    for (int i = 1; i < OBS_NOISE_MAX_TENSORS; ++i)
        if (i < a.n_tensors && blockIdx.x >= a.t[i].block_begin) t = i;
    ObsNoiseTensor T = a.t[0];
#pragma unroll
    for (int i = 1; i < OBS_NOISE_MAX_TENSORS; ++i)
        if (t == i) T = a.t[i];
    const unsigned blk = blockIdx.x - T.block_begin;
    // long rows (nq >= ITEMS): chunks_per_row workgroups per row, rows_per_block = 1;  short rows: the reverse
    const unsigned long long row0 = (unsigned long long)(blk / T.chunks_per_row) * T.rows_per_block;
    const unsigned long long q0 = (unsigned long long)(blk % T.chunks_per_row) * OBS_NOISE_ITEMS;
    const bool short_rows = T.nq < (unsigned)OBS_NOISE_ITEMS;
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32);
    const unsigned purpose = 4u + (unsigned)t;

    unsigned long long row[QUADS];
    unsigned q[QUADS];
    bool live[QUADS];
#pragma unroll
    for (int j = 0; j < QUADS; ++j) {
        const unsigned o = threadIdx.x + j * THREADS;    // < ITEMS
        unsigned r = 0, qi = o;
        if (short_rows) {
            r = o / T.nq;
            qi = o - r * T.nq;
        }
        row[j] = row0 + r;
        const unsigned long long qq = q0 + qi;
        q[j] = (unsigned)qq;                             // < nq <= 2^32 - 1 where live
        live[j] = r < T.rows_per_block && qq < T.nq && row[j] < a.n_rows;
    }

    if (T.vec) {                                         // uniform
        float4 x[QUADS];
#pragma unroll
        for (int j = 0; j < QUADS; ++j)
            if (live[j]) x[j] = *reinterpret_cast<const float4*>(T.src + row[j] * T.src_stride + ((size_t)q[j] << 2));
#pragma unroll
        for (int j = 0; j < QUADS; ++j) {
            if (!live[j]) continue;
            unsigned w[4];
            philox4x32_10(q[j], (unsigned)(a.row_offset + row[j]), a.draw, purpose, k0, k1, w);
            float4 y;
            y.x = perturb(x[j].x, a.alpha, w[0]);
            y.y = perturb(x[j].y, a.alpha, w[1]);
            y.z = perturb(x[j].z, a.alpha, w[2]);
            y.w = perturb(x[j].w, a.alpha, w[3]);
            *reinterpret_cast<float4*>(T.dst + row[j] * T.dst_stride + ((size_t)q[j] << 2)) = y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < QUADS; ++j) {
            if (!live[j]) continue;
            unsigned w[4];
            philox4x32_10(q[j], (unsigned)(a.row_offset + row[j]), a.draw, purpose, k0, k1, w);
            const unsigned long long e0 = (unsigned long long)q[j] << 2;
            const float* src = T.src + row[j] * T.src_stride + e0;
            float* dst = T.dst + row[j] * T.dst_stride + e0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < (unsigned long long)T.inner) dst[k] = perturb(src[k], a.alpha, w[k]);
        }
    }
}

}  // namespace

bool plan_obs_noise(ObsNoiseArgs& a) {
    if (a.n_rows < 1 || a.n_rows > 0x100000000ull || a.n_tensors < 1 || a.n_tensors > OBS_NOISE_MAX_TENSORS) return false;
    unsigned long long blocks = 0;
    for (int i = 0; i < a.n_tensors; ++i) {
        ObsNoiseTensor& T = a.t[i];
        const unsigned long long nq = (T.inner + 3) >> 2;
        if (nq > 0xffffffffull || T.src_stride < T.inner || T.dst_stride < T.inner) return false;
        T.nq = (unsigned)nq;
        T.block_begin = (unsigned)blocks;
        T.chunks_per_row = T.rows_per_block = 1;
        T.vec = ((reinterpret_cast<uintptr_t>(T.src) | reinterpret_cast<uintptr_t>(T.dst)) & 15) == 0 &&
                ((T.inner | T.src_stride | T.dst_stride) & 3) == 0;
        if (nq == 0) continue;                           // no workgroups; its purpose stays reserved
        unsigned long long n;
        if (nq >= (unsigned long long)OBS_NOISE_ITEMS) {
            T.chunks_per_row = (unsigned)((nq + OBS_NOISE_ITEMS - 1) / OBS_NOISE_ITEMS);             // <= 2^22
            n = a.n_rows * T.chunks_per_row;                                                         // n_rows <= 2^32
        } else {
            T.rows_per_block = (unsigned)(OBS_NOISE_ITEMS / nq);
            n = (a.n_rows + T.rows_per_block - 1) / T.rows_per_block;
        }
        blocks += n;
        if (blocks > 0x7fffffffull) return false;
    }
    a.blocks = (unsigned)blocks;
    return true;
}

hipError_t launch_obs_noise(const ObsNoiseArgs& a, hipStream_t s) {
    if (a.blocks == 0) return hipSuccess;                // every inner is 0: nothing to perturb
    hipLaunchKernelGGL(obs_noise_kernel, dim3(a.blocks), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdm
