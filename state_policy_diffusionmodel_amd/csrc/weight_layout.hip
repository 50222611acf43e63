// weight_layout.hip -- the device side of weight loading: every kernel-layout copy of a weight is produced on the device
// from the torch-layout blob (spdm_load_weights / spdm_update_weights), and the split format's range is checked there.
//
// A WeightCopy (kernels.h) describes one copy as a gather: a logical dense array [n0][n1][n2] whose element reads the blob
// at src + sum over axes of a linear step (or a table entry: channel maps, stacked tensors), zero beyond the real extent;
// its format says how the logical elements become the destination's bytes.  One launch per format walks every copy of that
// format: a workgroup writes 1024 consecutive destination floats of one copy (coalesced write side; the reads gather).
// Pure data movement and compares -- no matrix cores.
#include "device_utils.h"

namespace spdm {

static constexpr int WL_THREADS = 256, WL_PER_THREAD = 4;
static constexpr long long WL_BLOCK_FLOATS = (long long)WL_THREADS * WL_PER_THREAD;

// the copy of this workgroup: the last entry whose first block is <= blockIdx.x (entries ascend in blk0)
__device__ inline const WeightCopy& wl_find(const WeightCopy* __restrict__ c, int n) {
    int lo = 0, hi = n - 1;
    const long long b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    return c[lo];
}

// blob offset of logical element e, or -1 where the copy holds zero
__device__ inline long long wl_src(const WeightCopy& c, const long long* __restrict__ tabs, long long e) {
    const int i2 = (int)(e % c.n[2]);
    const long long r = e / c.n[2];
    const int i1 = (int)(r % c.n[1]), i0 = (int)(r / c.n[1]);
    const int co[3] = {i0, i1, i2};
    long long off = c.src;
    for (int k = 0; k < 3; ++k) {
        if (c.tab[k] >= 0) {
            const long long t = tabs[c.tab[k] + co[k]];
            if (t < 0) return -1;
            off += t;
        } else {
            if (co[k] >= c.lim[k]) return -1;
            off += (long long)co[k] * c.stride[k];
        }
    }
    return off;
}

__device__ inline float wl_val(const WeightCopy& c, const float* __restrict__ blob, const long long* __restrict__ tabs, long long e) {
    const long long o = wl_src(c, tabs, e);
    return o < 0 ? 0.f : blob[o];
}

// hi / lo fp16 halves of x' = 128 w (conv_gemm.hip PREC_SPLIT): hi = fp16(x') round-to-nearest-even, lo = fp16(x' - hi);
// x' - hi is exact.  The library is built without denormal flushing, so subnormal weights and results convert as on the host.
__device__ inline unsigned short wl_half(float w, bool lo) {
    const float x = w * 128.0f;
    const _Float16 hi = (_Float16)x;
    const _Float16 r = lo ? (_Float16)(x - (float)hi) : hi;
    return __builtin_bit_cast(unsigned short, r);
}

// split-format float s of the copy's logical array: per 32-element chunk, 32 hi halves then 32 lo halves
__device__ inline unsigned wl_split_float(const WeightCopy& c, const float* __restrict__ blob, const long long* __restrict__ tabs,
                                          long long s) {
    const long long base = s & ~31LL;
    const int hh = (int)(s & 31) * 2;                    // half index inside the chunk's 64
    const bool lo = hh >= 32;
    const long long e = base + (lo ? hh - 32 : hh);
    const unsigned a = wl_half(wl_val(c, blob, tabs, e), lo), b = wl_half(wl_val(c, blob, tabs, e + 1), lo);
    return a | (b << 16);
}

template <int FMT>
__global__ __launch_bounds__(WL_THREADS) void weight_copy_kernel(const float* __restrict__ blob, const long long* __restrict__ tabs,
                                                                 const WeightCopy* __restrict__ copies, int n_copies) {
    const WeightCopy& c = wl_find(copies, n_copies);
    const long long d0 = ((long long)blockIdx.x - c.blk0) * WL_BLOCK_FLOATS;
    unsigned* dst = (unsigned*)c.dst;
    for (int j = 0; j < WL_PER_THREAD; ++j) {
        const long long d = d0 + j * WL_THREADS + threadIdx.x;
        if (d >= c.count) break;
        unsigned v;
        if constexpr (FMT == WL_F32) {
            const long long o = wl_src(c, tabs, d);
            v = o < 0 ? 0u : ((const unsigned*)blob)[o];        // bit copy
        } else if constexpr (FMT == WL_SPLIT) {
            v = wl_split_float(c, blob, tabs, d);
        } else if constexpr (FMT == WL_FRAG) {
            // Fragment-order copy of split-format weights [taps][N][K] for conv_wide.hip (v_mfma_f32_16x16x32_f16 B operands):
            //   block ((tap K/32 + chunk) N/16 + nb16) x {hi, lo} of 1 KiB; lane (kg 16 + l16) -> 16 bytes = 8 fp16 of row
            //   nb16 16 + l16, k = chunk 32 + kg 8 .. -- so a wave's operand load is one coalesced global_load_dwordx4.
            //   Same bytes as the split array, permuted.  (N % 16 == 0, K % 32 == 0.)
            // Inverted here: destination float d <- split float s of [taps][N][K]
            const int nch = c.K / 32, nbn = c.N / 16;
            const int jj = (int)(d & 3);
            long long r = d >> 2;
            const int l16 = (int)(r & 15), kg = (int)((r >> 4) & 3), part = (int)((r >> 6) & 1);
            r >>= 7;
            const int nb = (int)(r % nbn);
            r /= nbn;
            const int ch = (int)(r % nch), t = (int)(r / nch);
            const long long s = ((long long)t * c.N + nb * 16 + l16) * c.K + ch * 32 + part * 16 + kg * 4 + jj;
            v = wl_split_float(c, blob, tabs, s);
        } else {
            // WL_PERM_HI / WL_PERM_LO (sa_fused.hip, C = 64): fp16 [out][64] in MFMA A-fragment order, input axis permuted by
            // perm16 = 0 1 2 3 8 9 10 11 | 4 5 6 7 12 13 14 15 inside each group of 16; halves 2d, 2d + 1 share the row and group
            const long long f = d * 2;
            const int j8 = (int)(f & 7), lane = (int)((f >> 3) & 63);
            const long long blk = f >> 9;
            const int kh = lane >> 5, ks = (int)(blk & 3);
            const long long o = (blk >> 2) * 32 + (lane & 31);
            unsigned hv[2];
            for (int q = 0; q < 2; ++q) {
                const int p = 8 * kh + j8 + q;
                const int pp = (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1);
                hv[q] = wl_half(wl_val(c, blob, tabs, o * 64 + 16 * ks + pp), FMT == WL_PERM_LO);
            }
            v = hv[0] | (hv[1] << 16);
        }
        dst[d] = v;
    }
}

// flags[slot] = 1 when a logical element of the copy is outside the split format's range: !(|w| < 511), NaN included
__global__ __launch_bounds__(WL_THREADS) void weight_range_kernel(const float* __restrict__ blob, const long long* __restrict__ tabs,
                                                                  const WeightCopy* __restrict__ copies, int n_copies, int* flags) {
    const WeightCopy& c = wl_find(copies, n_copies);
    const long long d0 = ((long long)blockIdx.x - c.blk0) * WL_BLOCK_FLOATS;
    int bad = 0;
    for (int j = 0; j < WL_PER_THREAD; ++j) {
        const long long d = d0 + j * WL_THREADS + threadIdx.x;
        if (d < c.count && !(fabsf(wl_val(c, blob, tabs, d)) < 511.0f)) bad = 1;
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) flags[c.slot] = 1;
}

long long weight_copy_blocks(long long count) { return (count + WL_BLOCK_FLOATS - 1) / WL_BLOCK_FLOATS; }

hipError_t launch_weight_copies(int fmt, const float* blob, const long long* tabs, const WeightCopy* copies, int n_copies,
                                long long blocks, int* flags, hipStream_t s) {
    if (n_copies <= 0 || blocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)blocks), block(WL_THREADS);
    switch (fmt) {
        case WL_F32: weight_copy_kernel<WL_F32><<<grid, block, 0, s>>>(blob, tabs, copies, n_copies); break;
        case WL_SPLIT: weight_copy_kernel<WL_SPLIT><<<grid, block, 0, s>>>(blob, tabs, copies, n_copies); break;
        case WL_FRAG: weight_copy_kernel<WL_FRAG><<<grid, block, 0, s>>>(blob, tabs, copies, n_copies); break;
        case WL_PERM_HI: weight_copy_kernel<WL_PERM_HI><<<grid, block, 0, s>>>(blob, tabs, copies, n_copies); break;
        case WL_PERM_LO: weight_copy_kernel<WL_PERM_LO><<<grid, block, 0, s>>>(blob, tabs, copies, n_copies); break;
        case WL_RANGE: weight_range_kernel<<<grid, block, 0, s>>>(blob, tabs, copies, n_copies, flags); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace spdm
