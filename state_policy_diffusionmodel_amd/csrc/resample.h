// resample.h -- the arithmetic of nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (models/Unet_FiLmLayer.py:191)
// on a tensor with a pending GroupNorm affine, in ONE place: upcat_kernel (elementwise.hip) materialises it, conv_skinny.hip
// (PRO_UPCAT) and conv_wide.hip (UP) read their input slab through it, and all three must give the same bits.  Every
// multiply-add is written as the fused operation the compiler contracts the plain expression to (-ffp-contract=fast, as
// upcat_kernel was built before the three shared this header), so that the result does not depend on the code around the call:
//     affine   (v - mu) * sc + be                                     ->  fma(sc, v - mu, be)
//     weight   f - (float)i0,  f = scale * (float)o                   ->  fma(scale, (float)o, -(float)i0), clamped to [0, 1]
//     blend    lh0 (lw0 v00 + lw1 v01) + lh1 (lw0 v10 + lw1 v11)      ->  fma(lh0, fma(lw0, v00, lw1 v01), lh1 fma(lw0, v10, lw1 v11))
// (i0 itself is the truncated ROUNDED product scale * (float)o, as before.)
#pragma once
#include <hip/hip_runtime.h>

namespace spdm {

// one element of a pending GroupNorm(1, C) affine: sc = rstd * gamma, formed by the caller
__device__ __forceinline__ float affine1(float v, float mu, float sc, float be) { return __builtin_fmaf(sc, v - mu, be); }

// source-index step per output index of one axis (align_corners=True): (n_in - 1) / (n_out - 1)
__device__ __forceinline__ float up_scale(int n_in, int n_out) { return (n_out > 1) ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }

// the two source indices (the second clamped to the last one) and weights of output index o along one axis
struct UpAxis { int i0, i1; float l0, l1; };
__device__ __forceinline__ UpAxis up_axis(float scale, int o, int n_in) {
    UpAxis x;
    const float f = scale * (float)o;
    x.i0 = (int)f;
    x.i1 = x.i0 + (x.i0 < n_in - 1 ? 1 : 0);
    x.l1 = fminf(fmaxf(__builtin_fmaf(scale, (float)o, -(float)x.i0), 0.f), 1.f);
    x.l0 = 1.f - x.l1;
    return x;
}

// v{h}{w}: the four (finished) source values at rows h.i0 / h.i1, columns w.i0 / w.i1
__device__ __forceinline__ float up_blend(const UpAxis& h, const UpAxis& w, float v00, float v01, float v10, float v11) {
    return __builtin_fmaf(h.l0, __builtin_fmaf(w.l0, v00, w.l1 * v01), h.l1 * __builtin_fmaf(w.l0, v10, w.l1 * v11));
}

}  // namespace spdm
