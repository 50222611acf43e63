// frame_tiles.h -- one third of a 96 x 96 x 3 frame from interleaved HWC (uint8 or fp32) to planar CHW fp32, through LDS.
// Shared by dataset.hip (spdm_dataset_gather: frames of a window out of the store) and policy.hip (spdm_policy_window: frames
// of the observation history out of the ring); the two differ only in where a frame begins.
//
// A slice is 3072 pixels.  Its bytes are read with one 16-byte load per lane, lanes contiguous, and written to LDS with
// ds_write_b128 at the same (contiguous) addresses.  Thread q of the slice then owns pixels 4q .. 4q+3: uint8, it reads the
// three dwords 3q .. 3q+2 (ds_read_b32, lane stride 3 dwords: odd, so the 32 lanes of a group fall on 32 different banks);
// fp32, it reads the three 16-byte slots 3q .. 3q+2 (ds_read_b128, lane stride 12 dwords: the 16 lanes of each of the
// instruction's lane groups fall on 16 different 4-bank slots).  Either way it ends with one float4 per channel and stores
// each with one 16-byte store, lanes contiguous within a plane.  No byte-wide and no 12-byte-stride global access.
#pragma once

#include <hip/hip_runtime.h>

namespace spdm {
namespace frame_tiles {

constexpr int THREADS = 256;                        // the workgroup a slice is written for
constexpr int FRAME_PIX = 96 * 96;                  // 9216
constexpr int SLICES = 3;                           // workgroups per frame
constexpr int SLICE_PIX = FRAME_PIX / SLICES;       // 3072: a multiple of 16 pixels, so a slice is whole 16-byte pieces in both formats
constexpr int SLICE_QUADS = SLICE_PIX / 4;          // 768 = 3 per thread
static_assert(SLICE_PIX % 16 == 0 && SLICE_QUADS % THREADS == 0, "slice shape");

// 16-byte pieces of LDS one slice of element type T needs: 9 KiB (uint8) or 36 KiB (fp32)
template <typename T> constexpr int slice_pieces() { return SLICE_PIX * 3 * (int)sizeof(T) / 16; }

template <typename T> struct Quad;
template <> struct Quad<unsigned char> {            // 12 bytes = 4 pixels x 3 channels, as three dwords
    static __device__ __forceinline__ void load(const uint4* lds, int q, float4 out[3]) {
        const unsigned* w = reinterpret_cast<const unsigned*>(lds) + 3 * q;
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
        unsigned char v[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = (unsigned char)(w0 >> (8 * k));
            v[4 + k] = (unsigned char)(w1 >> (8 * k));
            v[8 + k] = (unsigned char)(w2 >> (8 * k));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)                 // a correctly rounded division: float(k) / 255.0f == float(double(k) / 255.0)
            out[c] = make_float4(__fdiv_rn((float)v[c], 255.0f), __fdiv_rn((float)v[3 + c], 255.0f),
                                 __fdiv_rn((float)v[6 + c], 255.0f), __fdiv_rn((float)v[9 + c], 255.0f));
    }
};
template <> struct Quad<float> {                    // 12 floats, as three 16-byte slots
    static __device__ __forceinline__ void load(const uint4* lds, int q, float4 out[3]) {
        const float4* w = reinterpret_cast<const float4*>(lds) + 3 * q;
        const float4 f0 = w[0], f1 = w[1], f2 = w[2];
        out[0] = make_float4(f0.x, f0.w, f1.z, f2.y);
        out[1] = make_float4(f0.y, f1.x, f1.w, f2.z);
        out[2] = make_float4(f0.z, f1.y, f2.x, f2.w);
    }
};

// Slice `slice` of the frame whose first byte is `frame` (16-byte aligned, elements of type T) into the three planes of
// `planes` (3 x FRAME_PIX floats, 16-byte aligned).  Called by all THREADS threads of a workgroup; lds holds
// slice_pieces<T>() pieces.
template <typename T>
__device__ __forceinline__ void slice_to_planar(const void* frame, int slice, float* planes, uint4* lds) {
    constexpr int PIECES = slice_pieces<T>();                            // 576 (uint8) or 2304 (fp32) 16-byte pieces
    const uint4* src = reinterpret_cast<const uint4*>(static_cast<const char*>(frame) + (size_t)slice * SLICE_PIX * 3 * sizeof(T));
    constexpr int FULL = PIECES / THREADS, TAIL = PIECES % THREADS;      // 2 + 64 lanes (uint8) or 9 + 0 (fp32)
    uint4 v[FULL], vt = {};
#pragma unroll
    for (int k = 0; k < FULL; ++k) v[k] = src[k * THREADS + threadIdx.x];      // every load in flight before the first LDS write
    if (TAIL > 0 && (int)threadIdx.x < TAIL) vt = src[FULL * THREADS + threadIdx.x];
#pragma unroll
    for (int k = 0; k < FULL; ++k) lds[k * THREADS + threadIdx.x] = v[k];
    if (TAIL > 0 && (int)threadIdx.x < TAIL) lds[FULL * THREADS + threadIdx.x] = vt;
    __syncthreads();
    float* dst = planes + (size_t)slice * SLICE_PIX;
#pragma unroll
    for (int k = 0; k < SLICE_QUADS / THREADS; ++k) {
        const int q = k * THREADS + threadIdx.x;
        float4 o[3];
        Quad<T>::load(lds, q, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + (size_t)c * FRAME_PIX + 4 * q) = o[c];
    }
}

}  // namespace frame_tiles
}  // namespace spdm
