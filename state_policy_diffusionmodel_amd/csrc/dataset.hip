// dataset.hip -- training batches assembled on the device from a dataset that lives in HBM (spdm_dataset_gather).
//
// Replaces: CarRacingDataset.__getitem__ under its DataLoader (utils/load_data.py:91-99: sample_sequence_sparse,
// utils/data_utils.py:58-62, and _normalize_position, utils/load_data.py:85-89), the np.moveaxis(img, -1, 1) of _load_data
// (:47), the DataLoader's collate, and the .float() casts of the model's prepare_*_batch (models/diffusion_ddpm.py:287-290).
//
// ONE launch.  Workgroups [0, B * n_frames * SLICES) each turn a third of one frame from interleaved HWC (uint8 or fp32) into
// planar CHW fp32; the workgroups after them do the low-dimensional rows, one thread per (sample, window row), and the first
// of those counts the ids it had to clamp.
//
// Frame staging: frame_tiles.h, shared with policy.hip.
//
// The way back, fp32 planes to uint8 pixels laid out as tiles of a contact sheet, is spdm_frames_to_bytes,
// described at its kernel below.
//
// Safety: no row number comes from the caller.  A window id is clamped into [0, n_windows - 1] and a start read from the
// table is clamped into [0, T - 1 - (seq_len - 1) step_size] before either is used, so every store row lies in [0, T).
// No atomics: outputs are indexed by batch slot and the clamp count is one workgroup's fixed-order integer sum.
#include <hip/hip_runtime.h>

#include "frame_tiles.h"
#include "kernels.h"

namespace spdm {

namespace {

using frame_tiles::FRAME_PIX;
using frame_tiles::SLICES;
constexpr int THREADS = frame_tiles::THREADS;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// first store row of batch slot b: both the id and the table's start are clamped, whatever the caller passed
__device__ __forceinline__ int window_start(const DatasetGatherArgs& a, int b) {
    const int id = clampi(a.window_id[b], 0, a.n_windows - 1);
    const int start = a.window_start != nullptr ? a.window_start[id] : id;
    return clampi(start, 0, a.max_start);
}

// the reference's (x - min) / (max - min) * 2 - 1 in float64, every operation rounded on its own (no FMA)
__device__ __forceinline__ double normalize(double x, double lo, double range) {
    return __dsub_rn(__dmul_rn(__ddiv_rn(__dsub_rn(x, lo), range), 2.0), 1.0);
}

template <typename T>
__device__ __forceinline__ void gather_slice(const DatasetGatherArgs& a, uint4* lds, int blk) {
    const int f = blk / SLICES, slice = blk - f * SLICES;             // f = b * n_frames + r < B * n_frames
    const int b = f / a.n_frames, r = f - b * a.n_frames;
    const size_t row = (size_t)window_start(a, b) + (size_t)r * a.step_size;      // < T
    frame_tiles::slice_to_planar<T>(static_cast<const char*>(a.img) + row * FRAME_PIX * 3 * sizeof(T), slice,
                                    a.image_out + (size_t)f * 3 * FRAME_PIX, lds);
}

template <typename T>                                                  // T: the image store's element, unsigned char or float
__global__ __launch_bounds__(THREADS) void dataset_gather_kernel(const DatasetGatherArgs a) {
    __shared__ uint4 lds[frame_tiles::slice_pieces<T>()];             // one slice: 9 KiB (uint8) or 36 KiB (fp32)
    __shared__ int sh_cnt[THREADS / 64];
    const int blk = blockIdx.x;
    if (blk < a.img_blocks) {                                          // uniform per workgroup
        gather_slice<T>(a, lds, blk);
        return;
    }
    const int lb = blk - a.img_blocks;
    if (a.bad != nullptr && lb == 0) {                                 // the ids and table starts that had to be clamped
        int cnt = 0;
        for (int i = threadIdx.x; i < a.B; i += THREADS) {
            const int id = a.window_id[i];
            const int cid = clampi(id, 0, a.n_windows - 1);
            const int start = a.window_start != nullptr ? a.window_start[cid] : cid;
            cnt += (id != cid || start < 0 || start > a.max_start) ? 1 : 0;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if ((threadIdx.x & 63) == 0) sh_cnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
#pragma unroll
            for (int w = 0; w < THREADS / 64; ++w) tot += sh_cnt[w];
            *a.bad = tot;
        }
    }
    const int g = lb * THREADS + threadIdx.x;                          // (sample, window row)
    if (g >= a.B * a.seq_len) return;
    const int b = g / a.seq_len, r = g - b * a.seq_len;
    const int start = window_start(a, b);
    const size_t row = (size_t)start + (size_t)r * a.step_size;       // < T
    if (r == 0 && a.start_out != nullptr) a.start_out[b] = start;
    if (a.position_out != nullptr || a.translation_out != nullptr) {
        const double range = __dsub_rn(a.pos_max, a.pos_min);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const double sn0 = normalize(a.position[(size_t)start * 2 + c], a.pos_min, range);      // translation = sn[0]
            const double sn = normalize(a.position[row * 2 + c], a.pos_min, range);
            if (a.position_out != nullptr) a.position_out[(size_t)g * 2 + c] = (float)__ddiv_rn(__dsub_rn(sn, sn0), 2.0);
            if (r == 0 && a.translation_out != nullptr) a.translation_out[(size_t)b * 2 + c] = sn0;
        }
    }
    if (a.velocity_out != nullptr) {
#pragma unroll
        for (int c = 0; c < 2; ++c) a.velocity_out[(size_t)g * 2 + c] = a.velocity[row * 2 + c];
    }
    if (a.action_out != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.action_out[(size_t)g * 3 + c] = a.action[row * 3 + c];
    }
}

// spdm_frames_to_bytes: the inverse of the gather's frame path.  Planar CHW fp32 frames become interleaved
// HWC uint8 pixels, each frame one 96 x 96 tile of a contact sheet.
//
// Replaces: the recon.permute(1, 2, 0).cpu().numpy() and imshow's own float -> 8-bit conversion of the reference's
// models/encoder/eval_autoencoder.py:91-106, frame by frame on the host.
//
// ONE launch, a third of a frame (32 pixel rows, 3072 pixels) per workgroup.  Thread q of a pass owns pixels 4q .. 4q+3: one
// 16-byte load from each of the three planes (lanes contiguous within a plane), twelve bytes out as three dwords written to
// LDS at dwords 3q .. 3q+2 (ds_write_b32, lane stride 3 dwords: odd, the 32 lanes of a group fall on 32 different banks).
// The slice is then 9216 contiguous bytes in pixel order = 32 pixel rows of 288 B = 18 16-byte pieces each; piece p is read
// back with ds_read_b128 at consecutive addresses and stored with one 16-byte store at row p / 18, piece p % 18 of the tile,
// whose rows lie cols x 288 B apart in the sheet.  Every tile row starts 16-byte aligned because 288 = 18 x 16.
__device__ __forceinline__ unsigned quantise(float x) {
    const float v = x * 255.0f;                                        // ONE fp32 multiply
    const float q = rintf(v);                                          // ties to even
    return v != v ? 0u : (unsigned)(int)fminf(fmaxf(q, 0.0f), 255.0f);
}

__global__ __launch_bounds__(THREADS) void frames_to_u8_kernel(const FramesToU8Args a) {
    constexpr int SLICE_PIX = frame_tiles::SLICE_PIX, SLICE_QUADS = frame_tiles::SLICE_QUADS;
    constexpr int PIECES = SLICE_PIX * 3 / 16, ROW_PIECES = 96 * 3 / 16;   // 576 pieces, 18 per pixel row
    __shared__ uint4 lds[PIECES];                                      // 9 KiB
    const int f = blockIdx.x / SLICES, slice = blockIdx.x - f * SLICES;    // f < n
    const float* planes = a.frames + (size_t)f * 3 * FRAME_PIX + (size_t)slice * SLICE_PIX;
    unsigned* words = reinterpret_cast<unsigned*>(lds);
#pragma unroll
    for (int k = 0; k < SLICE_QUADS / THREADS; ++k) {
        const int q = k * THREADS + threadIdx.x;                       // < 768
        float4 c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = *reinterpret_cast<const float4*>(planes + (size_t)ch * FRAME_PIX + 4 * q);
        const unsigned r0 = quantise(c[0].x), g0 = quantise(c[1].x), b0 = quantise(c[2].x);
        const unsigned r1 = quantise(c[0].y), g1 = quantise(c[1].y), b1 = quantise(c[2].y);
        const unsigned r2 = quantise(c[0].z), g2 = quantise(c[1].z), b2 = quantise(c[2].z);
        const unsigned r3 = quantise(c[0].w), g3 = quantise(c[1].w), b3 = quantise(c[2].w);
        words[3 * q + 0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);   // little endian: byte 0 is the first pixel's red
        words[3 * q + 1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
        words[3 * q + 2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
    }
    __syncthreads();
    const long long tile = a.tile_offset + f;                          // < n_tiles
    const long long trow = tile / a.cols, tcol = tile - trow * a.cols;
    const size_t pitch = (size_t)a.cols * 96 * 3;                      // bytes per sheet row
    unsigned char* dst = a.out + ((size_t)trow * 96 + (size_t)slice * (SLICE_PIX / 96)) * pitch + (size_t)tcol * 96 * 3;
    for (int p = threadIdx.x; p < PIECES; p += THREADS) {
        const int row = p / ROW_PIECES, piece = p - row * ROW_PIECES;  // row < 32, piece < 18
        *reinterpret_cast<uint4*>(dst + (size_t)row * pitch + (size_t)piece * 16) = lds[p];
    }
}

}  // namespace

hipError_t launch_frames_to_u8(const FramesToU8Args& a, hipStream_t s) {
    if (a.n < 1 || a.cols < 1 || a.tile_offset < 0 || (long long)a.n * SLICES > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(frames_to_u8_kernel, dim3((unsigned)(a.n * SLICES)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dataset_gather(DatasetGatherArgs a, hipStream_t s) {
    if (a.B < 1 || a.seq_len < 1 || a.step_size < 1 || a.n_windows < 1 || a.n_frames < 0 || a.max_start < 0) return hipErrorInvalidValue;
    const long long img_blocks = a.image_out != nullptr ? (long long)a.B * a.n_frames * SLICES : 0;
    const long long low_blocks = ((long long)a.B * a.seq_len + THREADS - 1) / THREADS;
    if (img_blocks + low_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    a.img_blocks = (int)img_blocks;
    const dim3 grid((unsigned)(img_blocks + low_blocks));
    if (a.img_dtype == 0) hipLaunchKernelGGL(dataset_gather_kernel<unsigned char>, grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL(dataset_gather_kernel<float>, grid, dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdm
