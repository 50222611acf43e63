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

}  // namespace

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
