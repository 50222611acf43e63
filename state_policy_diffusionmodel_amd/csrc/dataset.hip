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
// Frame staging.  A slice is 3072 pixels.  Its bytes are read with one 16-byte load per lane, lanes contiguous, and written
// to LDS with ds_write_b128 at the same (contiguous) addresses.  Thread q of the slice then owns pixels 4q .. 4q+3: uint8, it
// reads the three dwords 3q .. 3q+2 (ds_read_b32, lane stride 3 dwords: odd, so the 32 lanes of a group fall on 32 different
// banks); fp32, it reads the three 16-byte slots 3q .. 3q+2 (ds_read_b128, lane stride 12 dwords: the 16 lanes of each of the
// instruction's lane groups fall on 16 different 4-bank slots).  Either way it ends with one float4 per channel and stores
// each with one 16-byte store, lanes contiguous within a plane.  No byte-wide and no 12-byte-stride global access.
//
// Safety: no row number comes from the caller.  A window id is clamped into [0, n_windows - 1] and a start read from the
// table is clamped into [0, T - 1 - (seq_len - 1) step_size] before either is used, so every store row lies in [0, T).
// No atomics: outputs are indexed by batch slot and the clamp count is one workgroup's fixed-order integer sum.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace spdm {

namespace {

constexpr int THREADS = 256;
constexpr int FRAME_PIX = 96 * 96;                  // 9216
constexpr int SLICES = 3;                           // workgroups per frame
constexpr int SLICE_PIX = FRAME_PIX / SLICES;       // 3072: a multiple of 16 pixels, so a slice is whole 16-byte pieces in both formats
constexpr int SLICE_QUADS = SLICE_PIX / 4;          // 768 = 3 per thread
static_assert(SLICE_PIX % 16 == 0 && SLICE_QUADS % THREADS == 0, "slice shape");

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

template <typename T>
__device__ __forceinline__ void gather_slice(const DatasetGatherArgs& a, uint4* lds, int blk) {
    constexpr int PIECES = SLICE_PIX * 3 * (int)sizeof(T) / 16;        // 576 (uint8) or 2304 (fp32) 16-byte pieces
    const int f = blk / SLICES, slice = blk - f * SLICES;             // f = b * n_frames + r < B * n_frames
    const int b = f / a.n_frames, r = f - b * a.n_frames;
    const size_t row = (size_t)window_start(a, b) + (size_t)r * a.step_size;      // < T
    const uint4* src = reinterpret_cast<const uint4*>(static_cast<const char*>(a.img) +
                                                      (row * FRAME_PIX + (size_t)slice * SLICE_PIX) * 3 * sizeof(T));
    constexpr int FULL = PIECES / THREADS, TAIL = PIECES % THREADS;      // 2 + 64 lanes (uint8) or 9 + 0 (fp32)
    uint4 v[FULL], vt = {};
#pragma unroll
    for (int k = 0; k < FULL; ++k) v[k] = src[k * THREADS + threadIdx.x];      // every load in flight before the first LDS write
    if (TAIL > 0 && (int)threadIdx.x < TAIL) vt = src[FULL * THREADS + threadIdx.x];
#pragma unroll
    for (int k = 0; k < FULL; ++k) lds[k * THREADS + threadIdx.x] = v[k];
    if (TAIL > 0 && (int)threadIdx.x < TAIL) lds[FULL * THREADS + threadIdx.x] = vt;
    __syncthreads();
    float* dst = a.image_out + (size_t)f * 3 * FRAME_PIX + (size_t)slice * SLICE_PIX;
#pragma unroll
    for (int k = 0; k < SLICE_QUADS / THREADS; ++k) {
        const int q = k * THREADS + threadIdx.x;
        float4 o[3];
        Quad<T>::load(lds, q, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(dst + (size_t)c * FRAME_PIX + 4 * q) = o[c];
    }
}

template <typename T>                                                  // T: the image store's element, unsigned char or float
__global__ __launch_bounds__(THREADS) void dataset_gather_kernel(const DatasetGatherArgs a) {
    __shared__ uint4 lds[SLICE_PIX * 3 * sizeof(T) / 16];             // one slice: 9 KiB (uint8) or 36 KiB (fp32)
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
