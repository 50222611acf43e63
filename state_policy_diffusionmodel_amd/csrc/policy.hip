// policy.hip -- the closed-loop caller's host side on the device: the observation history of E environments as rings in HBM,
// the conditioning batch built from them, and the plan back in the dataset's units (spdm_policy_push, spdm_policy_window,
// spdm_policy_unnormalize), the starting iterate of a warm-started plan (spdm_policy_warm_start; 8.18), and the
// choice of one of K candidate plans per environment (spdm_policy_select; 8.21).
//
// Replaces: the four deque(maxlen = obs_horizon step_size) of run_predictions.py:112-124 and their appends (:145-148),
// prepare_diffusion_batch (:30-60: list(deque)[::s], torch.tensor(..., float32) over every frame of the window, / 255, permute,
// normalize_data, normalize_position, all on the host, and the host-to-device copy of the result), and the .cpu() and
// unnormalize_position of :158-164.
//
// Push: ONE launch.  Workgroups [0, E x chunks) each copy up to 1024 16-byte pieces of one environment's frame, four per
// thread with all four loads in flight before the first store, into slot n % L of that environment's ring -- or, where the
// environment's fill word is set, into all L slots (the value is loaded once).  The workgroups after them write the seven
// low-dimensional floats, one thread per environment.
// Window: ONE launch.  Workgroups [0, E obs_h x 3) each turn a third of one ring frame into planar CHW fp32 (frame_tiles.h,
// shared with dataset.hip); the workgroups after them normalise the low-dimensional rows, one thread per (environment, entry).
// Unnormalise: ONE launch, one thread per (environment, predicted step), with the U and A of spdm_eval_errors (unnormalize.h).
// Warm start: ONE launch, one thread per four consecutive elements of an environment's (H, D) window: the previous plan shifted
// by the time that has passed, re-centred on the new window's first entry and noised to the level the loop's suffix starts
// from, with the Philox / Box-Muller stream of train_noise.hip (philox_normal.h) under purpose 8.
// Select: ONE launch, one workgroup per environment (described at the kernel).
//
// Arithmetic of the window: that of utils/data_utils.py:18-33 on CPU float32 torch tensors (include/spdm.h), written with the
// _rn intrinsics so that no two operations are ever contracted into an FMA.
//
// Safety: every index is built from scalars the host entry points have validated (include/spdm.h); a slot is (first + k
// step_size) mod L with first in [0, L), so it lies in [0, L).  The fill words are read, never used as an index.  No atomics.
#include <hip/hip_runtime.h>

#include "frame_tiles.h"
#include "kernels.h"
#include "philox_normal.h"
#include "unnormalize.h"

namespace spdm {

namespace {

using frame_tiles::FRAME_PIX;
using frame_tiles::SLICES;
constexpr int THREADS = frame_tiles::THREADS;
constexpr int PUSH_PER_THREAD = POLICY_PUSH_PIECES / THREADS;          // 4
static_assert(POLICY_PUSH_PIECES % THREADS == 0, "push chunk shape");

__global__ __launch_bounds__(THREADS) void policy_push_kernel(const PolicyPushArgs a) {
    const int blk = blockIdx.x;
    if (blk < a.img_blocks) {                                          // uniform per workgroup
        const int e = blk / a.chunks, chunk = blk - e * a.chunks;      // e < E
        const bool fill = a.fill[e] != 0;
        const uint4* src = static_cast<const uint4*>(a.img_in) + (size_t)e * a.frame_pieces;
        uint4* ring = static_cast<uint4*>(a.ring_img) + (size_t)e * a.L * a.frame_pieces;
        uint4 v[PUSH_PER_THREAD] = {};
        int p[PUSH_PER_THREAD];
#pragma unroll
        for (int k = 0; k < PUSH_PER_THREAD; ++k) {
            p[k] = chunk * POLICY_PUSH_PIECES + k * THREADS + threadIdx.x;
            if (p[k] < a.frame_pieces) v[k] = src[p[k]];
        }
        const int s0 = fill ? 0 : a.slot, s1 = fill ? a.L : a.slot + 1;        // slot < L: checked by the host
        for (int s = s0; s < s1; ++s) {
            uint4* dst = ring + (size_t)s * a.frame_pieces;
#pragma unroll
            for (int k = 0; k < PUSH_PER_THREAD; ++k)
                if (p[k] < a.frame_pieces) dst[p[k]] = v[k];
        }
        return;
    }
    const int e = (blk - a.img_blocks) * THREADS + threadIdx.x;
    if (e >= a.E) return;
    const bool fill = a.fill[e] != 0;
    const size_t e2 = (size_t)e * 2, e3 = (size_t)e * 3;
    const float px = a.pos_in[e2], py = a.pos_in[e2 + 1], vx = a.vel_in[e2], vy = a.vel_in[e2 + 1];
    const float a0 = a.act_in[e3], a1 = a.act_in[e3 + 1], a2 = a.act_in[e3 + 2];
    const int s0 = fill ? 0 : a.slot, s1 = fill ? a.L : a.slot + 1;
    for (int s = s0; s < s1; ++s) {
        const size_t i = (size_t)e * a.L + s;
        a.ring_pos[i * 2] = px; a.ring_pos[i * 2 + 1] = py;
        a.ring_vel[i * 2] = vx; a.ring_vel[i * 2 + 1] = vy;
        a.ring_act[i * 3] = a0; a.ring_act[i * 3 + 1] = a1; a.ring_act[i * 3 + 2] = a2;
    }
}

// normalize_data on a float32 tensor with float32 statistics: every operation a float32 operation rounded on its own
__device__ __forceinline__ float normalize_f32(float x, float lo, float range) {
    return __fsub_rn(__fmul_rn(__fdiv_rn(__fsub_rn(x, lo), range), 2.0f), 1.0f);
}

// ... with float64 statistics arrays: torch promotes to float64; the model's .float() rounds once
__device__ __forceinline__ float normalize_f64(float x, double lo, double range) {
    return (float)__dsub_rn(__dmul_rn(__ddiv_rn(__dsub_rn((double)x, lo), range), 2.0), 1.0);
}

__device__ __forceinline__ float normalize_channel(float x, double lo, double hi, int f32) {
    if (f32) return normalize_f32(x, (float)lo, __fsub_rn((float)hi, (float)lo));       // the statistics are float32 values: exact
    return normalize_f64(x, lo, __dsub_rn(hi, lo));
}

template <typename T>                                                  // T: the ring's frame element, unsigned char or float
__global__ __launch_bounds__(THREADS) void policy_window_kernel(const PolicyWindowArgs a) {
    __shared__ uint4 lds[frame_tiles::slice_pieces<T>()];              // one slice: 9 KiB (uint8) or 36 KiB (fp32)
    const int blk = blockIdx.x;
    if (blk < a.img_blocks) {                                          // uniform per workgroup
        const int f = blk / SLICES, slice = blk - f * SLICES;          // f = e * obs_h + k < E * obs_h
        const int e = f / a.obs_h, k = f - e * a.obs_h;
        const int slot = (int)(((long long)a.first + (long long)k * a.step_size) % a.L);
        const size_t frame = (size_t)e * a.L + slot;
        frame_tiles::slice_to_planar<T>(static_cast<const char*>(a.ring_img) + frame * FRAME_PIX * 3 * sizeof(T), slice,
                                        a.image_out + (size_t)f * 3 * FRAME_PIX, lds);
        return;
    }
    const int g = (blk - a.img_blocks) * THREADS + threadIdx.x;        // (environment, entry)
    if (g >= a.E * a.obs_h) return;
    const int e = g / a.obs_h, k = g - e * a.obs_h;
    const size_t row0 = (size_t)e * a.L + a.first;                                       // entry 0: the oldest
    const size_t row = (size_t)e * a.L + (int)(((long long)a.first + (long long)k * a.step_size) % a.L);
    if (a.position_out != nullptr || a.translation_out != nullptr) {
        const float lo = (float)a.pos_min, range = (float)__dsub_rn(a.pos_max, a.pos_min);       // the range is formed in float64
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float sn0 = normalize_f32(a.ring_pos[row0 * 2 + c], lo, range);           // translation = sn of entry 0
            const float sn = normalize_f32(a.ring_pos[row * 2 + c], lo, range);
            if (a.position_out != nullptr) a.position_out[(size_t)g * 2 + c] = __fdiv_rn(__fsub_rn(sn, sn0), 2.0f);
            if (k == 0 && a.translation_out != nullptr) a.translation_out[(size_t)e * 2 + c] = sn0;
        }
    }
    if (a.velocity_out != nullptr) {
#pragma unroll
        for (int c = 0; c < 2; ++c)
            a.velocity_out[(size_t)g * 2 + c] = normalize_channel(a.ring_vel[row * 2 + c], a.vel_min[c], a.vel_max[c], a.vel_f32);
    }
    if (a.action_out != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            a.action_out[(size_t)g * 3 + c] = normalize_channel(a.ring_act[row * 3 + c], a.act_min[c], a.act_max[c], a.act_f32);
    }
}

__global__ __launch_bounds__(THREADS) void policy_unnormalize_kernel(const PolicyUnnormalizeArgs a) {
    const int P = a.H - a.inp_h;
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;        // (environment, predicted step)
    if (g >= (long long)a.E * P) return;
    const int e = (int)(g / P), j = (int)(g - (long long)e * P);
    const float* x = a.x0 + ((size_t)e * a.H + a.inp_h + j) * a.D;            // inp_h + j < H
    const double range = __dsub_rn(a.pos_max, a.pos_min);
#pragma unroll
    for (int c = 0; c < 2; ++c)
        a.waypoints[(size_t)g * 2 + c] = unnormalize_position(x[c], (double)a.translation[(size_t)e * 2 + c], a.pos_min, range);
    if (a.actions != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            a.actions[(size_t)g * 3 + c] = unnormalize_action(x[2 + c], a.act_min[c], __dsub_rn(a.act_max[c], a.act_min[c]));
    }
}

// One thread per Philox quad: four consecutive elements of one environment's (H, D) window (the last quad of a window may be
// short).  No LDS, no barrier.  Rows: r + q + 1 <= 2 (H - 1) + 1 fits an int (q <= H - 1 and H D < 2^31 with D >= 2: the launch).
__global__ __launch_bounds__(THREADS) void policy_warm_start_kernel(const PolicyWarmStartArgs a) {
// every float operation written in this body is rounded on its own.  The _rn intrinsics do not promise that here: they are
// inline functions of plain operators, which the compiler contracts after inlining (it fused a + w (b - a) into an FMA)
#pragma clang fp contract(off)
    const int HD = a.H * a.D, nq = (HD >> 2) + ((HD & 3) != 0);                // HD < 2^31: the launch
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;        // (environment, quad)
    if (g >= (long long)a.E * nq) return;
    const int e = (int)(g / nq), i = (int)(g - (long long)e * nq);             // e < E, i < nq
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.noise_in == nullptr) {
        unsigned w[4];
        philox4x32_10((unsigned)i, (unsigned)(a.env_offset + (unsigned long long)e), a.draw, 8u, (unsigned)a.seed,
                      (unsigned)(a.seed >> 32), w);
        box_muller(w[0], w[1], z[0], z[1]);
        box_muller(w[2], w[3], z[2], z[3]);
    }
    const float w01 = a.f > 0 ? (float)a.f / (float)a.step_size : 0.0f;        // correctly rounded: hipcc's default for float division
    const int inp_e = a.inp_h * a.D;                     // elements [0, inp_e) of a window are the in-painted rows
    const size_t base = (size_t)e * HD;
    const float* prev = a.prev_x0 + base;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned el = ((unsigned)i << 2) + k;      // <= HD + 2: unsigned, so that a window of 2^31 - 1 elements cannot wrap
        if (el >= (unsigned)HD) break;
        const int r = (int)(el / (unsigned)a.D), c = (int)(el - (unsigned)r * a.D);      // r < H, c < D
        const int r0 = min(r + a.q, a.H - 1), r1 = min(r + a.q + (a.f > 0 ? 1 : 0), a.H - 1);
        float gs = prev[(size_t)r0 * a.D + c];
        if (a.f > 0) {                                   // uniform
            const float d = prev[(size_t)r1 * a.D + c] - gs;
            const float wd = w01 * d;
            gs = gs + wd;
        }
        if (c < 2) {                                     // the old plan's frame into the new one's: the scalings by 2 are exact
            const float sn = 2.0f * gs + a.prev_translation[(size_t)e * 2 + c];
            gs = (sn - a.translation[(size_t)e * 2 + c]) / 2.0f;
        }
        const size_t idx = base + el;
        const float zz = a.noise_in != nullptr ? a.noise_in[idx] : z[k];
        if (a.guess != nullptr) a.guess[idx] = gs;
        if (a.noise != nullptr && a.noise != a.noise_in) a.noise[idx] = zz;
        const float xa = a.sa * gs, xb = a.sb * zz;
        float x = xa + xb;
        if (el < (unsigned)inp_e) x = a.inpaint[(size_t)e * inp_e + el];       // add_constraints
        a.x[idx] = x;
    }
}

// ---- spdm_policy_select: one of K candidates per environment --------------------------------------------------
// One workgroup per environment.  Medoid: the K (K + 1) / 2 pairs j <= k are spread over the threads, each pair's distance is a
// serial float64 sum in one thread (so the bits do not depend on the mapping) and lands in a triangular table in LDS; thread j
// then adds row j of the table in k order.  Coherent: thread j sums candidate j against the guess.  The K <= 64 scores meet in
// wave 0, which picks the winner with six shuffle steps under a total order (below), and all threads copy the chosen row.
// Dynamic LDS: [64 scores][medoid: K (K + 1) / 2 distances] as doubles, then -- when it fits SELECT_LDS_BYTES -- the scored part
// of the K candidates as floats with an odd candidate stride, so that the threads of a wave, which read the same (r, c) of
// different candidates, fall on different banks, and the scored part of the guess.  The distance loops and the spread then
// read LDS; where it does not fit, the same loops read global memory.
constexpr int SELECT_LDS_BYTES = 64 * 1024;            // what a workgroup may ask for without an opt-in attribute

__host__ __device__ inline int select_pairs(int K) { return K * (K + 1) / 2; }
// candidate stride of the staged copy, in floats: odd, hence coprime to the bank count
__host__ __device__ inline int select_stage_stride(int P, int cols) { return (P * cols) | 1; }

// a beats b: the smaller score; a NaN loses against a number; on a tie, and between two NaNs, the lower index
__device__ __forceinline__ bool select_beats(double sa, int ia, double sb, int ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return sa < sb;
    return ia < ib;
}

// sum over `rows` rows of `cols` columns of (x - y)^2, r outer and c inner, each term subtract, multiply, add
template <typename PX, typename PY>
__device__ __forceinline__ double select_distance(PX x, int x_ld, PY y, int y_ld, int rows, int cols) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const double d = (double)x[r * x_ld + c] - (double)y[r * y_ld + c];
            const double dd = d * d;
            s = s + dd;
        }
    return s;
}

template <bool STAGED>
__global__ __launch_bounds__(THREADS) void policy_select_kernel(const PolicySelectArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double select_lds[];
    __shared__ int pick;
    const int e = blockIdx.x, t = threadIdx.x, K = a.K;                    // e < E: the grid
    const int P = a.H - a.inp_h, HD = a.H * a.D;                           // E K H D < 2^31: the host
    const float* xe = a.x0 + (size_t)e * K * HD;                           // candidate k: xe + k HD
    double* sc = select_lds;                                               // [64]
    double* tri = select_lds + POLICY_SELECT_MAX_K;                        // [K (K + 1) / 2]: row j holds d(j, k), k = j .. K - 1
    double mine = 0.0;                                                     // thread j < K: s_j
    const int npairs = a.mode == 0 ? select_pairs(K) : 0, n = P * a.cols;
    const int cs = select_stage_stride(P, a.cols);
    float* st = reinterpret_cast<float*>(tri + npairs);                    // [K][cs]: x_k[inp_h + r, c] at k cs + r cols + c
    float* gs = st + K * cs;                                               // coherent: [rows][cols] of the guess
    const float* g = a.mode == 1 ? a.guess + (size_t)e * (size_t)a.guess_row_stride * HD + a.inp_h * a.D : nullptr;
    if (STAGED) {
        for (int i = t; i < K * n; i += THREADS) {
            const int k = i / n, w = i - k * n, r = w / a.cols, c = w - r * a.cols;           // k < K, r < P, c < cols <= D
            st[k * cs + w] = xe[(size_t)k * HD + (a.inp_h + r) * a.D + c];
        }
        if (a.mode == 1)
            for (int i = t; i < a.rows * a.cols; i += THREADS) {
                const int r = i / a.cols, c = i - r * a.cols;                                 // r < rows <= P
                gs[i] = g[r * a.D + c];
            }
        __syncthreads();
    }
    if (a.mode == 0) {
        for (int p = t; p < npairs; p += THREADS) {
            int j = 0, rem = p, len = K;                                   // row j of the table has K - j entries
            while (rem >= len) { rem -= len; ++j; --len; }
            const int k = j + rem;                                         // j <= k < K
            if (STAGED) tri[p] = select_distance(st + j * cs, a.cols, st + k * cs, a.cols, P, a.cols);
            else tri[p] = select_distance(xe + (size_t)j * HD + a.inp_h * a.D, a.D, xe + (size_t)k * HD + a.inp_h * a.D, a.D, P, a.cols);
        }
        __syncthreads();
        if (t < K) {
            for (int k = 0; k < K; ++k) {
                const int lo = min(t, k), hi = max(t, k);
                mine = mine + tri[lo * K - lo * (lo - 1) / 2 + (hi - lo)];
            }
        }
    } else if (t < K) {                                                    // inp_h + rows <= H
        if (STAGED) mine = select_distance(st + t * cs, a.cols, gs, a.cols, a.rows, a.cols);
        else mine = select_distance(xe + (size_t)t * HD + a.inp_h * a.D, a.D, g, a.D, a.rows, a.cols);
    }
    if (t < K) {
        sc[t] = mine;
        if (a.scores != nullptr) a.scores[(size_t)e * K + t] = mine;
    }
    if (a.spread != nullptr) {
        const double range = a.pos_max - a.pos_min;
        const double tx = (double)a.translation[(size_t)e * 2], ty = (double)a.translation[(size_t)e * 2 + 1];
        for (int p = t; p < P; p += THREADS) {
            // candidate k's way-point p: x[k ld], x[k ld + 1] (cols >= 2: the staged copy holds both)
            const float* x = STAGED ? st + p * a.cols : xe + (a.inp_h + p) * a.D;
            const size_t ld = STAGED ? (size_t)cs : (size_t)HD;
            double su = 0.0, sv = 0.0;
            for (int k = 0; k < K; ++k) {
                su = su + unnormalize_position(x[k * ld], tx, a.pos_min, range);
                sv = sv + unnormalize_position(x[k * ld + 1], ty, a.pos_min, range);
            }
            const double mu = su / (double)K, mv = sv / (double)K;
            double q = 0.0;
            for (int k = 0; k < K; ++k) {
                const double du = unnormalize_position(x[k * ld], tx, a.pos_min, range) - mu;
                const double dv = unnormalize_position(x[k * ld + 1], ty, a.pos_min, range) - mv;
                const double du2 = du * du, dv2 = dv * dv;
                const double term = du2 + dv2;
                q = q + term;
            }
            a.spread[(size_t)e * P + p] = sqrt(q / (double)K);
        }
    }
    __syncthreads();                                                       // sc[] is complete
    if (t < 64) {                                                          // wave 0, all 64 lanes: lanes >= K hold a NaN and lose
        double s = t < K ? sc[t] : __longlong_as_double(0x7ff8000000000000LL);
        int idx = t;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double os = __shfl_xor(s, off);
            const int oi = __shfl_xor(idx, off);
            if (select_beats(os, oi, s, idx)) { s = os; idx = oi; }
        }
        if (t == 0) {
            idx = min(idx, K - 1);                                         // it is < K already: lane 0 beats every lane >= K
            pick = idx;
            a.chosen[e] = idx;
        }
    }
    __syncthreads();
    const float* src = xe + (size_t)pick * HD;                             // pick < K
    float* dst = a.x0_out + (size_t)e * HD;
    for (int i = t; i < HD; i += THREADS) dst[i] = src[i];
}

}  // namespace

// dynamic LDS of the select launch and whether the candidates are staged
static size_t select_lds_bytes(const PolicySelectArgs& a, bool& staged) {
    size_t bytes = sizeof(double) * (POLICY_SELECT_MAX_K + (a.mode == 0 ? select_pairs(a.K) : 0));
    const size_t stage = sizeof(float) * ((size_t)a.K * select_stage_stride(a.H - a.inp_h, a.cols) + (a.mode == 1 ? (size_t)a.rows * a.cols : 0));
    staged = bytes + stage <= (size_t)SELECT_LDS_BYTES;
    return staged ? bytes + stage : bytes;
}

hipError_t launch_policy_select(const PolicySelectArgs& a, hipStream_t s) {
    if (a.E < 1 || a.K < 1 || a.K > POLICY_SELECT_MAX_K || a.inp_h < 0 || a.H <= a.inp_h || a.D < 2 || a.cols < 2 || a.cols > a.D ||
        (a.mode != 0 && a.mode != 1) || (long long)a.H * a.D > 0x7fffffffLL || (long long)a.E * a.K > 0x7fffffffLL ||
        (long long)a.E * a.K * ((long long)a.H * a.D) > 0x7fffffffLL ||
        (a.mode == 1 && (a.guess == nullptr || a.rows < 1 || a.rows > a.H - a.inp_h || a.guess_row_stride < 1)) ||
        (a.spread != nullptr && a.translation == nullptr))
        return hipErrorInvalidValue;
    bool staged;
    const size_t lds = select_lds_bytes(a, staged);
    if (staged) hipLaunchKernelGGL(policy_select_kernel<true>, dim3((unsigned)a.E), dim3(THREADS), lds, s, a);
    else hipLaunchKernelGGL(policy_select_kernel<false>, dim3((unsigned)a.E), dim3(THREADS), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_policy_warm_start(const PolicyWarmStartArgs& a, hipStream_t s) {
    const long long HD = (long long)a.H * a.D, n = (long long)a.E * ((HD + 3) / 4);
    if (a.E < 1 || a.H < 1 || a.D < 2 || a.inp_h < 0 || a.inp_h > a.H || a.step_size < 1 || a.q < 0 || a.q > a.H - 1 || a.f < 0 ||
        a.f >= a.step_size || (long long)a.E * HD > 0x7fffffffLL)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(policy_warm_start_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_policy_push(PolicyPushArgs a, hipStream_t s) {
    if (a.E < 1 || a.L < 1 || a.slot < 0 || a.slot >= a.L || (a.img_dtype != 0 && a.img_dtype != 1)) return hipErrorInvalidValue;
    a.frame_pieces = FRAME_PIX * 3 * (a.img_dtype == 0 ? 1 : 4) / 16;
    a.chunks = (a.frame_pieces + POLICY_PUSH_PIECES - 1) / POLICY_PUSH_PIECES;
    const long long img_blocks = (long long)a.E * a.chunks, low_blocks = ((long long)a.E + THREADS - 1) / THREADS;
    if (img_blocks + low_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    a.img_blocks = (int)img_blocks;
    hipLaunchKernelGGL(policy_push_kernel, dim3((unsigned)(img_blocks + low_blocks)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_policy_window(PolicyWindowArgs a, hipStream_t s) {
    if (a.E < 1 || a.L < 1 || a.obs_h < 1 || a.step_size < 1 || a.first < 0 || a.first >= a.L) return hipErrorInvalidValue;
    const long long img_blocks = a.image_out != nullptr ? (long long)a.E * a.obs_h * SLICES : 0;
    const long long low_blocks = ((long long)a.E * a.obs_h + THREADS - 1) / THREADS;
    if (img_blocks + low_blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    a.img_blocks = (int)img_blocks;
    const dim3 grid((unsigned)(img_blocks + low_blocks));
    if (a.img_dtype == 0) hipLaunchKernelGGL(policy_window_kernel<unsigned char>, grid, dim3(THREADS), 0, s, a);
    else hipLaunchKernelGGL(policy_window_kernel<float>, grid, dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_policy_unnormalize(const PolicyUnnormalizeArgs& a, hipStream_t s) {
    const long long n = (long long)a.E * (a.H - a.inp_h);
    if (a.E < 1 || a.inp_h < 0 || a.H <= a.inp_h || n > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(policy_unnormalize_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace spdm
