// conv_chain.hip -- a chain of 3-tap convolutions of the width-1 level as ONE kernel per 64-row block.
//
// At this level a sample is HW = 4 (8, ...) rows, so a 64-row block holds whole samples and the GroupNorm(1, C) between two
// convolutions (models/Unet_FiLmLayer.py:101-115) needs no kernel boundary: one 8-wave workgroup owns the block and runs the
// whole list of layers on it, the activations never leaving LDS.  Same math, operand formats and scales as conv_wide.hip
// (split-fp16 operands, hi*hi + hi*lo + lo*hi into one fp32 accumulator, activations x 2^4, weights x 2^7):
//   * the current layer's input is in LDS, normalised, activated and split, chunk-major ([K / 32][64 rows][144 bytes], each row
//     32 fp16 hi | 32 fp16 lo | pad -- the slab row of conv_wide.hip); a vertical tap is a row shift of +-1, and a tap that would
//     leave the sample (h = 0 upwards, h = HW - 1 downwards) reads the all-zero row through a per-lane mask, so no tap reaches
//     another sample's rows and the slab has no halo;
//   * the weights are the WL_FRAG blocks conv_wide.hip reads (weight_layout.hip), loaded by each wave for its own column strip
//     straight into registers, one k-step (tap, chunk) ahead; the first fragments of the NEXT layer are requested before the
//     layer boundary, which they do not depend on;
//   * wave w owns the 64-row x (16 NCT)-column strip of 16-column tiles [w NCT, (w + 1) NCT), NCT = 1, 2 or 4 by the layer's
//     width; a wave whose strip lies past the layer's last column sits the layer out (narrow layers);
//   * layer boundary: per (wave, 4-row unit) fp32 sums of x and x^2 -- a lane's four accumulator registers are four consecutive
//     rows, one unit --, added over the eight waves and the units of a sample in fp64 in a fixed order, mean / rstd as every
//     other kernel forms them, then (v - mu) (rs gamma) + beta, GELU where the layer asks, split, written back over the input;
//   * the last layer stores its raw fp32 tile through LDS (16 bytes per lane) and one fp64 {sum x, sum x^2} slot per sample:
//     an ordinary tensor with a pending GroupNorm, StatsRef{m_tile = 64, n_tiles = 1};
//   * no atomics, nothing between workgroups; a ragged last block clamps nothing it stores: rows past M are staged as zeros
//     (they are whole dead samples) and neither stored nor counted.
#include "device_utils.h"

namespace spdm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr float ACT_SCALE = 16.0f;            // same scales as conv_wide.hip / conv_gemm.hip
constexpr float DESCALE = 1.0f / 2048.0f;
constexpr int CK = 32;
constexpr int ROWS = 64;                      // rows of a block
constexpr int LDK = 36;                       // floats per slab row (144 bytes)
constexpr int NTHR = 512, NWAVE = 8;
constexpr int MAXC = 512;                     // widest layer
constexpr int SLAB = (MAXC / CK) * ROWS * LDK;               // floats of the activation slab
constexpr int UNITS = ROWS / 4;               // 4-row units of a block
constexpr int LDS_FLOATS = SLAB + LDK + NWAVE * UNITS * 2 + 2 * UNITS;
static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "one workgroup per CU");
static_assert(ROWS * (MAXC + 4) <= SLAB, "the output tile fits the slab");

__device__ __forceinline__ f32x2 split2(float a, float b) {
    unsigned h, l;
    split_pair_f16(a * ACT_SCALE, b * ACT_SCALE, h, l);
    return f32x2{__builtin_bit_cast(float, h), __builtin_bit_cast(float, l)};
}

__device__ __forceinline__ int chain_nct(int N) { return N <= 128 ? 1 : N <= 256 ? 2 : 4; }

// B ring slot 0 <- the wave's fragments of step (tap 0, chunk 0) of layer L
__device__ __forceinline__ void chain_preload(f16x8 (&fb)[2][4][2], const ChainLayer& L, int wave, int lane) {
    const int nct = chain_nct(L.N);
    if (wave * nct * 16 >= L.N) return;
    asm volatile("" : "+v"(lane));             // (the lane's byte offset is formed here, not carried through the MFMA loops)
    const float* p = L.wfrag + (size_t)(wave * nct * 2) * 256 + lane * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < nct) {
            fb[0][c][0] = *reinterpret_cast<const f16x8*>(p + c * 512);
            fb[0][c][1] = *reinterpret_cast<const f16x8*>(p + c * 512 + 256);
        }
}

// One layer of the chain on the block's slab.  NCT: 16-column tiles per wave.
template <int NCT>
__device__ __forceinline__ void chain_layer(const ChainArgs& a, const int li, float* smem, f16x8 (&fb)[2][4][2], const unsigned am,
                                            const int m0, const int lhw, const bool no_mfma) {
    float* slab = smem;
    float* spart = smem + SLAB + LDK;             // [NWAVE][UNITS][2]
    float* smean = spart + NWAVE * UNITS * 2;     // [UNITS] (one per sample; HW >= 4)
    float* srstd = smean + UNITS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kg = lane >> 4;
    const ChainLayer& L = a.layer[li];
    const int K = L.K, N = L.N, nchunks = K / CK;
    const bool last = (li + 1 == a.n_layers);
    const bool active = wave * NCT * 16 < N;      // wave-uniform

    f32x4 acc[4][NCT];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int c = 0; c < NCT; ++c) acc[rt][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (active) {
        // B operand: fragment-order weights, block ((tap nchunks + chunk) N/16 + nb16) x {hi, lo} of 256 floats
        int lane_o = lane;
        asm volatile("" : "+v"(lane_o));
        const float* wfl = L.wfrag + (size_t)(wave * NCT * 2) * 256 + lane_o * 4;
        const size_t wtap = (size_t)(N >> 4) * 512;                 // floats per (tap, chunk)
        // A operand of row tile rt through tap t (dh = t - 1): lane (l16, kg) reads 16 bytes (8 fp16 of k = 8 kg ..) of slab
        // row chunk 64 + rt 16 + l16 + dh, or of the all-zero row where the tap leaves the sample
        const int aoff0 = l16 * LDK + kg * 4, zoff = SLAB + kg * 4;
        f16x8 fa[2][2];
#define CHAIN_LOAD_B(slot_, chunk_, tap_)                                                            \
        {                                                                                            \
            const float* p_ = wfl + (size_t)((tap_) * nchunks + (chunk_)) * wtap;                    \
            _Pragma("unroll") for (int c_ = 0; c_ < NCT; ++c_) {                                    \
                fb[slot_][c_][0] = *reinterpret_cast<const f16x8*>(p_ + c_ * 512);                   \
                fb[slot_][c_][1] = *reinterpret_cast<const f16x8*>(p_ + c_ * 512 + 256);             \
            }                                                                                        \
        }
#define CHAIN_LOAD_A(slot_, chunk_, tap_, rt_)                                                       \
        {                                                                                            \
            const bool ok_ = ((tap_) == 1) || (((am_o >> (2 * (rt_) + ((tap_) >> 1))) & 1u) != 0u);  \
            const int o_ = ok_ ? aoff_o + ((chunk_) * ROWS + (rt_) * 16 + (tap_) - 1) * LDK : zoff;  \
            fa[slot_][0] = *reinterpret_cast<const f16x8*>(slab + o_);                               \
            fa[slot_][1] = *reinterpret_cast<const f16x8*>(slab + o_ + 16);                          \
        }
        int aoff_o = aoff0;
        unsigned am_o = am;
        CHAIN_LOAD_A(0, 0, 0, 0)
        // two chunks = six steps per trip (K % 64 == 0: host), so every ring slot is a compile-time register set and step 0
        // of every layer lands in slot 0
        for (int cp = 0; cp < nchunks; cp += 2) {
            // (the 24 fragment offsets of a trip are loop-invariant up to the chunk; hoisted they are live registers the loop
            //  does not have.  Opaque copies, refreshed per trip, make the compiler form each where it is used: conv_wide.hip)
            asm volatile("" : "+v"(aoff_o), "+v"(am_o));
#pragma unroll
            for (int u = 0; u < 6; ++u) {
                const int chunk = cp + u / 3, tap = u % 3;
                // the step after this one; past the layer's end: a harmless re-read (every load here is unconditional)
                const bool wrap = (u == 5) && (cp + 2 >= nchunks);
                const int bchunk = wrap ? chunk : cp + (u + 1) / 3;
                const int btap = (u == 5) ? (wrap ? tap : 0) : (u + 1) % 3;
                CHAIN_LOAD_B((u + 1) & 1, bchunk, btap)
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    if (rt + 1 < 4) { CHAIN_LOAD_A((rt + 1) & 1, chunk, tap, rt + 1) }
                    else if (u < 5) { CHAIN_LOAD_A(0, cp + (u + 1) / 3, (u + 1) % 3, 0) }
                    else { CHAIN_LOAD_A(0, bchunk, 0, 0) }       // (tap 0 of the next pair's first chunk, or -- past the end -- of this one)
                    __builtin_amdgcn_sched_barrier(0);
                    if (!no_mfma) {
                        // hi*lo + lo*hi of the step summed apart and added to the accumulator by ONE fp32 add, ahead of hi*hi:
                        // two roundings at the accumulator's magnitude per step instead of three (the two small products round
                        // at their own magnitude, 2^-11 of it)
                        f32x4 t[NCT];
#pragma unroll
                        for (int c = 0; c < NCT; ++c)
                            t[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[rt & 1][0], fb[u & 1][c][1], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                        for (int c = 0; c < NCT; ++c)
                            t[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[rt & 1][1], fb[u & 1][c][0], t[c], 0, 0, 0);
#pragma unroll
                        for (int c = 0; c < NCT; ++c) {
                            acc[rt][c] += t[c];
                            acc[rt][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[rt & 1][0], fb[u & 1][c][0], acc[rt][c], 0, 0, 0);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
#undef CHAIN_LOAD_A
#undef CHAIN_LOAD_B
    }
    // the next layer's first weight fragments: in flight across the layer boundary
    if (!last) chain_preload(fb, a.layer[li + 1], wave, lane);
    __syncthreads();          // every wave is done reading the slab
    // (the epilogue's addresses depend on the lane alone: formed at kernel start they would be carried through every layer's
    //  MFMA loop, in scratch.  Opaque copies of the lane's coordinates make each layer form them here.)
    int l16e = l16, kge = kg, tide = tid;
    asm volatile("" : "+v"(l16e), "+v"(kge), "+v"(tide));

    // ---- GroupNorm partial sums: fp32 per (wave, 4-row unit), unit = rt 4 + kg ----
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            acc[rt][c] *= DESCALE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = acc[rt][c][j];
                s1 += v;
                s2 += v * v;
            }
        }
        s1 = row16_sum_dpp(s1);
        s2 = row16_sum_dpp(s2);
        if (l16e == 0) {
            spart[(wave * UNITS + rt * 4 + kge) * 2] = s1;
            spart[(wave * UNITS + rt * 4 + kge) * 2 + 1] = s2;
        }
    }
    if (last) {
        // the raw output tile, [ROWS][N + 4] fp32 over the slab
        if (active) {
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int c = 0; c < NCT; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        slab[(rt * 16 + kge * 4 + j) * (N + 4) + (wave * NCT + c) * 16 + l16e] = acc[rt][c][j];
        }
    }
    __syncthreads();
    // ---- per sample: the eight waves' partials of its units in fp64, fixed order ----
    const int HW = 1 << lhw, nsamp = ROWS >> lhw, ups = HW >> 2;
    if (tide < nsamp) {
        double d1 = 0.0, d2 = 0.0;
        for (int w = 0; w < NWAVE; ++w)
            for (int u = 0; u < ups; ++u) {
                d1 += (double)spart[(w * UNITS + tide * ups + u) * 2];
                d2 += (double)spart[(w * UNITS + tide * ups + u) * 2 + 1];
            }
        if (last) {
            const int b = (m0 >> lhw) + tide;
            if (m0 + tide * HW < a.M) {
                double* o = a.stats + (size_t)b * a.slots * 2;
                o[0] = d1;
                o[1] = d2;
            }
        } else {
            const double inv_count = 1.0 / ((double)N * (double)HW);
            const double m = d1 * inv_count;
            double var = d2 * inv_count - m * m;
            if (var < 0.0) var = 0.0;
            smean[tide] = (float)m;
            srstd[tide] = (float)(1.0 / sqrt(var + 1e-5));
        }
    }
    if (last) {
        const int qpr = N >> 2;                   // 16-byte pieces per row
        for (int q = tide; q < ROWS * qpr; q += NTHR) {
            const int row = q / qpr, c4 = q - row * qpr;
            if (m0 + row < a.M)
                *reinterpret_cast<f32x4*>(a.dst + (size_t)(m0 + row) * a.dst_ld + c4 * 4) =
                    *reinterpret_cast<const f32x4*>(slab + row * (N + 4) + c4 * 4);
        }
        return;
    }
    __syncthreads();
    // ---- the next layer's operands: (v - mu) (rs gamma) + beta [-> GELU] -> split, over the input slab ----
    if (active) {
        const ChainLayer& Ln = a.layer[li + 1];
        const bool gelu = Ln.gelu != 0;
        unsigned short* hs = reinterpret_cast<unsigned short*>(slab);
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
            const int n = (wave * NCT + c) * 16 + l16e;
            const float g = Ln.gamma[n], be = Ln.beta[n];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const int row0 = rt * 16 + kge * 4;
                const float mu = smean[row0 >> lhw], sc = srstd[row0 >> lhw] * g;
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = (acc[rt][c][j] - mu) * sc + be;
                    if (gelu) v[j] = gelu_erf(v[j]);
                }
                unsigned h01, l01, h23, l23;
                split_pair_f16(v[0] * ACT_SCALE, v[1] * ACT_SCALE, h01, l01);
                split_pair_f16(v[2] * ACT_SCALE, v[3] * ACT_SCALE, h23, l23);
                unsigned short* rp = hs + (((n >> 5) * ROWS + row0) * LDK) * 2 + (n & 31);      // fp16 hi of row0; lo: + 32
                rp[0] = (unsigned short)h01;            rp[2 * LDK] = (unsigned short)(h01 >> 16);
                rp[4 * LDK] = (unsigned short)h23;      rp[6 * LDK] = (unsigned short)(h23 >> 16);
                rp[32] = (unsigned short)l01;           rp[2 * LDK + 32] = (unsigned short)(l01 >> 16);
                rp[4 * LDK + 32] = (unsigned short)l23; rp[6 * LDK + 32] = (unsigned short)(l23 >> 16);
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(NTHR) void conv_chain_kernel(const ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15;
    const int m0 = blockIdx.x * ROWS;
    const int lhw = __builtin_ctz((unsigned)a.HW);
#ifdef SPDM_DIAG
    const bool no_mfma = (a.debug & DBG_NO_MFMA) != 0;          // ablation (timing only: wrong results)
#else
    constexpr bool no_mfma = false;
#endif
    if (tid < LDK) smem[SLAB + tid] = 0.f;                      // the all-zero row

    f16x8 fb[2][4][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int c = 0; c < 4; ++c) fb[s][c][0] = fb[s][c][1] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    chain_preload(fb, a.layer[0], wave, lane);

    // tap validity of the lane's row in each of the four row tiles: bit 2 rt = dh -1, bit 2 rt + 1 = dh +1
    unsigned am = 0u;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int h = (rt * 16 + l16) & (a.HW - 1);
        am |= (h > 0 ? 1u : 0u) << (2 * rt);
        am |= (h < a.HW - 1 ? 1u : 0u) << (2 * rt + 1);
    }

    // ---- the first layer's input: a finished tensor (no prologue), staged once; rows past M as zeros ----
    {
        const int K0 = a.layer[0].K, qpr = K0 >> 2;
        for (int q = tid; q < ROWS * qpr; q += NTHR) {
            const int row = q / qpr, c4 = q - row * qpr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (m0 + row < a.M) v = *reinterpret_cast<const f32x4*>(a.src + (size_t)(m0 + row) * a.src_ld + c4 * 4);
            const f32x2 p0 = split2(v.x, v.y), p1 = split2(v.z, v.w);
            float* r = smem + ((c4 >> 3) * ROWS + row) * LDK + (c4 & 7) * 2;
            *reinterpret_cast<f32x2*>(r) = f32x2{p0.x, p1.x};           // hi
            *reinterpret_cast<f32x2*>(r + 16) = f32x2{p0.y, p1.y};      // lo
        }
    }
    __syncthreads();

    for (int li = 0; li < a.n_layers; ++li) {
        const int nct = chain_nct(a.layer[li].N);
        if (nct == 4) chain_layer<4>(a, li, smem, fb, am, m0, lhw, no_mfma);
        else if (nct == 2) chain_layer<2>(a, li, smem, fb, am, m0, lhw, no_mfma);
        else chain_layer<1>(a, li, smem, fb, am, m0, lhw, no_mfma);
    }
}

}  // namespace

// Which chains run here (false: not here): split precision, 3-tap layers on a width-1 map whose samples are HW = 4 .. 64 rows
// (a power of two, so a 64-row block holds whole samples), 1 .. CHAIN_MAX_LAYERS layers, every width a multiple of 64 up to 512;
// chan: the n_layers + 1 widths, input first.
bool conv_chain_geometry(int M, int HW, int W, int taps, int split, int n_layers, const int* chan) {
    if (!split || taps != 3 || W != 1 || HW < 4 || HW > ROWS || (HW & (HW - 1)) != 0 || M <= 0 || M % HW != 0) return false;
    if (n_layers < 1 || n_layers > CHAIN_MAX_LAYERS || chan == nullptr) return false;
    for (int i = 0; i <= n_layers; ++i)
        if (chan[i] < 64 || chan[i] > MAXC || chan[i] % 64 != 0) return false;
    return true;
}

int conv_chain_blocks(int M) { return (M + ROWS - 1) / ROWS; }

hipError_t launch_conv_chain(const ChainArgs& a, hipStream_t s) {
    int chan[CHAIN_MAX_LAYERS + 1] = {};
    if (a.n_layers < 1 || a.n_layers > CHAIN_MAX_LAYERS) return hipErrorInvalidValue;
    chan[0] = a.layer[0].K;
    for (int i = 0; i < a.n_layers; ++i) {
        const ChainLayer& L = a.layer[i];
        if (L.K != chan[i] || L.wfrag == nullptr || (i > 0 && (L.gamma == nullptr || L.beta == nullptr))) return hipErrorInvalidValue;
        chan[i + 1] = L.N;
    }
    if (!conv_chain_geometry(a.M, a.HW, 1, 3, 1, a.n_layers, chan)) return hipErrorInvalidValue;
    if (a.src == nullptr || a.dst == nullptr || a.stats == nullptr || a.slots < 1 || a.src_ld < chan[0] || a.src_ld % 4 != 0 ||
        a.dst_ld < chan[a.n_layers] || a.dst_ld % 4 != 0) return hipErrorInvalidValue;
    auto kern = conv_chain_kernel;
    if (hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kern)); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(conv_chain_blocks(a.M)), dim3(NTHR), LDS_FLOATS * sizeof(float), s, a);
    return hipGetLastError();
}

// fp32-equivalent FLOPs of the chain: the sum of its layers' (gemm_flops of each, 3 taps)
double conv_chain_flops(const ChainArgs& a) {
    double f = 0.0;
    for (int i = 0; i < a.n_layers; ++i) f += 2.0 * (double)a.M * a.layer[i].N * a.layer[i].K * 3.0;
    return f;
}

}  // namespace spdm
