// kernels.h -- launch-side declarations of the hand-written gfx950 kernels.
//
// Activation layout everywhere: CHANNELS-LAST  act[b][p][c]  with p = h*W_l + w
// (the reference's NCHW "(B,C,H,W) image", models/Unet_FiLmLayer.py:286, viewed
// as tokens x channels -- which is also the (B,L,C) view its attention blocks
// take at :74).  A 3x3 convolution is then an implicit GEMM
//     out[m][n] = sum_{tap,ci} in[m + shift(tap)][ci] * w[tap][n][ci],   m = b*HW + p
// and a Linear layer is the same GEMM with one tap.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace spdm {

// Kernels that declare more than 64 KiB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize, a PER-DEVICE
// function attribute: set it once per (device, kernel) -- a process may hold handles on several GPUs.
inline hipError_t allow_full_lds(const void* kern) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({dev, kern})) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024));
    if (e == hipSuccess) done.insert({dev, kern});
    return e;
}

// GroupNorm(1,C) statistics are produced by the kernel that writes a tensor, as
// per-(sample, tile) partial sums in fp64:  stats[(b*slots + slot)*2 + {0,1}] =
// {sum x, sum x^2}.  Slot of the partial that tile (mt, nt) contributes to
// sample b:  (mt - (b*HW)/m_tile) * n_tiles + nt.  Consumers add the valid
// slots in a fixed order, so results are run-to-run deterministic.
struct StatsRef {
    const double* p;     // nullptr: no normalisation
    int slots;           // slots per sample
    int m_tile;          // rows per producer tile
    int n_tiles;         // producer tiles along channels
    int HW;              // rows per sample of the normalised tensor
    double inv_count;    // 1 / (C * HW)
};

__host__ __device__ inline int stats_slots(int HW, int m_tile, int n_tiles) {
    return ((HW + m_tile - 2) / m_tile + 1) * n_tiles;
}

// Kernel-selection switches.  Read from the environment ONCE (spdm_create / spdm_bench_gemm: switches_from_env) and
// carried in the handle; every launch decision and the step-graph key derive from this one word, so a mid-session
// change of the environment cannot change which kernels run.  spdm_set_switch flips one on a live handle (tests).
enum : unsigned {
    SW_NO_WIDE = 1u << 0, SW_NO_WIDE128 = 1u << 1, SW_NO_W2 = 1u << 2, SW_NO_T512 = 1u << 3, SW_T512 = 1u << 4,
    SW_T3_BIG = 1u << 5, SW_NO_SMALL_TPI3 = 1u << 6, SW_WIDE_N64_2X2 = 1u << 7, SW_NO_SA_FUSED = 1u << 8,
    SW_NO_SA_TAIL = 1u << 9, SW_ATTN_VALU = 1u << 10, SW_SA_NO_WLDS = 1u << 11, SW_NO_FILM_FOLD = 1u << 12,
    SW_NO_GRAPH = 1u << 13, SW_NO_SPLITK = 1u << 14, SW_ARENA_TRACE = 1u << 15, SW_NO_WIDE_PIPE = 1u << 16, SW_NO_SKINNY = 1u << 17, SW_DEEP = 1u << 18,
    SW_NO_FILM_LOCAL = 1u << 19, SW_NO_FUSED_SRC = 1u << 20, SW_FILM_LOCAL = 1u << 21, SW_PIN_GEOMETRY = 1u << 22, SW_NO_WP4 = 1u << 23, SW_G2 = 1u << 24, SW_NO_WP8 = 1u << 25, SW_NO_SA_HEAD = 1u << 26, SW_SA_HEAD = 1u << 27, SW_NO_REG64 = 1u << 28,
    SW_NO_SA_CROP = 1u << 29, SW_NO_SA_OUTC = 1u << 30, SW_NO_WHOLE_TILES = 1u << 31,
};
struct SwitchName { const char* env; unsigned bit; };
inline const SwitchName* switch_table(int* n) {
    static const SwitchName t[] = {
        {"SPDM_NO_WIDE", SW_NO_WIDE}, {"SPDM_NO_WIDE128", SW_NO_WIDE128}, {"SPDM_NO_W2", SW_NO_W2}, {"SPDM_NO_T512", SW_NO_T512},
        {"SPDM_T512", SW_T512}, {"SPDM_T3_BIG", SW_T3_BIG}, {"SPDM_NO_SMALL_TPI3", SW_NO_SMALL_TPI3},
        {"SPDM_WIDE_N64_2X2", SW_WIDE_N64_2X2}, {"SPDM_NO_SA_FUSED", SW_NO_SA_FUSED}, {"SPDM_NO_SA_TAIL", SW_NO_SA_TAIL},
        {"SPDM_ATTN_VALU", SW_ATTN_VALU}, {"SPDM_SA_NO_WLDS", SW_SA_NO_WLDS}, {"SPDM_NO_FILM_FOLD", SW_NO_FILM_FOLD},
        {"SPDM_NO_GRAPH", SW_NO_GRAPH}, {"SPDM_NO_SPLITK", SW_NO_SPLITK}, {"SPDM_ARENA_TRACE", SW_ARENA_TRACE}, {"SPDM_NO_WIDE_PIPE", SW_NO_WIDE_PIPE}, {"SPDM_NO_SKINNY", SW_NO_SKINNY}, {"SPDM_DEEP", SW_DEEP},
        {"SPDM_NO_FILM_LOCAL", SW_NO_FILM_LOCAL}, {"SPDM_NO_FUSED_SRC", SW_NO_FUSED_SRC},
        {"SPDM_FILM_LOCAL", SW_FILM_LOCAL}, {"SPDM_PIN_GEOMETRY", SW_PIN_GEOMETRY},
        {"SPDM_NO_WP4", SW_NO_WP4}, {"SPDM_G2", SW_G2}, {"SPDM_NO_WP8", SW_NO_WP8},
        {"SPDM_NO_SA_HEAD", SW_NO_SA_HEAD}, {"SPDM_SA_HEAD", SW_SA_HEAD}, {"SPDM_NO_REG64", SW_NO_REG64},
        {"SPDM_NO_SA_CROP", SW_NO_SA_CROP}, {"SPDM_NO_SA_OUTC", SW_NO_SA_OUTC}, {"SPDM_NO_WHOLE_TILES", SW_NO_WHOLE_TILES}};
    *n = (int)(sizeof(t) / sizeof(t[0]));
    return t;
}
unsigned switches_from_env();          // spdm_api.hip
int spdm_tune(int idx, int dflt);      // conv_gemm.hip: SPDM_TUNE<idx> (read once per process) or dflt -- tuning experiments only

// Load prologue of a convolution.  PRO_POOL / PRO_UPCAT: the FIRST convolution of a Down / UpSample block reads the block's input
// through the resampling op itself (GemmArgs: "fused sources") instead of a materialised pooled / concatenated tensor.
// PRO_GN_POOLED (conv_reg.hip on width-4 maps, plan only): src is the RAW MaxPool2d(2) map a producer's epilogue wrote
// (GemmArgs::pool_dst) and pro_* the FINER level's pending GroupNorm, applied in pool_kernel's arithmetic (resample.h affine1).
enum { PRO_NONE = 0, PRO_GN = 1, PRO_GN_GELU = 2, PRO_POOL = 3, PRO_UPCAT = 4, PRO_GN_POOLED = 5 };
enum { EPI_STATS = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_BIAS_RESID = 3, EPI_PLAIN = 4 };

// The kernel configuration a launch dispatched, recorded by the launch itself when GemmArgs::route is set (spdm_op_gemm).
enum { ROUTE_GEMM = 0, ROUTE_SKINNY = 1, ROUTE_REG = 2, ROUTE_WIDE = 3 };
// variant: 0 plain; 1 width-2 zero-tap skipping; 2 / 3 width-4 / width-8 row classes (conv_wide); 4 pipelined slab hand-over
// (conv_wide); 5 two chunks per hand-over (conv_wide, SPDM_G2)
enum { VAR_PLAIN = 0, VAR_W2 = 1, VAR_WP4 = 2, VAR_WP8 = 3, VAR_PIPE = 4, VAR_G2 = 5 };
struct GemmRoute { int kernel, variant, m_tile, n_tile, whole; };      // whole: conv_wide's staging (0 halo'd slab, 1 whole-sample tiles, 2 one sample per tile)

struct GemmArgs {
    const float* src;  int src_ld;     // [M][src_ld], K valid channels
    const float* wgt;                  // [taps][N][K]  (k contiguous); split: per 32-k chunk [32 fp16 hi | 32 fp16 lo]
    int split;                         // 0: fp32 MFMA (exact); 1: split-fp16 MFMA (wgt in the split format)
    const float* wgt_frag;             // optional: fragment-order copy of the split weights (WL_FRAG, weight_layout.hip) -> conv_wide.hip
    float* dst;        int dst_ld;
    int M, K, N;
    int geom_M;                        // > 0: choose tiles / split-K / kernel as for THIS many rows (SW_PIN_GEOMETRY: a shard of a larger batch
                                       // then runs exactly the kernels the whole batch would, and reproduces it bit for bit)
    int taps;                          // 1, 3 (vertical taps, W == 1) or 9
    int H, W, HW;                      // spatial dims of this level
    int pro;  StatsRef pro_stats;  const float* pro_gamma;  const float* pro_beta;
    // Fused sources (gemm_takes_fused_source says which launches: conv_skinny.hip takes both modes on its small grids,
    // conv_wide.hip PRO_UPCAT on whole-sample two-source tiles at large batch; PRO_POOL at large batch is refused):
    //   PRO_POOL : the conv input is MaxPool2d(2) (models/Unet_FiLmLayer.py:132,159) of src, src being the FINER level's tensor
    //              [B][4 HW][K] -- a (2 H) x (2 W) map per sample -- with its pending GroupNorm in pro_stats / pro_gamma / pro_beta
    //              (pro_stats.p == nullptr: none; the affine is applied per tap: max does not commute with a negative gain);
    //   PRO_UPCAT: torch.cat([Upsample(x2, bilinear, align_corners=True)(x), x_res], dim=1) (:191,217-218): input channels
    //              [0, up_C) are the upsample of src, the COARSER level's tensor [B][HW / 4][up_C] (pending GroupNorm in pro_*),
    //              channels [up_C, K) are skip [B][HW][K - up_C] (pending GroupNorm in skip_*; skip_stats.p == nullptr: none).
    int up_C;  const float* skip;  int skip_ld;  StatsRef skip_stats;  const float* skip_gamma;  const float* skip_beta;
    int epi;  double* epi_stats;   const float* bias;  const float* resid;  int resid_ld;
    // Pooled epilogue (conv_reg.hip, width-8 maps; null everywhere but the plan's inc.second): the launch also writes
    // MaxPool2d(2) of dst as a RAW map [B][HW / 4][pool_ld] -- per channel the max of a window's raw values where pool_gamma, the
    // gain of the GroupNorm pending on dst, is >= 0, and the min where it is < 0 -- for a PRO_GN_POOLED consumer.
    float* pool_dst;  int pool_ld;  const float* pool_gamma;
    double* row_stats;                 // optional: per-row {sum, sum^2} of the STORED values, [row][n_tiles][2] (LayerNorm of the consumer)
    // Split-K (small grids: few rows, long K).  ksplit > 1: the launch has ksplit x as many workgroups; workgroup (tile, ks)
    // walks the 32-channel chunks [ks nchunks / ksplit, (ks + 1) nchunks / ksplit) of every tap and stores its raw fp32
    // partial tile to partial[ks][M][N]; no statistics, no dst.  launch_splitk_combine then adds the slabs in the fixed
    // order ks = 0, 1, ... (deterministic: no atomics), writes dst and the GroupNorm partial sums.
    int ksplit;  float* partial;
    unsigned sw;                       // kernel-selection switches (SW_*) of the owning handle
    int debug;                         // ablation knobs for spdm_bench_gemm only (0 in the product path)
    unsigned long long* stamps;        // DBG_STAMP: [2][128] s_memtime stamps of one workgroup (diagnostic builds of the bench)
    GemmRoute* route;                  // optional (host): the launch records the configuration it dispatched (spdm_op_gemm; null in the plan)
};
enum { DBG_NO_MFMA = 1, DBG_NO_WLOAD = 2, DBG_NO_GELU = 4, DBG_NO_STORE = 8, DBG_NO_ALOAD = 16, DBG_PP = 64, DBG_STAMP = 128 };

// geometry of the stats the GEMM writes (EPI_STATS)
struct GemmGeom {
    int m_tile, n_tile, n_tiles;     // output tile of the GEMM kernel
    int slots;                       // statistics slots per sample of whoever writes them
    int ksplit;                      // > 1: split-K launch + combine
    int skinny;                      // 1: conv_skinny.hip (a handful of rows: whole-K slab in LDS, the waves of a workgroup split K)
    int reg;                         // 1: conv_reg.hip (64 -> 64 channels on the width-8 level: activations in registers, weights in LDS)
    int st_m_tile, st_n_tiles;       // StatsRef geometry of the statistics (the GEMM's own tiling, or the combine kernel's)
};
// K = input channels (per tap); ksplit is only ever > 1 for split-precision 3x3 / 3x1 convolutions with the statistics
// epilogue (the callers that pass stats_epi = true)
GemmGeom gemm_geometry(int M, int N, int K, int HW, int W, int taps, int split, unsigned sw, bool stats_epi = false);
// ... of a launch, as launch_gemm chooses it: rows as geom_M says, split-K only with the statistics epilogue and a partial buffer
GemmGeom gemm_geometry(const GemmArgs& a);
constexpr size_t SPLITK_WORKSPACE_BYTES = (size_t)48 << 20;     // partial slabs of one launch (handle-owned buffer)
// rows of one sample a combine workgroup owns (a power-of-two fraction of HW; <= 2048 values = two 16-byte pieces per thread
// where HW allows: at batch 1 the combine is a handful of workgroups, so each must be short)
__host__ __device__ inline int combine_rows(int HW, int N) {
    int r = HW;
    while ((r & 1) == 0 && (long long)r * N > 2048) r >>= 1;
    return r;
}
// dst[m][n] = sum_ks partial[ks][m][n] (ks ascending) + GroupNorm partial sums in the layout StatsRef{slots = HW / rows + 1,
// m_tile = rows, n_tiles = 1} with rows = combine_rows(HW, N)
// conv_skinny.hip: 3x3 / 3x1 convolutions of <= 256 rows (batch 1-4).  conv_skinny_geometry is the shape rule (false: not here)
bool conv_skinny_geometry(int M, int N, int K, int HW, int W, int taps, int split, unsigned sw, int* m_tile, int* n_tile);
hipError_t launch_conv_skinny(const GemmArgs& a, const GemmGeom& g, hipStream_t s);
// conv_reg.hip: 3x3 convolutions 64 -> 64 on width-8 maps at large batch (64-row wave tiles; one statistics slot per wave tile)
bool conv_reg_geometry(int M, int N, int K, int HW, int W, int taps, int split, unsigned sw);
hipError_t launch_conv_reg64(const GemmArgs& a, const GemmGeom& g, hipStream_t s);
// PRO_GN_POOLED sums the finer tensor's statistics slots serially (sample_mean_rstd); pool_kernel does so for whole-tile samples
// of up to 8 slots (sample_mean_rstd_wave), and only then are the two means bit-identical
inline bool pooled_stats_serial(const StatsRef& st) {
    return st.m_tile > 0 && st.HW % st.m_tile == 0 && (st.HW / st.m_tile) * st.n_tiles <= 8;
}
hipError_t launch_splitk_combine(const float* partial, int ksplit, float* dst, int M, int N, int HW, double* stats,
                                 hipStream_t s);
hipError_t launch_gemm(const GemmArgs& a, hipStream_t s);
// would launch_gemm run this statistics-epilogue convolution on a kernel that takes a fused source (pro = PRO_POOL / PRO_UPCAT)?
// (a: the complete launch arguments, as launch_gemm would get them)
bool gemm_takes_fused_source(const GemmArgs& a);
// ... or a two-source input (pro = PRO_NONE / PRO_GN with `skip` set: channels [0, up_C) from src, [up_C, K) from skip, the
// prologue applying to the skip part only)?  conv_wide.hip's 128-wide configurations.
bool gemm_takes_two_sources(const GemmArgs& a);
double gemm_flops(const GemmArgs& a);
// conv_wide.hip: the 4-wave / 128x64-per-wave configuration of the 3x3 implicit GEMM (256 x 128 tiles, two
// workgroups per CU); launch_gemm routes to it when conv_wide_supported
bool conv_wide_supported(const GemmArgs& a, const GemmGeom& g);
// ... and takes pro = PRO_UPCAT itself (the upsample formed in its slab loader) when the launch is a whole-sample two-source
// tile of 256 rows on a width-8 / 4 / 2 map; a (ksplit as launch_gemm sets it) and the geometry launch_gemm chose
bool conv_wide_takes_upcat(const GemmArgs& a, const GemmGeom& g);
int gemm_wide_upcat_launches();        // conv_gemm.hip: how many launches of this process launch_gemm sent that way (host-side count)
hipError_t launch_conv_wide(const GemmArgs& a, const GemmGeom& g, hipStream_t s);

// conv_chain.hip: a list of 3-tap convolutions of a width-1 map (split precision) run end to end by one 8-wave workgroup per
// 64-row block, the GroupNorm [-> GELU] between two layers applied in LDS.  Layer i reads K channels and writes N; gamma / beta /
// gelu describe the GroupNorm pending on the layer's INPUT (layer 0 reads a finished tensor: they are unused there).
constexpr int CHAIN_MAX_LAYERS = 8;
struct ChainLayer {
    const float* wfrag;                // WL_FRAG copy of the [3][N][K] split weights (weight_layout.hip)
    const float* gamma;  const float* beta;
    int K, N, gelu;
};
struct ChainArgs {
    const float* src;  int src_ld;     // [M][src_ld], finished
    float* dst;        int dst_ld;     // raw output of the last layer
    double* stats;     int slots;      // its GroupNorm partials, [sample][slots][2]: slot 0 written (StatsRef{m_tile = 64, n_tiles = 1})
    int M, HW;                         // rows; rows per sample
    int n_layers;
    int debug;                         // DBG_NO_MFMA (diagnostic builds only; 0 in the product path)
    ChainLayer layer[CHAIN_MAX_LAYERS];
};
constexpr int CHAIN_M_TILE = 64;
// the shape rule (false: not here); chan: the n_layers + 1 widths, input first
bool conv_chain_geometry(int M, int HW, int W, int taps, int split, int n_layers, const int* chan);
int conv_chain_blocks(int M);
double conv_chain_flops(const ChainArgs& a);       // the sum of gemm_flops of its layers
hipError_t launch_conv_chain(const ChainArgs& a, hipStream_t s);

// ---- streaming / small kernels (elementwise.hip) -------------------------------------------
// first conv, Cin = 1, fused zero-padding of the (H0, D) trajectory to (Hp, Wp)
// ... and, as the first kernel of a denoise step, the loop bookkeeping (adv: -2 none, -1 advance by one, >= 0 set the step)
int conv_in_parts(int Hp, int Wp, int B);        // row parts per sample = statistics slots it writes (m_tile = HW / parts)
hipError_t launch_conv_in(const float* x, const float* w /*[9][64]*/, float* dst, double* stats,
                          int B, int H0, int D, int Hp, int Wp, int lh, int lw, int* step_dev, int* t_dev,
                          const int* timesteps_dev, int n_steps, int adv, hipStream_t s, int B_geom = 0);     // B_geom > 0: row parts as for that batch

struct AffineSrc {               // a tensor + the per-(sample,channel) affine that finishes it
    const float* x; int C;       // channels-last [B][HW][C]
    StatsRef st; const float* gamma; const float* beta;   // GroupNorm part (st.p may be null)
};
// MaxPool2d(2) of affine(src):  (B, H*W, C) -> (B, H/2*W/2, C)
hipError_t launch_pool(const AffineSrc& src, float* dst, int B, int H, int W, hipStream_t s);
// cat([bilinear_x2_align_corners(affine(up)), affine(skip)], channel)
hipError_t launch_upcat(const AffineSrc& up, const AffineSrc& skip, float* dst, int B, int Hin, int Win,
                        hipStream_t s);
// block tail: y = scale * (GN(x) + temb[t]) + bias   (FiLM; film == nullptr: y = GN(x) + temb)
// row_stats (optional): per-token {sum, sum^2} over C of y as fp64 -- the LayerNorm statistics the
// attention block's first GEMM applies in its load prologue
hipError_t launch_film_apply(const AffineSrc& src, const float* temb_table /*[T][C]*/, const int* t_dev,
                             int t_count, const float* film /*[B][2C] or null*/, float* dst, double* row_stats,
                             int B, int HW, hipStream_t s);
// The same tail as a recipe: the attention kernels that read the block input themselves (sa_qkv / sa_tail / sa_fused64) evaluate
// the coefficients of the samples their tile touches at kernel start (device_utils.h film_coef_row_wave: statistics slots, one
// time-embedding row, the FiLM row) instead of reading them from a film_coef_kernel launch -- one launch per block less, which is
// what a small-batch step is made of (64 launches of ~5-8 us at batch 1).
struct FilmSpec {
    StatsRef st; const float* gamma; const float* beta;   // GroupNorm(1,C) still pending on the raw tensor (st.p may be null)
    const float* temb; const int* t_dev; int t_count;     // time-embedding table [T][C] and the device timestep(s); temb may be null
    const float* film;                                    // [B][2C] = [scale | bias] of the FiLM encoder, or null
    int C;
    int on;                                               // 0: unused (the consumer takes `ab` from memory, or nothing)
};
// the same tail as per-(sample, channel) coefficients ab[b] = [A (C) | B (C)], y = A x + B, for consumers that apply it on load
hipError_t launch_film_coef(const AffineSrc& src, const float* temb_table, const int* t_dev, int t_count, const float* film,
                            float* ab, int B, hipStream_t s);
// encoder.hip: the three stride-2 2x2 convolutions (+ReLU) of the observation autoencoder's encoder
// (models/encoder/autoencoder.py:11-17), (n,3,96,96) -> flattened (n, 64*12*12) rows for its Linear layer
hipError_t launch_encoder_convs(const float* img, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* w3, const float* b3, float* feat, int n_images, hipStream_t s);
// encoder_train.hip: the encoder's training pass (spdm_encoder_train_forward / spdm_encoder_backward).
// Row layouts: x3 [n*144][128] = conv 2's map as conv 3's space-to-depth rows (k = ci*4 + ky*2 + kx); x2 [n*576][64] = conv 1's
// map as conv 2's rows, row (n*144 + q)*4 + kk = the conv-2 position kk of conv-3 window q.
// the forward's convolutions, bit for bit launch_encoder_convs, which also keep x3
hipError_t launch_encoder_train_convs(const float* img, const float* w1, const float* b1, const float* w2, const float* b2,
                                      const float* w3, const float* b3, float* feat, float* x3, int n_images, hipStream_t s);
// the three pre-activations again in float64; a saved value (feat, x3) on the other side of its ReLU kink is rewritten so that
// "saved > 0" is the exact network's mask (run after the Linear layer has read feat)
hipError_t launch_encoder_kinks(const float* img, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* w3, const float* b3, float* feat, float* x3, int n_images, hipStream_t s);
// x2 recomputed from the frames
hipError_t launch_encoder_x2(const float* img, const float* w1, const float* b1, int n_images, float* x2, hipStream_t s);
// dz3 [n*144][64] = dfeat (Flatten order) under feat's ReLU mask; dz2 [n*576][32] = dx3 under x3's
hipError_t launch_encoder_dz3(const float* dfeat, const float* feat, int n_images, float* dz3, hipStream_t s);
hipError_t launch_encoder_dz2(const float* dx3, const float* x3, int n_images, float* dz2, hipStream_t s);
// conv 1's weight (16,3,2,2) and bias gradient from dx2 under x2's ReLU mask; part: [encoder_conv1_wgrad_blocks(n)][208]
int encoder_conv1_wgrad_blocks(int n_images);
hipError_t launch_encoder_conv1_wgrad(const float* img, const float* dx2, const float* x2, int n_images, float* part,
                                      float* dw, float* db, hipStream_t s);
hipError_t launch_add(const float* src, size_t n, float* dst, hipStream_t s);               // dst += src
// decoder.hip: the autoencoder's decoder (models/encoder/autoencoder.py:23-32) and its reconstruction training.
// Row layouts, channels-last: h0 [n*144][64] (the Linear's output, column q*64 + c of its [n][9216] rows), a1 [n*576][32] with row
// (n*144 + q)*4 + kk1, a2 [n*2304][16] with row r2*4 + kk2; weights w2 [64][4][32], w4 [32][4][16], w6 [16][4][3] = [ci][kk][co].
// the three transposed convolutions + ReLU / sigmoid of n frames -> recon (n,3,96,96)
hipError_t launch_decoder_convs(const float* h0, const float* w2, const float* b2, const float* w4, const float* b4,
                                const float* w6, const float* b6, float* recon, int n_frames, hipStream_t s);
// ... bit for bit the same reconstruction, which also keeps a1, a2 and sq[frame] = sum (recon - target)^2
hipError_t launch_decoder_train_convs(const float* h0, const float* w2, const float* b2, const float* w4, const float* b4,
                                      const float* w6, const float* b6, float* recon, const float* target, float* a1, float* a2,
                                      double* sq, int n_frames, hipStream_t s);
// the Linear and the two ReLU layers again in float64 from the latents (w0 / b0: the Linear in its kernel layout, rows q*64 + c);
// a saved value (a1, a2) on the other side of its ReLU kink is rewritten so that "saved > 0" is the exact network's mask
hipError_t launch_decoder_kinks(const float* latent, const float* w0, const float* b0, const float* w2, const float* b2,
                                const float* w4, const float* b4, float* a1, float* a2, int n_frames, hipStream_t s);
// loss = sum_frames sq / (n 27648), fixed order
hipError_t launch_decoder_loss(const double* sq, int n_frames, float* loss, hipStream_t s);
// layer 6 backwards: dw (16,3,2,2) and db (3) of these frames, dz4 [n*576][64] (column kk2*16 + co) under a2's ReLU mask;
// scale = 2 / (N 27648) with N the frames of the whole loss; part: [n_frames][208]
hipError_t launch_decoder_bwd6(const float* recon, const float* target, const float* a2, const float* w6, float scale,
                               int n_frames, float* dz4, float* part, float* dw, float* db, hipStream_t s);
// dz2 [n*576][32] = dz4 w4^T under a1's ReLU mask
hipError_t launch_decoder_dgrad4(const float* dz4, const float* a1, const float* w4, int n_frames, float* dz2, hipStream_t s);
// two-level column sum of src [M][C] (C % 64 == 0); fold 4: dst[co] = sum_kk column kk*n_out + co (n_out = C / 4); fold 1: the
// Linear's 9216 columns q*64 + c back to Flatten order c*144 + q.  part: [decoder_colsum_slabs(M)][C]
int decoder_colsum_slab_rows(long long M);
int decoder_colsum_slabs(long long M);
hipError_t launch_decoder_colsum(const float* src, int C, long long M, int n_out, int fold, float* part, float* dst, hipStream_t s);
// weight gradients back in torch layout: [cin][kk*cout + co] -> (cin, cout, 2, 2); [q*64 + c][128] -> (9216, 128)
hipError_t launch_decoder_unperm_conv(const float* src, int cin, int cout, float* dst, hipStream_t s);
hipError_t launch_decoder_unperm_linear(const float* src, float* dst, hipStream_t s);
// plain GN apply (materialise): y = GN(x)
hipError_t launch_gn_apply(const AffineSrc& src, float* dst, int B, int HW, hipStream_t s);
hipError_t launch_layernorm(const float* x, const float* g, const float* b, float* y, int rows, int C,
                            hipStream_t s);
hipError_t launch_mish_pad(const float* cond, float* dst, int B, int cond_dim, int Kp, hipStream_t s);
hipError_t launch_silu(const float* x, float* y, size_t n, hipStream_t s);
hipError_t launch_gelu(const float* x, float* y, size_t n, hipStream_t s);
// the concat-conditioned U-Net (models/simple_Unet.py; channel-padded storage)
hipError_t launch_silu_pad(const float* cond, float* dst, int B, int cond_dim, int Kp, hipStream_t s);
// y = GELU(GN(x) + res) (res null: GELU(GN(x))), (B, HW, C) -> same
hipError_t launch_dc_finish(const AffineSrc& src, const float* res, float* dst, int B, int HW, hipStream_t s);
// block tail: y[:, :Cr] = GELU(GN(x)) + temb[t][c], y[:, Cr:Cr+32] = cemb[b], zeros up to Co
hipError_t launch_simple_tail(const AffineSrc& src, int Cr, const float* temb, int temb_ld, const int* t_dev, int t_count,
                              const float* cemb, int cemb_ld, float* dst, int Co, int B, int HW, hipStream_t s);

struct StepArgs {
    const float* feat;            // (B, Hp*Wp, 64) channels-last
    const float* w; float bias;   // outc 1x1 conv
    float* x;                     // (B, H0, D) current iterate, updated in place
    float* eps_out;               // non-null: only write eps (spdm_unet_forward)
    const float* eps_in;          // non-null: eps [B][H0][D] already computed (sa6's epilogue, SaCrop::eps); feat, w, bias unused
    const float* coef;            // device [n_steps][6]
    const int* step_dev;          // device scalar: loop iteration
    int kind;
    const float* noise;           // (n_steps, B, H0, D) or null
    const unsigned long long* rng_dev;   // device {seed, first global trajectory index} of the Philox noise stream
    int* flag_dev;                // device word, set to 1 when an updated iterate (or eps) is not finite
    const float* inpaint; int inp_h; int inpaint_per_sample;
    float* history;               // (n_steps+1, B, H0, D) or null
    // Sampling loop: the three caller-owned buffers above are read from this device block {inpaint, noise, history} instead
    // (written by spdm_sample_begin), so the launch arguments -- and with them the captured step graph -- do not depend on
    // where a caller's tensors happen to live.  Null: the fields above are used as given (spdm_unet_forward).
    const void* const* ptrs_dev;
    int B, H0, D, Hp, Wp, lh, lw;
};
hipError_t launch_out_step(const StepArgs& a, hipStream_t s);

// the DPM-Solver++ (2M) update on a ready eps (elementwise.hip solver_step_kernel; spdm_solver_step and the SPDM_DPMPP_2M loop)
struct SolverStepArgs {
    const float* eps;             // (B, H0, D)
    float* x;                     // (B, H0, D) current iterate, updated in place
    float* x0_prev;               // (B, H0, D) the previous step's predicted x0: read on second-order steps, always written
    const float* coef;            // device [n_steps][6] = {sigma_s, alpha_s, k_x, k0f, k0, k1}
    const int* step_dev;          // device scalar: loop iteration
    const int* first_dev;         // device scalar: the iteration that runs first order whatever its row says (-1: none)
    int* flag_dev;                // as StepArgs
    const float* inpaint; int inp_h; int inpaint_per_sample;
    float* history;
    const void* const* ptrs_dev;  // as StepArgs ({inpaint, noise, history}; the noise entry is not read)
    int B, H0, D;
};
hipError_t launch_solver_step(const SolverStepArgs& a, hipStream_t s);

// train.hip: the training-loss gradient of UNet_Film_noAttention (spdm_train_loss_grad).  Channels-last [B][HW][C] throughout.
// weight gradient of a 3x3 (taps 9), 3x1 (taps 3, W == 1) or 1x1 / Linear (taps 1) layer: dst = sum_m dy[m][co] x[shift(m)][ci]
// on fp32 MFMA, rows split into partial slabs (budget_floats of `partial`) added in a fixed order; conv9: (Co, Ci, 3, 3) torch
// layout (taps 3: side columns exact zeros), else (Co, Ci)
int wgrad_chunks(long long M, int taps, int Co, int Ci, size_t budget_floats);
hipError_t launch_wgrad(const float* dy, int ldy, const float* x, int ldx, long long M, int H, int W, int taps, int Co, int Ci,
                        int conv9, float* partial, size_t budget_floats, float* dst, hipStream_t s);
// the same for a channel-padded layer (models/simple_Unet.py, taps 9 or 3): dy [M][Co], x [M][Ci] at storage widths, dst the
// (no, ni, 3, 3) torch tensor of the real channels, gathered through the device maps pos_o[no] / pos_i[ni]
hipError_t launch_wgrad_mapped(const float* dy, const float* x, long long M, int H, int W, int taps, int Co, int Ci,
                               const int* pos_o, int no, const int* pos_i, int ni, float* partial, size_t budget_floats, float* dst,
                               hipStream_t s);
hipError_t launch_colsum(const float* src, int ld, long long M, int C, float* dst, hipStream_t s);
hipError_t launch_gn_stats(const float* y, int B, int n, float* mean, float* rstd, hipStream_t s);
// ... statistics over cnt of the n values per sample (channel-padded storage: HW * C_real, the padded lanes hold zeros)
hipError_t launch_gn_stats_real(const float* y, int B, int n, int cnt, float* mean, float* rstd, hipStream_t s);
hipError_t launch_gn_act(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta, int B,
                         int HW, int C, int gelu, float* out, hipStream_t s);
hipError_t launch_gn_bwd(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* g, int gelu, int B, int HW, int C, float* dy, float* dgb, hipStream_t s);
hipError_t launch_gn_param(const float* p0, const float* p1, int B, int C, float* dgamma, float* dbeta, hipStream_t s);
hipError_t launch_film_bwd(const float* z, const float* temb, const int* t_dev, int t_count, const float* film,
                           const float* dout, int B, int HW, int C, float* dz, float* de, float* dfilm, hipStream_t s);
hipError_t launch_gather_rows(const float* table, const int* t_dev, int t_count, int B, int n, float* out, hipStream_t s);
hipError_t launch_pad(const float* x, int B, int H0, int D, int Hp, int Wp, int lh, int lw, float* xp, hipStream_t s);
hipError_t launch_conv_in_plain(const float* xp, const float* w /*[9][64]*/, int B, int H, int W, float* out, hipStream_t s);
hipError_t launch_outc(const float* u, const float* w, float bias, long long M, float* out, hipStream_t s);
hipError_t launch_outc_bwd(const float* deps, const float* w, long long M, float* du, hipStream_t s);
hipError_t launch_mse(const float* eps_pad, const float* noise, int B, int H0, int D, int Hp, int Wp, int lh, int lw,
                      float* loss, float* deps_pad, float* eps_out, hipStream_t s);
hipError_t launch_pool_bwd(const float* in, const float* dout, int B, int H, int W, int C, float* din, hipStream_t s);
hipError_t launch_up_bwd(const float* dcat, int ld, int B, int h, int w, int C, float* dx, hipStream_t s);
hipError_t launch_add_cols(const float* src, int ld, int c0, long long M, int C, float* dst, hipStream_t s);
hipError_t launch_mish_bwd(const float* dm, int nblk, int B, int ld, const float* cond, int cond_dim, float* grad_cond,
                           hipStream_t s);

// train_attn.hip: the SelfAttention blocks of the training pass (SPDM_FLAG_TRAIN_ATTENTION), exact fp32.  Rows are tokens, [rows][C].
// LayerNorm(C), C in {64, 128, 256}: y, and the per-row mean and 1 / std the backward pass reads
hipError_t launch_ln_fwd(const float* x, const float* g, const float* b, long long rows, int C, float* y, float* mean, float* rstd,
                         hipStream_t s);
// dx = LayerNorm backward of gy (+ add, may be null); part [ln_bwd_blocks(rows)][2C]: per-workgroup [d gamma | d beta] partials
constexpr int LN_BWD_ROWS = 64;
int ln_bwd_blocks(long long rows);
hipError_t launch_ln_bwd(const float* x, const float* mean, const float* rstd, const float* gamma, const float* gy,
                         const float* add, long long rows, int C, float* dx, float* part, hipStream_t s);
hipError_t launch_gelu_bwd(const float* u, const float* dh, size_t n, float* du, hipStream_t s);

// train_simple.hip: the training pass of models/simple_Unet.py (SPDM_FLAG_TRAIN_SIMPLE) in channel-padded storage; a channel map
// is its device array pos[nreal] (storage lane of each real channel), C the storage width (multiple of 64, <= 512)
hipError_t launch_gn_bwd_mapped(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                const float* g, int gelu, int B, int HW, int C, const int* pos, int nreal, float* dy, float* dgb,
                                hipStream_t s);
hipError_t launch_gn_param_mapped(const float* p0, const float* p1, int B, int C, const int* pos, int nreal, float* dgamma,
                                  float* dbeta, hipStream_t s);
// pre = GN(y) + res, out = GELU(pre) (the end of a residual DoubleConvolution)
hipError_t launch_gn_res(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         const float* res, int B, int HW, int C, float* pre, float* out, hipStream_t s);
// block tail: out[:, :Cr] = GELU(GN(y)) + temb[b], out[:, Cr:Cr+32] = cemb[b], zeros up to Co; and its backward
hipError_t launch_simple_tail_fwd(const float* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                  int Cz, int Cr, const float* temb, int temb_ld, const float* cemb, int cemb_ld, int B, int HW,
                                  int Co, float* out, hipStream_t s);
hipError_t launch_simple_tail_bwd(const float* dout, int B, int HW, int Co, int Cr, int Cz, float* dz, float* dtemb, float* dcemb,
                                  int cemb_ld, hipStream_t s);
// out[b] = SiLU(pe[t_b] * scale[b]) (PositionalEncoding's dropout as a per-sample multiplier)
hipError_t launch_time_rows_scaled(const float* pe, const int* t_dev, int t_count, const float* scale, int B, int n, float* out,
                                   hipStream_t s);
hipError_t launch_silu_bwd(const float* ds, int ld, const float* cond, int B, int cond_dim, float* grad_cond, hipStream_t s);
// attention core with its log-sum-exp (lse [B heads][L]), and its backward into dqkv [B L][3C] (in_proj's packed layout)
bool attn_train_supported(int L, int C, int heads);
hipError_t launch_attn_fwd_lse(const float* qkv, float* out, float* lse, int B, int L, int C, int heads, hipStream_t s);
hipError_t launch_attn_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int L,
                           int C, int heads, hipStream_t s);

// ---- gradient clipping + Adam (optim.hip; spdm_adam_step) ------------------------------------------------
// Workgroups of both launches, a compile-time constant: 4 per CU.  The workspace is ADAM_GRID fp64 partial sums of g^2
// followed by the gradient norm.
constexpr int ADAM_GRID = 1024;
constexpr int OPTIM_MAX_SEGMENTS = 4;
struct OptimSeg { float* p; const float* g; float* m; float* v; unsigned long long n; };     // flat fp32 arrays of n floats, 16-byte aligned
struct OptimArgs {
    OptimSeg seg[OPTIM_MAX_SEGMENTS];
    int nseg;
    int clip;                          // 1: the norm launch runs and the update scales g by min(1, max_norm / (norm + 1e-6))
    float max_norm;
    float beta1, beta1_lo, one_minus_beta1, beta2, beta2_lo, one_minus_beta2, eps;     // beta = hi + lo, 1 - beta rounded once from double
    float step_size;                   // lr / (1 - beta1^step), evaluated in double
    float bc2_sqrt;                    // sqrt(1 - beta2^step), evaluated in double
    unsigned long long quads, per;     // filled by the launch: 4-float pieces of all segments, and pieces per workgroup
};
// one or two launches on s: [partial sums of g^2 ->] Adam on every segment in place; workspace: ADAM_GRID + 1 doubles
hipError_t launch_adam_step(OptimArgs a, double* workspace, hipStream_t s);

// ---- EMA of the weights (optim.hip; spdm_ema_step) -----------------------------------------------------------
struct EmaSeg { float* ema; const float* p; unsigned long long n; };     // two flat fp32 arrays of n floats, 16-byte aligned, disjoint
struct EmaArgs {
    EmaSeg seg[OPTIM_MAX_SEGMENTS];
    int nseg;
    float omd;                         // 1 - decay, rounded once from double by the caller
    unsigned long long quads, per;     // filled by the launch, as OptimArgs'
};
// one launch of ADAM_GRID workgroups on s: ema = ema - omd (ema - p) on every segment, on adam_apply_kernel's partition
hipError_t launch_ema_step(EmaArgs a, hipStream_t s);

// ---- the forward (noising) process of a training step (train_noise.hip; spdm_train_forward_process) --------
struct ForwardProcessArgs {
    int B, H, D, inp_h, T;
    const float* x0;                   // (B, H, D) clean window
    const float* inpaint;              // (B, inp_h, D); null iff inp_h == 0
    const float* sqrt_abar;            // [T]
    const float* sqrt_1m_abar;         // [T]
    unsigned long long seed, sample_offset;
    unsigned step;
    const int* t_in;                   // (B) or null: drawn (Philox purpose 2)
    const float* noise_in;             // (B, H, D) or null: drawn (Philox purpose 1)
    int* t_out;                        // (B): the timesteps used (a given one clamped into [0, T)); may be null when t_in is set
    float* noise_out;                  // (B, H, D): the noise used; may be null when noise_in is set
    float* x_noisy;                    // (B, H, D)
    float* time_scale;  int time_dim;  float dropout_p, keep_scale;     // optional (B, time_dim) dropout mask x keep_scale (purpose 3)
    int* clamped;                      // optional: entries of t_in outside [0, T)
};
// one launch of B workgroups
hipError_t launch_forward_process(const ForwardProcessArgs& a, hipStream_t s);
// dst[i] = min(max(src[i], 0), T - 1), i < n (spdm_train_loss_grad_dt: the caller's device timesteps into the handle's)
hipError_t launch_copy_t_clamped(const int* src, int n, int T, int* dst, hipStream_t s);

// ---- training batches gathered from a device-resident dataset (dataset.hip; spdm_dataset_gather) ----------
struct DatasetGatherArgs {
    int n_windows, B, seq_len, step_size, n_frames, img_dtype;      // img_dtype: 0 uint8 (divided by 255), 1 fp32
    int max_start;                     // T - 1 - (seq_len - 1) step_size >= 0: the last start whose window ends inside the stores
    int img_blocks;                    // filled by the launch: B n_frames x 3 frame slices (0 without d_image_out)
    const void* img;                   // (T, 96, 96, 3), 16-byte aligned
    const double* position;            // (T, 2) raw
    const float* velocity;             // (T, 2) normalised
    const float* action;               // (T, 3) normalised
    const int* window_start;           // (n_windows), or null: window i starts at row i
    const int* window_id;              // (B): clamped into [0, n_windows) before use
    double pos_min, pos_max;
    float* image_out;                  // (B, n_frames, 3, 96, 96), 16-byte aligned, or null
    float* position_out;               // (B, seq_len, 2) or null
    float* velocity_out;               // (B, seq_len, 2) or null
    float* action_out;                 // (B, seq_len, 3) or null
    double* translation_out;           // (B, 2) or null
    int* start_out;                    // (B) or null
    int* bad;                          // one int or null: SET to the number of batch slots whose id or start was clamped
};
// one launch of B n_frames x 3 + ceil(B seq_len / 256) workgroups
hipError_t launch_dataset_gather(DatasetGatherArgs a, hipStream_t s);

// ---- planar fp32 frames to interleaved uint8 tiles of a contact sheet (dataset.hip; spdm_frames_to_bytes) ----
struct FramesToU8Args {
    int n, cols;                       // frames; tiles per sheet row
    long long tile_offset;             // frame i is tile tile_offset + i, inside [0, n_tiles): checked by the host
    const float* frames;               // (n, 3, 96, 96), 16-byte aligned
    unsigned char* out;                // (ceil(n_tiles / cols) 96, cols 96, 3), 16-byte aligned
};
// one launch of n x 3 workgroups (a third of a frame each)
hipError_t launch_frames_to_u8(const FramesToU8Args& a, hipStream_t s);

// ---- position / action error of sampled trajectories and its statistics (evaluation.hip; spdm_eval_*) -----
struct EvalErrorsArgs {
    int B, H, D, seq, obs_h, inp_h, P, runs;
    long long first_traj, window_base; // row b belongs to truth slot (first_traj + b) / runs - window_base, in [0, n_slots)
    const float* pred;                 // (B, H, D): the sampler's x_0
    const float* truth_pos;            // (n_slots, seq, 2) normalised
    const float* truth_act;            // (n_slots, seq, 3) normalised; null iff act_err is null
    const double* translation;         // (n_slots, 2)
    double pos_min, pos_max, act_min[3], act_max[3];
    double* pos_err;                   // (B, P)
    double* act_err;                   // (B, P, 3) or null
};
// one launch of ceil(B P / 256) workgroups
hipError_t launch_eval_errors(const EvalErrorsArgs& a, hipStream_t s);

constexpr int EVAL_ROWS_PER_BLOCK = 1024;      // rows one workgroup of the all-rows reduction sums for one column
inline long long eval_reduce_blocks(long long N) { return (N + EVAL_ROWS_PER_BLOCK - 1) / EVAL_ROWS_PER_BLOCK; }
struct EvalReduceArgs {
    long long N, windows;              // N = windows x runs rows
    int C, runs;
    const double* err;                 // (N, C)
    double* window_mean;               // (windows, C)
    double* window_std;                // (windows, C)
    double* mean;                      // (C)
    double* std;                       // (C)
    double* workspace;                 // eval_reduce_blocks(N) x C doubles
};
// five launches on s, each ordered behind the one before: per-window statistics, then sum / mean / squares / std over all rows
hipError_t launch_eval_reduce(const EvalReduceArgs& a, hipStream_t s);

// ---- uniform noise on the observations of a batch of windows (obs_noise.hip; spdm_obs_noise) ---------------
constexpr int OBS_NOISE_MAX_TENSORS = 4;
constexpr int OBS_NOISE_ITEMS = 1024;  // quads (of four elements) one workgroup perturbs
struct ObsNoiseTensor {
    const float* src;                  // rows of src_stride elements; may equal dst
    float* dst;                        // rows of dst_stride elements
    long long inner, src_stride, dst_stride;       // 0 <= inner <= both strides: elements [0, inner) of a row are perturbed
    // filled by plan_obs_noise:
    unsigned nq;                       // quads per row, ceil(inner / 4)
    unsigned block_begin;              // first workgroup of this tensor
    unsigned chunks_per_row;           // nq >= OBS_NOISE_ITEMS: workgroups a row is cut into; else 1
    unsigned rows_per_block;           // nq <  OBS_NOISE_ITEMS: whole rows a workgroup takes; else 1
    int vec;                           // both pointers 16-byte aligned, inner and both strides multiples of 4: 16-byte accesses
};
struct ObsNoiseArgs {
    unsigned long long n_rows, row_offset;         // row_offset + n_rows <= 2^32: checked by the host
    unsigned long long seed;
    unsigned draw;
    float alpha;
    int n_tensors;                     // 1 .. OBS_NOISE_MAX_TENSORS; tensor i draws from Philox purpose 4 + i
    unsigned blocks;                   // filled by plan_obs_noise
    ObsNoiseTensor t[OBS_NOISE_MAX_TENSORS];
};
// host only: the launch geometry of a; false when a row has 2^32 quads or more, a stride is below inner, or the grid would
// exceed 2^31 - 1 workgroups
bool plan_obs_noise(ObsNoiseArgs& a);
// one launch of a.blocks workgroups (none when every inner is 0); a has been through plan_obs_noise
hipError_t launch_obs_noise(const ObsNoiseArgs& a, hipStream_t s);

// ---- the closed-loop policy's observation history and plan (policy.hip; spdm_policy_*) --------------------
constexpr int POLICY_PUSH_PIECES = 1024;           // 16-byte pieces of one frame a workgroup of the push copies (4 per thread)
struct PolicyPushArgs {
    int E, L, img_dtype;               // environments, ring slots per environment, 0 uint8 / 1 fp32
    int slot;                          // n % L: the slot push n goes to
    int frame_pieces;                  // filled by the launch: 1728 (uint8) or 6912 (fp32) 16-byte pieces per frame
    int chunks;                        // filled by the launch: ceil(frame_pieces / POLICY_PUSH_PIECES) workgroups per environment
    int img_blocks;                    // filled by the launch: E x chunks
    const void* img_in;                // (E, 96, 96, 3), 16-byte aligned
    const float* pos_in;               // (E, 2)
    const float* vel_in;               // (E, 2)
    const float* act_in;               // (E, 3)
    const int* fill;                   // (E): non-zero -> the observation goes into all L slots
    void* ring_img;                    // (E, L, 96, 96, 3), 16-byte aligned
    float* ring_pos;                   // (E, L, 2)
    float* ring_vel;                   // (E, L, 2)
    float* ring_act;                   // (E, L, 3)
};
// one launch of E x chunks + ceil(E / 256) workgroups
hipError_t launch_policy_push(PolicyPushArgs a, hipStream_t s);

struct PolicyWindowArgs {
    int E, L, obs_h, step_size, img_dtype;
    int first;                         // n % L: the slot of the oldest entry (the one the next push overwrites)
    int vel_f32, act_f32;              // the statistics arrays' precision: 1 float32 arithmetic, 0 float64 rounded once
    int img_blocks;                    // filled by the launch: E obs_h x 3 frame slices (0 without image_out)
    const void* ring_img;
    const float* ring_pos;
    const float* ring_vel;
    const float* ring_act;
    double pos_min, pos_max, vel_min[2], vel_max[2], act_min[3], act_max[3];
    float* image_out;                  // (E, obs_h, 3, 96, 96), 16-byte aligned, or null
    float* position_out;               // (E, obs_h, 2) or null
    float* velocity_out;               // (E, obs_h, 2) or null
    float* action_out;                 // (E, obs_h, 3) or null
    float* translation_out;            // (E, 2) or null
};
// one launch of E obs_h x 3 + ceil(E obs_h / 256) workgroups
hipError_t launch_policy_window(PolicyWindowArgs a, hipStream_t s);

struct PolicyUnnormalizeArgs {
    int E, H, D, inp_h;
    const float* x0;                   // (E, H, D)
    const float* translation;          // (E, 2)
    double pos_min, pos_max, act_min[3], act_max[3];
    double* waypoints;                 // (E, H - inp_h, 2)
    double* actions;                   // (E, H - inp_h, 3) or null
};
// one launch of ceil(E (H - inp_h) / 256) workgroups
hipError_t launch_policy_unnormalize(const PolicyUnnormalizeArgs& a, hipStream_t s);

// the starting iterate of a warm-started plan (spdm_policy_warm_start)
struct PolicyWarmStartArgs {
    int E, H, D, inp_h;
    int q, f, step_size;               // delta / step_size (clamped to H: beyond that every row is the held last one), delta % step_size
    float sa, sb;                      // sqrt(abar_t), sqrt(1 - abar_t) of the first timestep the loop denoises from
    unsigned long long seed, env_offset;
    unsigned draw;
    const float* prev_x0;              // (E, H, D)
    const float* prev_translation;     // (E, 2)
    const float* translation;          // (E, 2)
    const float* inpaint;              // (E, inp_h, D); null iff inp_h == 0
    const float* noise_in;             // (E, H, D) or null: drawn
    float* x;                          // (E, H, D)
    float* guess;                      // (E, H, D) or null
    float* noise;                      // (E, H, D) or null
};
// one launch of ceil(E ceil(H D / 4) / 256) workgroups
hipError_t launch_policy_warm_start(const PolicyWarmStartArgs& a, hipStream_t s);

// one of K candidate plans per environment (spdm_policy_select)
constexpr int POLICY_SELECT_MAX_K = 64;            // an environment's scores fit one wave
struct PolicySelectArgs {
    int E, K, H, D, inp_h, cols;
    int mode;                          // 0 medoid, 1 coherent
    int rows;                          // coherent: rows [inp_h, inp_h + rows) are scored
    long long guess_row_stride;        // coherent: environment e's guess is row e x guess_row_stride of `guess`
    const float* x0;                   // (E K, H, D)
    const float* guess;                // rows of H D floats, or null (medoid)
    const float* translation;          // (E, 2); null iff spread is null
    double pos_min, pos_max;
    int* chosen;                       // (E)
    float* x0_out;                     // (E, H, D)
    double* scores;                    // (E, K) or null
    double* spread;                    // (E, H - inp_h) or null
};
// one launch of E workgroups
hipError_t launch_policy_select(const PolicySelectArgs& a, hipStream_t s);

// ---- per-sample terms of a validation pass's loss (train_metrics.hip; spdm_loss_terms) -------------------
constexpr int LOSS_WAVES = 4;          // samples (one wave each) per workgroup
struct LossTermsArgs {
    int B, n;                          // samples, elements per sample (H x D)
    long long slot_offset;             // sample b writes slot slot_offset + b, inside [0, n_slots): checked by the host
    const float* eps;                  // (B, n)
    const float* noise;                // (B, n)
    double* terms;                     // (n_slots)
    const int* t_in;                   // (B) or null
    int* slot_t;                       // (n_slots) or null; null iff t_in is null
};
// one launch of ceil(B / LOSS_WAVES) workgroups
hipError_t launch_loss_terms(const LossTermsArgs& a, hipStream_t s);

// ---- per-frame reconstruction error of a validation batch (train_metrics.hip; spdm_recon_terms) -----------
constexpr int RECON_FRAME = 3 * 96 * 96;           // 27648 elements = 6912 quads of four consecutive floats
constexpr int RECON_THREADS = 256;                 // one workgroup per frame: 27 quads per thread
struct ReconTermsArgs {
    int n;                             // frames
    long long slot_offset;             // frame b writes slot slot_offset + b, inside [0, n_slots): checked by the host
    const float* recon;                // (n, 3, 96, 96), 16-byte aligned
    const float* target;               // (n, 3, 96, 96), 16-byte aligned
    double* terms;                     // (n_slots)
};
// one launch of n workgroups
hipError_t launch_recon_terms(const ReconTermsArgs& a, hipStream_t s);

hipError_t launch_advance(int* step_dev, int* t_dev, const int* timesteps_dev, int n_steps, hipStream_t s);
hipError_t launch_set_step(int* step_dev, int* t_dev, const int* timesteps_dev, int n_steps, int i, hipStream_t s);

// What a forward SelfAttention launcher dispatched, recorded by the launcher itself when `route` is given (spdm_op_sa; null in
// the plan).  dry != 0 on entry: the launcher checks, decides and records as for a launch, then returns before it touches the
// device (the grid of sa_fused64's persistent walk, which asks the device for its CU count, then stays -1).
enum { SA_ROUTE_FUSED = 0, SA_ROUTE_FUSED_PAIR, SA_ROUTE_CROP, SA_ROUTE_QKV, SA_ROUTE_HEAD, SA_ROUTE_TAIL, SA_ROUTE_CORE_DS,
       SA_ROUTE_CORE_VALU, SA_ROUTE_CORE_MFMA };
struct SaRoute { int dry; int kernel, waves, grid, wlds, qw; };      // waves per workgroup, workgroups; qw: queries per wave (crop)

// ---- attention core (attention.hip): softmax(q k^T / sqrt d) v per (sample, head) -----------
hipError_t launch_attention(const float* qkv /*[B*L][3C]*/, float* out /*[B*L][C]*/, int B, int L, int C,
                            int heads, hipStream_t s, SaRoute* route = nullptr);        // VALU kernel (small L)
hipError_t launch_attention_auto(const float* qkv, float* out, int B, int L, int C, int heads, unsigned sw, hipStream_t s,
                                 SaRoute* route = nullptr);  // MFMA kernel for L >= 32

// ---- fused SelfAttention block for the C = 64 levels (sa_fused.hip) -------------------------------------
bool sa_fused_supported(int L, int C);
// w_hl: {Wqkv hi, lo, Wo hi, lo, W1 hi, lo, W2 hi, lo} as fp16 [rows][64], input axis permuted by perm16 inside
// each group of 16, pre-scaled by 128 (spdm_api.hip: Loader::perm_split)
// ab (optional): the block input is ab-affine of x per sample (film_coef_kernel), applied on load
// crop (optional): the block's only consumer is outc + unpad (sa6), so only the H0 x D tokens at (lh, lw) of the Hp x Wp map
// are computed (sa_crop64_kernel): out holds the block output at those tokens only, or -- eps non-null -- outc is applied in the
// epilogue and eps [B][H0][D] is written instead of out
struct SaCrop { int H0, D, Wp, lh, lw; const float* outc_w; float outc_b; float* eps; };
bool sa_crop_supported(int L, int C, int H0, int D);
hipError_t launch_sa_fused64(const float* x, float* out, int B, int L, const float* ln1_g, const float* ln1_b,
                             const float* ln2_g, const float* ln2_b, const void* const w_hl[8], const float* bqkv,
                             const float* bo, const float* b1, const float* b2, const float* ab, unsigned sw, hipStream_t s,
                             const FilmSpec* fs = nullptr, const SaCrop* crop = nullptr, SaRoute* route = nullptr);

// ---- row-wise tail of a C = 128 / 256 SelfAttention block (sa_tail.hip): out_proj + x -> LayerNorm -> ff1 -> GELU -> ff2 + av ----
bool sa_tail_supported(int C, unsigned sw);
hipError_t launch_sa_tail(int C, const float* o, const float* x, float* out, int rows, const float* wf_o, const float* wf_1,
                          const float* wf_2, const float* b_o, const float* b_1, const float* b_2, const float* ln_g,
                          const float* ln_b, const float* ab, int L, hipStream_t s, const FilmSpec* fs = nullptr,
                          SaRoute* route = nullptr, float* pool = nullptr, int W = 0);
// pool (optional, null from spdm_op_sa): the launch also writes MaxPool2d(2) of out, [rows / 4][C], the samples being L-row maps W
// columns wide -- where sa_tail_pools says every window lies inside one workgroup's rows
bool sa_tail_pools(int C, int L, int W, int rows);
// may the two kernels evaluate the FiLM coefficients themselves for samples of L rows?  (their LDS row per touched sample)
bool sa_tail_film_local(int C, int L);
// LayerNorm + in_proj + attention core in one kernel (att = softmax(q k^T / sqrt d) v per sample and head, heads concatenated):
// blocks whose 8192 / C-row tile holds whole samples of L tokens
bool sa_head_supported(int C, int L, unsigned sw);
hipError_t launch_sa_head(int C, const float* x, float* att, int rows, const float* wf_in, const float* b_in, const float* ln_g,
                          const float* ln_b, const float* ab, int L, hipStream_t s, const FilmSpec* fs = nullptr,
                          SaRoute* route = nullptr);
// qkv = LayerNorm(x) W_in^T + b_in of the same blocks (LayerNorm from the row itself)
hipError_t launch_sa_qkv(int C, const float* x, float* qkv, int rows, const float* wf_in, const float* b_in, const float* ln_g,
                         const float* ln_b, const float* ab, int L, hipStream_t s, const FilmSpec* fs = nullptr,
                         SaRoute* route = nullptr);

// ---- weight re-layout on the device (weight_layout.hip; spdm_api.hip's Recorder records the copies) ----------------------
// One kernel-layout copy of a weight as a gather from the torch-layout blob: logical dense array [n0][n1][n2], element
// (i0, i1, i2) = blob[src + sum_k contrib_k] where axis k contributes i_k * stride[k] (zero when i_k >= lim[k]) or, tab[k] >= 0,
// tabs[tab[k] + i_k] (zero when that entry is -1).  fmt says how the logical elements become the destination:
//   WL_F32      the logical array itself (bit copy)
//   WL_SPLIT    split format of it: per 32-element chunk 32 fp16 hi | 32 fp16 lo of 128 w (same byte size)
//   WL_FRAG     the fragment-order copy of that split array, read as [taps][N][K] (layout: weight_layout.hip)
//   WL_PERM_HI / _LO   the hi / lo fp16 halves of a [out][64] matrix in sa_fused.hip's fragment order (half the bytes)
//   WL_RANGE    no destination: flags[slot] = 1 when an element is outside the split format's range, !(|w| < 511)
enum { WL_F32 = 0, WL_SPLIT, WL_FRAG, WL_PERM_HI, WL_PERM_LO, WL_RANGE, WL_NFMT };
struct WeightCopy {
    long long src = 0;
    long long stride[3] = {0, 0, 0};
    int n[3] = {1, 1, 1};
    int lim[3] = {1, 1, 1};
    int tab[3] = {-1, -1, -1};
    int fmt = WL_F32;
    int taps = 1, N = 0, K = 0;          // WL_FRAG geometry
    int slot = -1;                       // WL_RANGE: flag index (one per tensor name)
    void* dst = nullptr;
    long long count = 0;                 // destination floats (WL_RANGE: logical elements)
    long long blk0 = 0;                  // first workgroup of this copy in its format's launch
};
long long weight_copy_blocks(long long count);
// one launch over copies[0, n_copies) -- all of format fmt, blk0 ascending, `blocks` workgroups in all
hipError_t launch_weight_copies(int fmt, const float* blob, const long long* tabs, const WeightCopy* copies, int n_copies,
                                long long blocks, int* flags, hipStream_t s);

}  // namespace spdm
