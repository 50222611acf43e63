// spdm_api.hip -- host side of libspdm_hip.so: the C ABI of include/spdm.h, the weight re-layout,
// the workspace arena and the launch plan of one U-Net evaluation / one denoise step.
//
// The plan follows UNet_Film.forward (models/Unet_FiLmLayer.py:277-312) block by block; every
// launch_* call names the kernel that replaces the torch ops of that line range (kernels.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/spdm.h"
#include "kernels.h"

using namespace spdm;

// -------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail(SPDM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define SPDM_TRY(expr)              \
    do {                            \
        int _r = (expr);            \
        if (_r != SPDM_OK) return _r; \
    } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// -------------------------------------------------------------------------------------------------
// Workspace arena: first-fit free list over one hipMalloc'd slab.  The plan allocates and releases
// in a deterministic order, so a dry run with max_batch at create() sizes the slab exactly.
struct Arena {
    char* base = nullptr;
    size_t cap = 0, peak = 0;
    bool dry = false, keep = false;
    struct Blk { size_t off, size; bool free; };
    std::vector<Blk> blks;
    void reset() {
        blks.clear();
        blks.push_back({0, (size_t)1 << 60, true});
    }
    bool alloc(size_t bytes, size_t* off) {
        bytes = align_up(std::max<size_t>(bytes, 256), 256);
        for (size_t i = 0; i < blks.size(); ++i) {
            if (blks[i].free && blks[i].size >= bytes) {
                const size_t o = blks[i].off, rest = blks[i].size - bytes;
                blks[i].size = bytes;
                blks[i].free = false;
                if (rest) blks.insert(blks.begin() + i + 1, Blk{o + bytes, rest, true});
                peak = std::max(peak, o + bytes);
                if (!dry && o + bytes > cap) return false;
                *off = o;
                return true;
            }
        }
        return false;
    }
    void release(size_t off) {
        if (keep) return;
        for (size_t i = 0; i < blks.size(); ++i)
            if (blks[i].off == off && !blks[i].free) {
                blks[i].free = true;
                if (i + 1 < blks.size() && blks[i + 1].free) {
                    blks[i].size += blks[i + 1].size;
                    blks.erase(blks.begin() + i + 1);
                }
                if (i > 0 && blks[i - 1].free) {
                    blks[i - 1].size += blks[i].size;
                    blks.erase(blks.begin() + i);
                }
                return;
            }
    }
};

struct Tensor {            // channels-last activation [B][HW_level][C] living in the arena
    float* p = nullptr;
    size_t off = 0;
    int C = 0, level = 0;
    bool valid = false;
};
struct StatsBuf {          // GroupNorm partial sums of a raw conv output
    double* p = nullptr;
    size_t off = 0;
    StatsRef ref{};
    bool valid = false;
};
struct Value {             // a tensor plus the GroupNorm affine still pending on it (if any)
    Tensor t;
    StatsBuf st;
    const float* gamma = nullptr;
    const float* beta = nullptr;
    bool pending_gn() const { return st.valid; }
};

struct ConvW { float* w = nullptr; float* ws = nullptr; float* wf = nullptr; int taps = 0, cin = 0, cout = 0;
               int cnorm = 0;
               float* wt = nullptr; };   // wt (SPDM_FLAG_TRAIN): [taps][Cin][Cout], taps flipped -- the data-gradient convolution's weights
                                         // (SPDM_FLAG_TRAIN_SIMPLE: at the padded widths, [taps][mi.width][mo.width])
                                         // cnorm > 0: real output channels of a channel-padded layer (its GroupNorm divides by these)   // ws: split-fp16 copy; wf: its fragment-order copy (conv_wide.hip)
struct DoubleConvW { ConvW first, second; float* gamma = nullptr; float* beta = nullptr; };
struct LinW { float* w = nullptr; float* ws = nullptr; float* b = nullptr; int in = 0, out = 0;
              float* wt = nullptr; };   // wt (SPDM_FLAG_TRAIN, FiLM encoders): [in padded to 64][out], the data gradient's weights;
                                        // (SPDM_FLAG_TRAIN_ATTENTION, attention Linears): [in][out]
struct ResampleW { DoubleConvW dc1, dc2; LinW emb, film; float* temb_table = nullptr; int cout = 0; };
struct AttnW {
    LinW in_proj, out_proj, ff1, ff2;
    float* ln_g = nullptr; float* ln_b = nullptr; float* ff_ln_g = nullptr; float* ff_ln_b = nullptr;
    int C = 0;
    void* fw[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // fused-kernel weights (C == 64)
    float* tail_wf[3] = {nullptr, nullptr, nullptr};   // fragment-order split copies of out_proj / ff1 / ff2 (C == 128: sa_tail.hip)
    float* qkv_wf = nullptr;                           // ... and of in_proj
};

// -------------------------------------------------------------------------------------------------
// The device weight-copy table (weight_layout.hip): the recorded copies (a Recorder, below, fills it in), the split format's
// range checks and the copies' offset tables, their device mirrors and every device allocation made for them, the copies'
// destinations included.  A spdm_handle and each frame handle (FrameNet: spdm_encoder, spdm_decoder) hold one; the standalone
// GEMM entry points build a temporary one.
struct WeightTable {
    std::vector<WeightCopy> copies;       // every copy, in the order it was recorded (spdm_debug_weight_digest)
    std::vector<WeightCopy> ranges;       // the split format's range checks (WL_RANGE)
    std::vector<long long> tabs;          // offset tables of the copies' table axes
    std::vector<std::string> slots;       // tensor name of each range slot
    std::vector<int> oor;                 // ... outside the range at load (those tensors have no split copies)
    long long scalar_off = -1;            // >= 0: one blob float read back with the verdicts (outc's bias)
    WeightCopy* d_copies = nullptr;       // the copies on the device, grouped by format
    WeightCopy* d_ranges = nullptr;
    int first[WL_NFMT] = {}, count[WL_NFMT] = {};
    long long blocks[WL_NFMT] = {};       // per format: first entry, entries and workgroups of its launch
    long long* d_tabs = nullptr;
    int* d_flags = nullptr;               // [slots] range verdicts + the scalar (bits), read back together
    std::vector<void*> owned;             // every hipMalloc to free
    size_t bytes = 0;
    WeightTable() = default;
    WeightTable(const WeightTable&) = delete;
    WeightTable& operator=(const WeightTable&) = delete;
    ~WeightTable() { clear(); }
    void clear() {                        // back to an empty table
        for (void* p : owned) (void)hipFree(p);
        owned.clear(); copies.clear(); ranges.clear(); tabs.clear(); slots.clear(); oor.clear();
        d_copies = d_ranges = nullptr; d_tabs = nullptr; d_flags = nullptr;
        scalar_off = -1; bytes = 0;
    }
    int alloc(void** p, size_t n) {
        HIP_TRY(hipMalloc(p, std::max<size_t>(n, 256)));
        owned.push_back(*p);
        bytes += n;
        return SPDM_OK;
    }
    // the recorded range checks (rng) or copies on the device, grouped by format in launch order (each format's workgroups
    // numbered from 0).  Called again when more copies have been recorded; the earlier mirror stays owned.
    int upload(bool rng) {
        if (!d_tabs && !tabs.empty()) {
            SPDM_TRY(alloc((void**)&d_tabs, sizeof(long long) * tabs.size()));
            HIP_TRY(hipMemcpy(d_tabs, tabs.data(), sizeof(long long) * tabs.size(), hipMemcpyHostToDevice));
        }
        if (rng) SPDM_TRY(alloc((void**)&d_flags, sizeof(int) * (slots.size() + 1)));
        std::vector<WeightCopy> t;
        for (int f = rng ? WL_RANGE : 0; f < (rng ? WL_RANGE + 1 : WL_RANGE); ++f) {
            first[f] = (int)t.size();
            long long blk = 0;
            for (WeightCopy c : rng ? ranges : copies)
                if (c.fmt == f) { c.blk0 = blk; blk += weight_copy_blocks(c.count); t.push_back(c); }
            count[f] = (int)t.size() - first[f];
            blocks[f] = blk;
        }
        if (t.empty()) return SPDM_OK;
        WeightCopy** d = rng ? &d_ranges : &d_copies;
        SPDM_TRY(alloc((void**)d, sizeof(WeightCopy) * t.size()));
        HIP_TRY(hipMemcpy(*d, t.data(), sizeof(WeightCopy) * t.size(), hipMemcpyHostToDevice));
        return SPDM_OK;
    }
    // enqueue the range checks of a device blob and read their verdicts back, with the scalar: one synchronisation
    int check_ranges(const float* d_blob, hipStream_t s, std::vector<int>* verdicts, float* scalar = nullptr) {
        const size_t ns = slots.size();
        if (ns) HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int) * ns, s));
        HIP_TRY(launch_weight_copies(WL_RANGE, d_blob, d_tabs, d_ranges, count[WL_RANGE], blocks[WL_RANGE], d_flags, s));
        if (scalar_off >= 0) HIP_TRY(hipMemcpyAsync(d_flags + ns, d_blob + scalar_off, sizeof(float), hipMemcpyDeviceToDevice, s));
        std::vector<int> back(ns + 1);
        HIP_TRY(hipMemcpyAsync(back.data(), d_flags, sizeof(int) * (ns + 1), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        verdicts->assign(back.begin(), back.begin() + ns);
        if (scalar) memcpy(scalar, &back[ns], sizeof(float));
        return SPDM_OK;
    }
    // enqueue every kernel-layout copy of a device blob into the copies' buffers
    int relayout(const float* d_blob, hipStream_t s) {
        for (int f = WL_F32; f < WL_RANGE; ++f)
            HIP_TRY(launch_weight_copies(f, d_blob, d_tabs, d_copies + first[f], count[f], blocks[f], nullptr, s));
        return SPDM_OK;
    }
};

// a host blob on the device for as long as a table is being built from it
struct DevBlob {
    float* p = nullptr;
    ~DevBlob() { if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); } }
    int upload(const float* blob, size_t n) {
        HIP_TRY(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(float)));
        HIP_TRY(hipMemcpy(p, blob, n * sizeof(float), hipMemcpyHostToDevice));
        return SPDM_OK;
    }
};

struct ProfEvt { hipEvent_t a, b; double flops; int launches; };

struct spdm_handle {
    spdm_config cfg{};
    int Hp = 0, Wp = 0, lh = 0, uh = 0, lw = 0, uw = 0;
    int film_kp = 0;
    // weights
    std::vector<void*> owned;             // every hipMalloc to free
    float* w_inc_first = nullptr;         // [9][64]
    DoubleConvW inc, bot[3];
    ResampleW down[3], up[3];
    AttnW sa[6];
    float* outc_w = nullptr;
    float outc_b = 0.f;                   // a host scalar: the step kernel's argument
    WeightTable wt;                       // every kernel-layout copy of the weights; what spdm_update_weights replays on a new blob
    size_t blob_floats = 0;               // size of the loaded blob
    bool weights_loaded = false, temb_ready = false;
    bool train = false;                   // SPDM_FLAG_TRAIN: spdm_train_loss_grad (train_pass)
    bool train_attn = false;              // ... SPDM_FLAG_TRAIN_ATTENTION: through the SelfAttention blocks (TrainPass::sa_fwd / sa_bwd)
    std::map<std::string, size_t> grad_off;   // ... offset of every tensor in the last spdm_load_weights blob
    size_t grad_floats = 0;               // ... and that blob's size
    float* tws = nullptr;                 // ... training workspace (train_pass at max_batch)
    size_t tws_floats = 0;
    bool simple = false;                  // SPDM_FLAG_SIMPLE_UNET: models/simple_Unet.py (plan_simple); inc / down / up hold its blocks
    LinW cemb;                            // ... its six cond_emb_layer projections stacked: [6 x 32][film_kp]
                                          //     (SPDM_FLAG_TRAIN_SIMPLE: cemb.wt = [cond_dim padded to 64][6 x 32], d SiLU(cond))
    bool train_simple = false;            // SPDM_FLAG_TRAIN_SIMPLE: spdm_train_loss_grad of simple_Unet.py (train_pass_simple)
    int* d_pos16 = nullptr;               // ... device channel maps (ChanMap::pos) of input_conv's 16 channels,
    int* d_pos_in[6] = {};                //     of each block's input and
    int* d_pos_out[6] = {};               //     of its doubleConv2 output (simple_in_map(k), ChanMap::ident(cout))
    float* d_time_pe = nullptr;           // ... the raw time table pe (T, time_dim) on the device, for the dropout multiplier
    const float* t_scale = nullptr;       // ... spdm_train_set_time_scale: (t_scale_B, time_dim) multiplier of the next call
    int t_scale_B = 0;
    float* d_cemb = nullptr;              // ... Linear(SiLU(cond)) of the call, [B][6 x 32]
    bool split = true;                    // split-fp16 MFMA path (default); SPDM_PREC=f32 selects the exact fp32 MFMA path
    unsigned sw = 0;                      // kernel-selection switches (SW_*, kernels.h): environment read once at create
    int demoted = 0;                      // tensors outside the split format's range, kept on the exact fp32 kernels
    std::vector<float> time_table;        // host (T, time_dim)
    float* d_time_silu = nullptr;         // device SiLU(pos_encoding) (T, time_dim)
    // schedule
    int sched_kind = -1, n_steps = 0;
    std::vector<int> timesteps;
    int* d_timesteps = nullptr;
    float* d_coef = nullptr;
    // SPDM_DPMPP_2M only, allocated when such a schedule is first installed (install_schedule)
    float* d_x0_prev = nullptr;           // [max_batch][H][D] the previous step's predicted x0 (solver_step_kernel)
    float* d_solver_eps = nullptr;        // [max_batch][H][D] eps of the step on routes where sa6's epilogue has not produced it
    int* d_first = nullptr;               // the iteration the running spdm_sample_run starts at, or -1 when it continues the history
    // persistent per-call state (sized for max_batch)
    int* d_t = nullptr;                   // [max_batch] timestep(s) of the current evaluation
    int* d_step = nullptr;                // [0] loop iteration, [2] non-finite flag (set by out_step_kernel)
    unsigned long long* d_rng = nullptr;  // {seed, first global trajectory index} of the device noise stream
    const void** d_ptrs = nullptr;        // {inpaint, noise, history} of the session: read by out_step_kernel (StepArgs::ptrs_dev)
    float* d_condm = nullptr;             // Mish(cond), K padded
    float* d_film[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float* d_x = nullptr;                 // current iterate (B,H0,D)
    float* d_partial = nullptr;           // split-K partial slabs of the launch in flight (SPLITK_WORKSPACE_BYTES)
    bool have_film = false;
    // sampling session
    int sB = 0, s_inp_h = 0, s_inp_per_sample = 0;
    const float* s_inpaint = nullptr;
    const float* s_noise = nullptr;
    float* s_history = nullptr;
    unsigned long long s_seed = 0, s_offset = 0;
    bool session = false;
    int s_last_step = -2;                 // the last iteration this session completed (-2: none); SPDM_DPMPP_2M's history is its x0
    // arena
    Arena arena;
    size_t persistent_bytes = 0;
    // debug
    std::map<std::string, Tensor> taps;
    int tapB = 0;
    // hipGraph of one denoise step (advance -> U-Net -> scheduler update), replayed by spdm_sample_run
    struct StepGraphKey {
        int B = 0, inp_h = 0, per_sample = 0, have_film = 0, sched_kind = 0, n_steps = 0;
        unsigned env = 0;                 // the handle's kernel-selection switches when the step was captured
        // NOT part of the key: seed and trajectory offset (out_step_kernel reads them from d_rng) and the ADDRESSES of the
        // caller's inpaint / noise / history buffers (read from d_ptrs) -- a fresh seed, or freshly allocated tensors of the
        // same shapes, replay the same graph.  Presence or absence of a buffer needs no entry either: the kernel tests the
        // pointer it loads.
        bool operator==(const StepGraphKey& o) const {
            return env == o.env && B == o.B && inp_h == o.inp_h && per_sample == o.per_sample && have_film == o.have_film &&
                   sched_kind == o.sched_kind && n_steps == o.n_steps;
        }
    } graph_key;
    long long graph_captures = 0;         // step graphs built so far (spdm_graph_captures)
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
    hipStream_t gstream = nullptr;        // blocking stream the loop runs on when the caller passes the NULL stream
    // profiling of the dominant kernel class
    bool prof = false;
    std::vector<ProfEvt> prof_evts;       // event pairs in use since the last reset
    std::vector<ProfEvt> prof_pool;       // created ahead of time (spdm_profile_enable(h, 2)) / recycled: no hipEventCreate while timing
    int prof_open = -1;                   // index of the event pair that brackets the current run of consecutive conv launches
    long long prof_launches = 0;
    double prof_ms = 0.0, prof_flops = 0.0;
};

static int dev_alloc(spdm_handle* h, void** p, size_t bytes) {
    HIP_TRY(hipMalloc(p, std::max<size_t>(bytes, 256)));
    h->owned.push_back(*p);
    h->persistent_bytes += bytes;
    return SPDM_OK;
}

// -------------------------------------------------------------------------------------------------
// schedule tables (host, fp32, operation order of diffusers 0.17.1 -- see oracle/scheduler_ref.py)
#pragma clang fp contract(off)
static int build_schedule(int kind, int T, int n, float beta_start, float beta_end, int* ts, float* coef) {
    if (T < 1 || n < 1 || n > T) return fail(SPDM_ERR_INVALID, "schedule: need 1 <= n (%d) <= T (%d)", n, T);
    if (kind != SPDM_DDPM && kind != SPDM_DDIM) return fail(SPDM_ERR_INVALID, "schedule: unknown kind %d", kind);
    std::vector<float> acp(T);
    {   // torch.linspace(fp32): symmetric evaluation from both ends; alphas = 1 - betas; cumprod
        const float step = (T > 1) ? (beta_end - beta_start) / (float)(T - 1) : 0.f;
        float run = 1.0f;
        for (int i = 0; i < T; ++i) {
            const float beta = (i < T / 2) ? beta_start + step * (float)i : beta_end - step * (float)(T - 1 - i);
            const float alpha = 1.0f - beta;
            run = (i == 0) ? alpha : run * alpha;
            acp[i] = run;
        }
    }
    const int ratio = T / n;
    for (int i = 0; i < n; ++i) {
        const int t = (n - 1 - i) * ratio;
        const int prev_t = t - ratio;
        ts[i] = t;
        const float a_t = acp[t];
        const float a_prev = (prev_t >= 0) ? acp[prev_t] : 1.0f;
        const float b_t = 1.0f - a_t;
        float* c = coef + (size_t)i * 6;
        c[0] = sqrtf(b_t);
        c[1] = sqrtf(a_t);
        c[2] = c[3] = c[4] = c[5] = 0.f;
        if (kind == SPDM_DDPM) {
            const float b_prev = 1.0f - a_prev;
            const float cur_a = a_t / a_prev;
            const float cur_b = 1.0f - cur_a;
            c[2] = (sqrtf(a_prev) * cur_b) / b_t;
            c[3] = sqrtf(cur_a) * b_prev / b_t;
            if (t > 0) {
                float var = (1.0f - a_prev) / (1.0f - a_t) * cur_b;
                if (var < 1e-20f) var = 1e-20f;
                c[5] = sqrtf(var);
            }
        } else {
            c[2] = sqrtf(a_prev);
            c[4] = sqrtf(1.0f - a_prev - 0.0f);
        }
    }
    return SPDM_OK;
}

// pos_encoding(t) for t = 0..T-1 (models/Unet_FiLmLayer.py:266-274), default host computation
static void default_time_table(std::vector<float>& tab, int T, int dim) {
    tab.resize((size_t)T * dim);
    const int half = dim / 2;
    for (int i = 0; i < half; ++i) {
        const float expo = (float)(2 * i) / (float)dim;
        const float inv_freq = 1.0f / powf(10000.0f, expo);
        for (int t = 0; t < T; ++t) {
            const float arg = (float)t * inv_freq;
            tab[(size_t)t * dim + i] = sinf(arg);
            tab[(size_t)t * dim + half + i] = cosf(arg);
        }
    }
}

// -------------------------------------------------------------------------------------------------
unsigned spdm::switches_from_env() {
    int n = 0;
    const SwitchName* t = switch_table(&n);
    unsigned sw = 0;
    for (int i = 0; i < n; ++i)
        if (getenv(t[i].env) != nullptr) sw |= t[i].bit;
    return sw;
}

extern "C" int spdm_abi_version(void) { return SPDM_ABI_VERSION; }
extern "C" const char* spdm_last_error(void) { return g_err; }

extern "C" int spdm_schedule_tables(int32_t kind, int32_t T, int32_t n, float beta_start, float beta_end,
                                    int32_t* ts, float* coef) {
    if (!ts || !coef) return fail(SPDM_ERR_INVALID, "null output");
    return build_schedule(kind, T, n, beta_start, beta_end, ts, coef);
}

static int dry_plan_all(spdm_handle* h);      // the sizing pass, with the plan below

// ---- models/simple_Unet.py in channel-padded storage ----
// Every tensor and every convolution of this network is stored with a multiple of 64 channels (the implicit-GEMM kernels need
// K % 32 == 0 and N % 64 == 0).  A ChanMap says where each real channel lives; the other lanes hold exact zeros: zero weight
// rows and columns, zero GroupNorm gain and offset, statistics over the real channel count (ConvW::cnorm).  An UpSample's
// concatenation keeps both halves at their own padded widths, so its first convolution's input channels are re-laid out on load.
struct ChanMap {
    int width = 0;
    std::vector<int> pos;                 // storage position of real channel i
    int real() const { return (int)pos.size(); }
    static ChanMap ident(int C) {
        ChanMap m;
        m.width = (int)align_up((size_t)C, 64);
        for (int i = 0; i < C; ++i) m.pos.push_back(i);
        return m;
    }
    static ChanMap cat(const ChanMap& a, const ChanMap& b) {
        ChanMap m;
        m.width = a.width + b.width;
        m.pos = a.pos;
        for (int p : b.pos) m.pos.push_back(a.width + p);
        return m;
    }
};
// UNet.__init__, simple_Unet.py:270-280: blocks down1..3, up1..3 -- input channels (cin_b > 0: cat(upsampled cin_a, skip cin_b))
// and the output channels of doubleConv2; each block then appends 32 conditioning channels
struct SimpleBlock { int cin_a, cin_b, cout; };
static const SimpleBlock kSimpleBlocks[6] = {{16, 0, 32}, {64, 0, 128}, {160, 0, 256}, {288, 160, 128}, {160, 64, 64}, {96, 16, 32}};
static constexpr int SIMPLE_COND_CH = 32;       // cond_emb_layer output width (simple_Unet.py:149,200)
static ChanMap simple_in_map(int k) {
    const SimpleBlock& b = kSimpleBlocks[k];
    return b.cin_b ? ChanMap::cat(ChanMap::ident(b.cin_a), ChanMap::ident(b.cin_b)) : ChanMap::ident(b.cin_a);
}
static int simple_out_width(int k) { return (int)align_up((size_t)kSimpleBlocks[k].cout + SIMPLE_COND_CH, 64); }
static ResampleW& simple_block(spdm_handle* h, int k) { return k < 3 ? h->down[k] : h->up[k - 3]; }

// channel / tap geometry of every layer (UNet_Film.__init__, models/Unet_FiLmLayer.py:246-264); known
// before any weight is loaded, so that create() can size the workspace with a dry run of the plan
static void init_arch(spdm_handle* h) {
    // level-3 maps are (Hp/8) x 1: a 3x3 kernel only ever multiplies its centre column there
    const int t3 = (h->Wp >> 3) == 1 ? 3 : 9;
    if (h->simple) {
        auto shape = [](ConvW& c, const ChanMap& in, const ChanMap& out, int taps) {
            c.cin = in.width; c.cout = out.width; c.taps = taps; c.cnorm = out.real();
        };
        const ChanMap c16 = ChanMap::ident(16);
        shape(h->inc.second, c16, c16, 9);
        for (int k = 0; k < 6; ++k) {
            ResampleW& r = simple_block(h, k);
            const ChanMap in = simple_in_map(k), out = ChanMap::ident(kSimpleBlocks[k].cout);
            const int taps = (k == 2) ? t3 : 9;   // down3 runs on the level-3 maps
            shape(r.dc1.first, in, in, taps);
            shape(r.dc1.second, in, in, taps);
            shape(r.dc2.first, in, out, taps);
            shape(r.dc2.second, out, out, taps);
            r.cout = kSimpleBlocks[k].cout;
        }
        return;
    }
    auto dc = [](DoubleConvW& d, int cin, int cout, int taps) {
        d.first.cin = cin; d.first.cout = cout; d.first.taps = taps;
        d.second.cin = cout; d.second.cout = cout; d.second.taps = taps;
    };
    auto rs = [&](ResampleW& r, int cin, int cout, int taps) {
        dc(r.dc1, cin, cin, taps);
        dc(r.dc2, cin, cout, taps);
        r.cout = cout;
    };
    dc(h->inc, 1, 64, 9);
    rs(h->down[0], 64, 128, 9);
    rs(h->down[1], 128, 256, 9);
    rs(h->down[2], 256, 256, t3);
    dc(h->bot[0], 256, 512, t3);
    dc(h->bot[1], 512, 512, t3);
    dc(h->bot[2], 512, 256, t3);
    rs(h->up[0], 512, 128, 9);
    rs(h->up[1], 256, 64, 9);
    rs(h->up[2], 128, 64, 9);
    static const int sc[6] = {128, 256, 256, 128, 64, 64};
    for (int i = 0; i < 6; ++i) h->sa[i].C = sc[i];
}

static size_t train_workspace_floats(spdm_handle* h);

extern "C" int spdm_create(const spdm_config* cfg, spdm_handle** out) {
    if (!cfg || !out) return fail(SPDM_ERR_INVALID, "null argument");
    if (cfg->horizon < 1 || cfg->state_dim < 1 || cfg->state_dim > 8)
        return fail(SPDM_ERR_INVALID, "horizon must be >= 1 and 1 <= state_dim <= 8 (got %d, %d)", cfg->horizon, cfg->state_dim);
    if (cfg->time_dim < 32 || cfg->time_dim % 32 != 0) return fail(SPDM_ERR_INVALID, "time_dim must be a multiple of 32");
    if (cfg->cond_dim < 0 || cfg->max_batch < 1 || cfg->num_train_timesteps < 1)
        return fail(SPDM_ERR_INVALID, "cond_dim >= 0, max_batch >= 1, num_train_timesteps >= 1 required");
    if ((cfg->flags & SPDM_FLAG_SIMPLE_UNET) && cfg->attention != 0)
        return fail(SPDM_ERR_INVALID, "SPDM_FLAG_SIMPLE_UNET (models/simple_Unet.py) has no attention blocks: attention must be 0");
    if ((cfg->flags & SPDM_FLAG_TRAIN_ATTENTION) &&
        (!(cfg->flags & SPDM_FLAG_TRAIN) || cfg->attention == 0 || (cfg->flags & SPDM_FLAG_SIMPLE_UNET)))
        return fail(SPDM_ERR_INVALID, "SPDM_FLAG_TRAIN_ATTENTION needs SPDM_FLAG_TRAIN and attention = 1 (UNet_Film), no SPDM_FLAG_SIMPLE_UNET");
    if ((cfg->flags & SPDM_FLAG_TRAIN_SIMPLE) &&
        (!(cfg->flags & SPDM_FLAG_TRAIN) || !(cfg->flags & SPDM_FLAG_SIMPLE_UNET) || (cfg->flags & SPDM_FLAG_TRAIN_ATTENTION)))
        return fail(SPDM_ERR_INVALID, "SPDM_FLAG_TRAIN_SIMPLE needs SPDM_FLAG_TRAIN and SPDM_FLAG_SIMPLE_UNET, no SPDM_FLAG_TRAIN_ATTENTION");
    if ((cfg->flags & SPDM_FLAG_TRAIN) && (cfg->flags & SPDM_FLAG_SIMPLE_UNET) && !(cfg->flags & SPDM_FLAG_TRAIN_SIMPLE))
        return fail(SPDM_ERR_INVALID, "SPDM_FLAG_TRAIN with SPDM_FLAG_SIMPLE_UNET (simple_Unet.py) needs SPDM_FLAG_TRAIN_SIMPLE as well; "
                                      "without it the flag serves UNet_Film_noAttention, or UNet_Film with SPDM_FLAG_TRAIN_ATTENTION");
    if ((cfg->flags & SPDM_FLAG_TRAIN) && cfg->attention != 0 && !(cfg->flags & SPDM_FLAG_TRAIN_ATTENTION))
        return fail(SPDM_ERR_INVALID, "SPDM_FLAG_TRAIN with attention = 1 (UNet_Film) needs SPDM_FLAG_TRAIN_ATTENTION as well; "
                                      "without it the flag serves UNet_Film_noAttention only (attention = 0)");
    if ((cfg->flags & SPDM_FLAG_SIMPLE_UNET) && cfg->cond_dim < 1)
        return fail(SPDM_ERR_INVALID, "SPDM_FLAG_SIMPLE_UNET needs cond_dim >= 1 (the network is only defined with conditioning)");
    HIP_TRY(hipSetDevice(cfg->device));
    spdm_handle* h = new spdm_handle();
    h->cfg = *cfg;
    h->simple = (cfg->flags & SPDM_FLAG_SIMPLE_UNET) != 0;
    h->train = (cfg->flags & SPDM_FLAG_TRAIN) != 0;
    h->train_attn = (cfg->flags & SPDM_FLAG_TRAIN_ATTENTION) != 0;
    h->train_simple = (cfg->flags & SPDM_FLAG_TRAIN_SIMPLE) != 0;
    h->sw = switches_from_env();          // the ONLY place the product path reads SPDM_* switches
    if (const char* pe = getenv("SPDM_PREC")) h->split = !(strcmp(pe, "f32") == 0 || strcmp(pe, "fp32") == 0);
    if (cfg->flags & SPDM_FLAG_EXACT_FP32) h->split = false;
    // pad_to(x, 8): models/Unet_FiLmLayer.py:15-28
    const int H0 = cfg->horizon, D = cfg->state_dim;
    h->Hp = (H0 % 8) ? H0 + 8 - H0 % 8 : H0;
    h->Wp = (D % 8) ? D + 8 - D % 8 : D;
    h->lh = (h->Hp - H0) / 2;  h->uh = (h->Hp - H0) - h->lh;
    h->lw = (h->Wp - D) / 2;   h->uw = (h->Wp - D) - h->lw;
    h->film_kp = (int)align_up((size_t)std::max(cfg->cond_dim, 1), 32);
    const int mb = cfg->max_batch;
    init_arch(h);
    for (int i = 0; i < 6 && h->train_attn; ++i) {
        const int lv = (i < 3) ? i + 1 : 2 - (i - 3);
        const int L = (h->Hp >> lv) * (h->Wp >> lv);
        if (!attn_train_supported(L, h->sa[i].C, 4)) {
            const int C = h->sa[i].C;
            spdm_destroy(h);
            return fail(SPDM_ERR_INVALID, "SPDM_FLAG_TRAIN_ATTENTION: sa%d has %d tokens of %d channels; the training attention "
                                          "kernels take 1 .. 512 tokens (horizon <= 64)", i + 1, L, C);
        }
    }
    int rc = SPDM_OK;
    do {
        if ((rc = dev_alloc(h, (void**)&h->d_t, sizeof(int) * mb))) break;
        if ((rc = dev_alloc(h, (void**)&h->d_step, sizeof(int) * 4))) break;
        if ((rc = dev_alloc(h, (void**)&h->d_rng, sizeof(unsigned long long) * 2))) break;
        if ((rc = dev_alloc(h, (void**)&h->d_ptrs, sizeof(void*) * 4))) break;
        if (hipMemset(h->d_step, 0, sizeof(int) * 4) != hipSuccess) { rc = fail(SPDM_ERR_HIP, "memset failed"); break; }
        if ((rc = dev_alloc(h, (void**)&h->d_condm, sizeof(float) * (size_t)mb * h->film_kp))) break;
        static const int film_c[6] = {128, 256, 256, 128, 64, 64};
        if (h->simple) rc = dev_alloc(h, (void**)&h->d_cemb, sizeof(float) * (size_t)mb * 6 * SIMPLE_COND_CH);
        for (int i = 0; i < 6 && !rc && !h->simple; ++i) rc = dev_alloc(h, (void**)&h->d_film[i], sizeof(float) * (size_t)mb * 2 * film_c[i]);
        if (rc) break;
        if ((rc = dev_alloc(h, (void**)&h->d_x, sizeof(float) * (size_t)mb * H0 * D))) break;
        if (h->split && !(h->sw & SW_NO_SPLITK) && (rc = dev_alloc(h, (void**)&h->d_partial, SPLITK_WORKSPACE_BYTES))) break;
        // size the arena with a dry run of the plan at max_batch
        h->arena.dry = true;
        h->arena.keep = (cfg->flags & SPDM_FLAG_DEBUG_KEEP) != 0;
        h->arena.reset();
        if ((rc = dry_plan_all(h))) break;
        h->arena.dry = false;
        h->arena.cap = align_up(h->arena.peak, 4096);
        hipError_t e = hipMalloc((void**)&h->arena.base, h->arena.cap);
        if (e != hipSuccess) { rc = fail(SPDM_ERR_NOMEM, "workspace of %zu bytes: %s", h->arena.cap, hipGetErrorString(e)); break; }
        h->owned.push_back(h->arena.base);
        if (h->sw & SW_ARENA_TRACE) fprintf(stderr, "[spdm] arena %p, %zu MiB\n", (void*)h->arena.base, h->arena.cap >> 20);
        if (h->train) {
            h->tws_floats = train_workspace_floats(h);
            if ((rc = dev_alloc(h, (void**)&h->tws, sizeof(float) * h->tws_floats))) break;
        }
    } while (0);
    if (rc) { spdm_destroy(h); return rc; }
    default_time_table(h->time_table, cfg->num_train_timesteps, cfg->time_dim);
    *out = h;
    return SPDM_OK;
}

extern "C" void spdm_destroy(spdm_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    if (h->step_exec) (void)hipGraphExecDestroy(h->step_exec);
    if (h->step_graph) (void)hipGraphDestroy(h->step_graph);
    if (h->gstream) (void)hipStreamDestroy(h->gstream);
    for (void* p : h->owned) (void)hipFree(p);
    for (auto& e : h->prof_evts) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (auto& e : h->prof_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    delete h;
}

extern "C" int32_t spdm_uses_split_precision(const spdm_handle* h) { return (h && h->split) ? 1 : 0; }

extern "C" size_t spdm_device_bytes(const spdm_handle* h) { return h ? h->persistent_bytes + h->wt.bytes + h->arena.cap : 0; }

// -------------------------------------------------------------------------------------------------
// weights
//
// Every kernel-layout copy of a weight is made on the device from the torch-layout blob (weight_layout.hip).  The Recorder
// below is the one place each layout is defined: it records one WeightCopy (a gather, kernels.h) per copy into a WeightTable,
// for the Loader as it walks the network, for the encoder and for the standalone GEMM entry points alike; the table's
// relayout then makes the copies (spdm_load_weights, spdm_update_weights, ...).  A walk runs twice: the plan pass checks every
// name and shape and records the split format's range checks; once the device has answered them, the load pass allocates
// the copies -- a tensor outside the range gets no split copy -- and records them (both_passes).  A table with no split
// copies needs the load pass only (plan = false).
static char g_plan_only;                   // the plan pass's stand-in for a copy it does not allocate

struct Recorder {
    WeightTable& wt;
    size_t n;                              // floats of the blob
    std::map<std::string, const spdm_tensor_index*> idx;
    int err = SPDM_OK;
    bool plan = true;
    std::map<std::string, int> slot_of;    // range slot of each tensor name (the stacked cond_emb_layer is one name)
    std::vector<long long> plan_tabs;      // the plan pass's offset tables: the load pass must build the same
    std::set<std::string> demoted;         // tensors outside the split format's range (once each, however many copies they lose)
    Recorder(WeightTable& table, size_t blob_floats, const spdm_tensor_index* index = nullptr, int n_index = 0)
        : wt(table), n(blob_floats) {
        for (int i = 0; i < n_index; ++i) {
            char name[SPDM_NAME_MAX + 1];
            memcpy(name, index[i].name, SPDM_NAME_MAX);
            name[SPDM_NAME_MAX] = 0;
            idx[name] = &index[i];
        }
    }
    long long at(const std::string& name, const std::vector<int>& shape) {
        auto it = idx.find(name);
        if (it == idx.end()) { err = fail(SPDM_ERR_MISSING, "tensor '%s' not in the index", name.c_str()); return -1; }
        const spdm_tensor_index* e = it->second;
        size_t numel = 1;
        int d = 0;
        for (int sdim : shape) {
            if (d >= e->ndim || e->shape[d] != sdim) { err = fail(SPDM_ERR_INVALID, "tensor '%s': unexpected shape", name.c_str()); return -1; }
            numel *= (size_t)sdim;
            ++d;
        }
        if (d != e->ndim || numel != e->numel || e->offset + e->numel > n) { err = fail(SPDM_ERR_INVALID, "tensor '%s': bad extent", name.c_str()); return -1; }
        return (long long)e->offset;
    }
    // ---- the gathers ----
    // dense [n0][n1][n2] read row-major from src
    static WeightCopy dense(long long src, int n0, int n1, int n2) {
        WeightCopy c;
        c.src = src;
        c.n[0] = c.lim[0] = n0; c.n[1] = c.lim[1] = n1; c.n[2] = c.lim[2] = n2;
        c.stride[0] = (long long)n1 * n2; c.stride[1] = n2; c.stride[2] = 1;
        return c;
    }
    // axis 0 = the taps of a (Cout, Cin, 3, 3) tensor: taps == 3 keeps only the centre column (W == 1 levels, where the left /
    // right taps only ever see zero padding); flipped = rotated 180 degrees (the data gradient's convolution)
    static void tap_axis(WeightCopy& c, int taps, bool flipped) {
        c.n[0] = c.lim[0] = taps;
        if (taps == 9) { c.src += flipped ? 8 : 0; c.stride[0] = flipped ? -1 : 1; }
        else { c.src += flipped ? 7 : 1; c.stride[0] = flipped ? -3 : 3; }
    }
    // (Cout, Cin, 3, 3) at src as [taps][Cout][Cin]
    static WeightCopy conv_taps(long long src, int cout, int cin, int taps) {
        WeightCopy v = dense(src, taps, cout, cin);
        v.stride[1] = (long long)cin * 9; v.stride[2] = 9;
        tap_axis(v, taps, false);
        return v;
    }
    int table(const std::vector<long long>& tab) {
        const int at = (int)wt.tabs.size();
        wt.tabs.insert(wt.tabs.end(), tab.begin(), tab.end());
        return at;
    }
    // storage position -> source step of its real channel (ChanMap), -1 for a padding lane
    int map_table(const ChanMap& m, long long stride) {
        std::vector<long long> tab(m.width, -1);
        for (int i = 0; i < m.real(); ++i) tab[m.pos[i]] = (long long)i * stride;
        return table(tab);
    }
    // every element the copy can read lies inside the blob
    bool inside(const WeightCopy& c) const {
        long long lo = c.src, hi = c.src;
        for (int k = 0; k < 3; ++k) {
            if (c.tab[k] >= 0) {
                long long tmin = LLONG_MAX, tmax = LLONG_MIN;
                for (int i = 0; i < c.n[k]; ++i) {
                    const long long v = wt.tabs[c.tab[k] + i];
                    if (v >= 0) { tmin = std::min(tmin, v); tmax = std::max(tmax, v); }
                }
                if (tmin == LLONG_MAX) continue;
                lo += tmin; hi += tmax;
            } else {
                const long long span = (long long)(std::min(c.lim[k], c.n[k]) - 1) * c.stride[k];
                if (span < 0) lo += span; else hi += span;
            }
        }
        return lo >= 0 && hi < (long long)n;
    }
    void* put(WeightCopy c, int fmt) {
        c.fmt = fmt;
        c.count = (long long)c.n[0] * c.n[1] * c.n[2];
        if (fmt == WL_PERM_HI || fmt == WL_PERM_LO) c.count /= 2;          // fp16 halves
        if (plan) return &g_plan_only;
        if (!inside(c)) { err = fail(SPDM_ERR_INVALID, "weight copy reads outside the blob"); return nullptr; }
        if (wt.alloc(&c.dst, (size_t)c.count * sizeof(float)) != SPDM_OK) { err = SPDM_ERR_HIP; return nullptr; }
        wt.copies.push_back(c);
        return c.dst;
    }
    float* f32(const WeightCopy& c) { return (float*)put(c, WL_F32); }
    // fragment-order split copy (WL_FRAG, weight_layout.hip) of the logical [taps][N][K] array
    float* frag(WeightCopy c, int taps, int N, int K) {
        c.taps = taps; c.N = N; c.K = K;
        return (float*)put(c, WL_FRAG);
    }
    // The split format scales weights by 2^7 before the fp16 cast: |w| >= 511.75 would become inf.  Such a tensor gets no
    // split copy and its layer runs on the exact fp32 kernel instead (same results, 5x slower for that layer).  Plan pass:
    // queue the check of this copy's logical array under the tensor's name; load pass: the device's verdict.
    bool in_range(WeightCopy c, const std::string& name) {
        auto it = slot_of.find(name);
        int s = 0;
        if (it == slot_of.end()) { s = (int)wt.slots.size(); slot_of[name] = s; wt.slots.push_back(name); }
        else s = it->second;
        if (plan) {
            c.fmt = WL_RANGE; c.slot = s; c.count = (long long)c.n[0] * c.n[1] * c.n[2];
            if (!inside(c)) { err = fail(SPDM_ERR_INVALID, "weight copy reads outside the blob"); return false; }
            wt.ranges.push_back(c);
            return true;
        }
        if (wt.oor[s]) { demoted.insert(name); return false; }
        return true;
    }
    // fp32 [rows][K] -> per 32-k chunk [32 x fp16 hi | 32 x fp16 lo] of x' = 128 x (conv_gemm.hip, PREC_SPLIT)
    float* split(const WeightCopy& c, int K, const std::string& name) {
        if (K % 32 != 0) { err = fail(SPDM_ERR_INVALID, "split weights need K %% 32 == 0"); return nullptr; }
        if (!in_range(c, name)) return nullptr;
        return (float*)put(c, WL_SPLIT);
    }
    // (out, in) at src -> [in][out]: the weights of a Linear layer's data gradient (dx = dy W)
    float* transposed(long long src, int out, int in) {
        if (src < 0) return nullptr;
        WeightCopy c = dense(src, 1, in, out);
        c.stride[1] = 1; c.stride[2] = in;
        return f32(c);
    }
    // (out, 64) fp32 -> two fp16 arrays (hi, lo of 128 x) of [out][64] in MFMA A-fragment order, input axis permuted inside each
    // group of 16 by perm16 = 0 1 2 3 8 9 10 11 | 4 5 6 7 12 13 14 15: the k-slot order of an accumulator tile used as B operand
    // (sa_fused.hip)
    void perm_split(const std::string& wname, int out, void** hi_dev, void** lo_dev) {
        const long long o = at(wname, {out, 64});
        if (o < 0) return;
        const WeightCopy v = dense(o, 1, out, 64);
        if (!in_range(v, wname)) return;        // block falls back to the GEMM chain
        *hi_dev = put(v, WL_PERM_HI);
        *lo_dev = put(v, WL_PERM_LO);
    }
    // fragment-order split copy of a (out, in) Linear weight (sa_tail.hip reads its B operands straight from it)
    float* linear_frag(const std::string& wname, int out, int in) {
        const long long o = at(wname, {out, in});
        if (o < 0) return nullptr;
        const WeightCopy v = dense(o, 1, out, in);
        if (!in_range(v, wname)) return nullptr;
        return frag(v, 1, out, in);
    }
    // walk() records through this Recorder and returns err.  Plan pass; the device answers the range checks on the blob; load pass
    template <class Walk>
    int both_passes(const float* d_blob, Walk walk) {
        SPDM_TRY(walk());
        SPDM_TRY(wt.upload(true));
        SPDM_TRY(wt.check_ranges(d_blob, nullptr, &wt.oor));
        plan_tabs.swap(wt.tabs);
        plan = false;
        SPDM_TRY(walk());
        return finish(d_blob);
    }
    // after the load pass: the recorded copies on the device, made from the blob
    int finish(const float* d_blob) {
        SPDM_TRY(err);
        if (wt.tabs != plan_tabs) return fail(SPDM_ERR_INVALID, "weight layout tables differ between the loader's passes");
        SPDM_TRY(wt.upload(false));
        SPDM_TRY(wt.relayout(d_blob, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        return SPDM_OK;
    }
};

// The model walkers: the one part of weight loading that reads the handle's configuration (h->train*, h->cfg, h->film_kp)
struct Loader : Recorder {
    spdm_handle* h;
    const float* blob;                     // host blob (spdm_load_weights): the few values the host itself keeps
    Loader(spdm_handle* handle, const float* host_blob, size_t blob_floats, const spdm_tensor_index* index, int n_index)
        : Recorder(handle->wt, blob_floats, index, n_index), h(handle), blob(host_blob) {}
    // (Cout,Cin,3,3) -> w [taps][Cout][Cin], its split and fragment-order copies, and (SPDM_FLAG_TRAIN) wt [taps][Cin][Cout]
    // with the taps rotated 180 degrees: the weights of the convolution that takes the output gradient to the input gradient
    ConvW conv(const std::string& name, int cout, int cin, int taps) {
        ConvW c;
        const long long o = at(name, {cout, cin, 3, 3});
        if (o < 0) return c;
        const WeightCopy v = conv_taps(o, cout, cin, taps);
        c.w = f32(v);
        if (h->train) {
            WeightCopy t = dense(o, taps, cin, cout);
            t.stride[1] = 9; t.stride[2] = (long long)cin * 9;
            tap_axis(t, taps, true);
            c.wt = f32(t);
        }
        c.ws = (cin % 32 == 0) ? split(v, cin, name) : nullptr;
        if (c.ws && cout % 64 == 0) c.wf = frag(v, taps, cout, cin);
        c.taps = taps; c.cin = cin; c.cout = cout;
        return c;
    }
    float* vec(const std::string& name, int nelem) {
        const long long o = at(name, {nelem});
        return o < 0 ? nullptr : f32(dense(o, 1, 1, nelem));
    }
    // (out, in) -> [out][in_pad], zero columns beyond in
    LinW linear(const std::string& wname, const std::string& bname, int out, int in, int in_pad) {
        LinW l;
        const long long o = at(wname, {out, in});
        if (o < 0) return l;
        WeightCopy v = dense(o, 1, out, in_pad);
        v.stride[1] = in; v.lim[2] = in;
        l.w = f32(v);
        l.ws = (in_pad % 32 == 0) ? split(v, in_pad, wname) : nullptr;
        l.b = vec(bname, out);
        l.in = in_pad; l.out = out;
        return l;
    }
    DoubleConvW dconv(const std::string& p, int cin, int cout, int taps) {
        DoubleConvW d;
        d.first = conv(p + ".first.weight", cout, cin, taps);
        d.second = conv(p + ".second.weight", cout, cout, taps);
        d.gamma = vec(p + ".norm.weight", cout);
        d.beta = vec(p + ".norm.bias", cout);
        return d;
    }
    ResampleW resample(const std::string& p, int cin, int cout, int taps) {
        ResampleW r;
        r.dc1 = dconv(p + ".doubleConv1", cin, cin, taps);
        r.dc2 = dconv(p + ".doubleConv2", cin, cout, taps);
        r.emb = linear(p + ".emb_layer.1.weight", p + ".emb_layer.1.bias", cout, h->cfg.time_dim, h->cfg.time_dim);
        if (h->cfg.cond_dim > 0) {
            r.film = linear(p + ".cond_encoder.2.weight", p + ".cond_encoder.2.bias", 2 * cout, h->cfg.cond_dim, h->film_kp);
            if (h->train) {      // (2 cout, cond_dim) -> [cond_dim padded to 64][2 cout]: the FiLM encoder's data gradient
                const int cd = h->cfg.cond_dim;
                const long long o = at(p + ".cond_encoder.2.weight", {2 * cout, cd});
                if (o >= 0) {
                    WeightCopy t = dense(o, 1, (int)align_up(cd, 64), 2 * cout);
                    t.stride[1] = 1; t.lim[1] = cd; t.stride[2] = cd;
                    r.film.wt = f32(t);
                }
            }
        }
        r.cout = cout;
        return r;
    }
    // ---- models/simple_Unet.py: re-layout into channel-padded storage (ChanMap) ----
    // (Cout, Cin, 3, 3) -> [taps][mo.width][mi.width], real (o, i) at (mo.pos[o], mi.pos[i]), zeros elsewhere
    ConvW conv_mapped(const std::string& name, const ChanMap& mo, const ChanMap& mi, int taps) {
        ConvW c;
        const int co = mo.real(), ci = mi.real(), N = mo.width, K = mi.width;
        const long long o = at(name, {co, ci, 3, 3});
        if (o < 0) return c;
        WeightCopy v = dense(o, taps, N, K);
        tap_axis(v, taps, false);
        v.tab[1] = map_table(mo, (long long)ci * 9);
        v.tab[2] = map_table(mi, 9);
        c.w = f32(v);
        c.ws = split(v, K, name);
        if (c.ws) c.wf = frag(v, taps, N, K);
        if (h->train_simple) {     // [taps][K][N], taps rotated 180 degrees (conv_taps_flipped at the padded widths)
            WeightCopy t = dense(o, taps, K, N);
            tap_axis(t, taps, true);
            t.tab[1] = map_table(mi, 9);
            t.tab[2] = map_table(mo, (long long)ci * 9);
            c.wt = f32(t);
        }
        c.taps = taps; c.cin = K; c.cout = N; c.cnorm = co;
        return c;
    }
    float* vec_mapped(const std::string& name, const ChanMap& m) {
        const long long o = at(name, {m.real()});
        if (o < 0) return nullptr;
        WeightCopy v = dense(o, 1, 1, m.width);
        v.tab[2] = map_table(m, 1);
        return f32(v);
    }
    // DoubleConvolution (simple_Unet.py:92-104): ONE GroupNorm module serves both convolutions
    DoubleConvW dconv_mapped(const std::string& p, const ChanMap& mi, const ChanMap& mo, int taps) {
        DoubleConvW d;
        d.first = conv_mapped(p + ".first.weight", mo, mi, taps);
        d.second = conv_mapped(p + ".second.weight", mo, mo, taps);
        d.gamma = vec_mapped(p + ".norm.weight", mo);
        d.beta = vec_mapped(p + ".norm.bias", mo);
        return d;
    }
    // Linear (out, in) with its output rows padded to out_pad (zero rows, zero bias)
    LinW linear_pad_out(const std::string& wname, const std::string& bname, int out, int in, int out_pad) {
        LinW l;
        const long long w = at(wname, {out, in});
        const long long b = at(bname, {out});
        if (w < 0 || b < 0) return l;
        WeightCopy v = dense(w, 1, out_pad, in);
        v.lim[1] = out;
        l.w = f32(v);
        l.ws = (in % 32 == 0) ? split(v, in, wname) : nullptr;
        WeightCopy bv = dense(b, 1, 1, out_pad);
        bv.lim[2] = out;
        l.b = f32(bv);
        l.in = in; l.out = out_pad;
        return l;
    }
    AttnW attn(const std::string& p, int C) {
        AttnW a;
        a.C = C;
        if (C == 128 || C == 256) {
            a.tail_wf[0] = linear_frag(p + ".attention.out_proj.weight", C, C);
            a.tail_wf[1] = linear_frag(p + ".ff_self.1.weight", C, C);
            a.tail_wf[2] = linear_frag(p + ".ff_self.3.weight", C, C);
            a.qkv_wf = linear_frag(p + ".attention.in_proj_weight", 3 * C, C);
        }
        if (C == 64) {
            perm_split(p + ".attention.in_proj_weight", 192, &a.fw[0], &a.fw[1]);
            perm_split(p + ".attention.out_proj.weight", 64, &a.fw[2], &a.fw[3]);
            perm_split(p + ".ff_self.1.weight", 64, &a.fw[4], &a.fw[5]);
            perm_split(p + ".ff_self.3.weight", 64, &a.fw[6], &a.fw[7]);
            for (int k = 0; k < 8; ++k)
                if (!a.fw[k]) { a.fw[0] = nullptr; break; }        // the fused kernel needs all four matrices
        }
        if ((C == 128 || C == 256) && !(a.tail_wf[0] && a.tail_wf[1] && a.tail_wf[2])) a.tail_wf[0] = nullptr;
        a.in_proj = linear(p + ".attention.in_proj_weight", p + ".attention.in_proj_bias", 3 * C, C, C);
        a.out_proj = linear(p + ".attention.out_proj.weight", p + ".attention.out_proj.bias", C, C, C);
        a.ln_g = vec(p + ".ln.weight", C);
        a.ln_b = vec(p + ".ln.bias", C);
        a.ff_ln_g = vec(p + ".ff_self.0.weight", C);
        a.ff_ln_b = vec(p + ".ff_self.0.bias", C);
        a.ff1 = linear(p + ".ff_self.1.weight", p + ".ff_self.1.bias", C, C, C);
        a.ff2 = linear(p + ".ff_self.3.weight", p + ".ff_self.3.bias", C, C, C);
        if (h->train_attn) {
            a.in_proj.wt = transposed(at(p + ".attention.in_proj_weight", {3 * C, C}), 3 * C, C);
            a.out_proj.wt = transposed(at(p + ".attention.out_proj.weight", {C, C}), C, C);
            a.ff1.wt = transposed(at(p + ".ff_self.1.weight", {C, C}), C, C);
            a.ff2.wt = transposed(at(p + ".ff_self.3.weight", {C, C}), C, C);
        }
        return a;
    }
    // first conv (cout, 1, 3, 3) -> [9][64] (conv_in_kernel's layout; output lanes cout..63 zero)
    float* conv_in(const std::string& name, int cout) {
        const long long o = at(name, {cout, 1, 3, 3});
        if (o < 0) return nullptr;
        WeightCopy v = dense(o, 1, 9, 64);
        v.stride[1] = 1; v.stride[2] = 9; v.lim[2] = cout;
        return f32(v);
    }
    // outc: Conv2d(64, 1, 1) with bias -- its bias is a host scalar of the handle (the step kernel's argument)
    void outc() {
        h->outc_w = nullptr;
        const long long w = at("outc.weight", {1, 64, 1, 1});
        const long long b = at("outc.bias", {1});
        if (w < 0 || b < 0) return;
        h->outc_w = f32(dense(w, 1, 1, 64));
        h->outc_b = blob[b];
        wt.scalar_off = b;
    }
};

// dry run of the plan at max_batch with the handle's current kernel selection; grows the slab if this plan needs more
static int replan_arena(spdm_handle* h) {
    (void)hipDeviceSynchronize();         // nothing may still be running in the slab about to be re-planned
    const bool keep = h->arena.keep;
    h->arena.dry = true;
    const int rc = dry_plan_all(h);
    h->arena.dry = false;
    h->arena.keep = keep;
    if (rc != SPDM_OK) return rc;
    if (align_up(h->arena.peak, 4096) > h->arena.cap) {
        char* nb = nullptr;
        const size_t cap = align_up(h->arena.peak, 4096);
        hipError_t e = hipMalloc((void**)&nb, cap);
        if (e != hipSuccess) return fail(SPDM_ERR_NOMEM, "workspace of %zu bytes: %s", cap, hipGetErrorString(e));
        h->owned.push_back(nb);        // (the smaller slab stays owned until destroy)
        h->arena.base = nb;
        h->arena.cap = cap;
    }
    return SPDM_OK;
}

// UNet.state_dict() of models/simple_Unet.py (SPDM_FLAG_SIMPLE_UNET) into channel-padded storage; Loader::err carries failures
static int load_simple(spdm_handle* h, Loader& L, int t3) {
    const ChanMap c16 = ChanMap::ident(16);
    h->w_inc_first = L.conv_in("input_conv.first.weight", 16);
    h->inc.second = L.conv_mapped("input_conv.second.weight", c16, c16, 9);
    h->inc.gamma = L.vec_mapped("input_conv.norm.weight", c16);
    h->inc.beta = L.vec_mapped("input_conv.norm.bias", c16);
    static const char* names[6] = {"down1", "down2", "down3", "up1", "up2", "up3"};
    const int Kp = h->film_kp, cd = h->cfg.cond_dim, td = h->cfg.time_dim;
    std::vector<long long> cw_off(6, -1), cb_off(6, -1);
    for (int k = 0; k < 6; ++k) {
        const std::string p = names[k];
        ResampleW& r = simple_block(h, k);
        const ChanMap in = simple_in_map(k), out = ChanMap::ident(kSimpleBlocks[k].cout);
        const int taps = (k == 2) ? t3 : 9;
        r.dc1 = L.dconv_mapped(p + ".doubleConv1", in, in, taps);
        r.dc2 = L.dconv_mapped(p + ".doubleConv2", in, out, taps);
        r.emb = L.linear_pad_out(p + ".emb_layer.1.weight", p + ".emb_layer.1.bias", out.real(), td, out.width);
        r.cout = out.real();
        cw_off[k] = L.at(p + ".cond_emb_layer.1.weight", {SIMPLE_COND_CH, cd});
        cb_off[k] = L.at(p + ".cond_emb_layer.1.bias", {SIMPLE_COND_CH});
    }
    if (L.err != SPDM_OK) return L.err;
    {   // the six cond_emb_layer Linears stacked: w [6 x 32][Kp] (columns beyond cond_dim zero), b [6 x 32]
        WeightCopy cw = Recorder::dense(0, 6, SIMPLE_COND_CH, Kp);
        cw.tab[0] = L.table(cw_off);
        cw.stride[1] = cd; cw.lim[2] = cd;
        WeightCopy cb = Recorder::dense(0, 1, 6, SIMPLE_COND_CH);
        cb.tab[1] = L.table(cb_off);
        h->cemb.w = L.f32(cw);
        h->cemb.ws = L.split(cw, Kp, "cond_emb_layer");
        h->cemb.b = L.f32(cb);
        h->cemb.in = Kp; h->cemb.out = 6 * SIMPLE_COND_CH;
        if (h->train_simple) {
            // d SiLU(cond) = dcemb [B][6 x 32] . W_stacked: the transposed copy [cond_dim padded to 64][6 x 32] (the GEMM's N % 64)
            WeightCopy t = Recorder::dense(0, (int)align_up((size_t)cd, 64), 6, SIMPLE_COND_CH);
            t.stride[0] = 1; t.lim[0] = cd;
            t.tab[1] = L.table(cw_off);
            t.stride[2] = cd;
            h->cemb.wt = L.f32(t);
        }
    }
    if (h->train_simple && !L.plan) {
        // the channel maps the backward pass gathers through (GroupNorm lanes, weight-gradient write-out)
        auto upload_map = [&](const ChanMap& m) -> int* {
            void* p = nullptr;
            if (dev_alloc(h, &p, sizeof(int) * m.pos.size()) != SPDM_OK) { L.err = SPDM_ERR_HIP; return nullptr; }
            if (hipMemcpy(p, m.pos.data(), sizeof(int) * m.pos.size(), hipMemcpyHostToDevice) != hipSuccess) {
                L.err = fail(SPDM_ERR_HIP, "channel map upload failed");
                return nullptr;
            }
            return (int*)p;
        };
        h->d_pos16 = upload_map(c16);
        for (int k = 0; k < 6; ++k) {
            h->d_pos_in[k] = upload_map(simple_in_map(k));
            h->d_pos_out[k] = upload_map(ChanMap::ident(kSimpleBlocks[k].cout));
        }
        if (dev_alloc(h, (void**)&h->d_time_pe, sizeof(float) * (size_t)h->cfg.num_train_timesteps * td) != SPDM_OK) L.err = SPDM_ERR_HIP;
    }
    L.outc();      // Conv2d(64, out, 1) with bias (simple_Unet.py:280); the 64 channels are up3's 32 + 32, unpadded
    if (L.err != SPDM_OK) return L.err;
    // pos_encoding.pos_encoding (noise_steps + 1, time_dim): the sin/cos-interleaved table of PositionalEncoding (:226-257)
    // IS the time table of this network (spdm_update_weights does not read this slot)
    auto it = L.idx.find("pos_encoding.pos_encoding");
    if (it == L.idx.end()) return fail(SPDM_ERR_MISSING, "tensor 'pos_encoding.pos_encoding' not in the index");
    const spdm_tensor_index* e = it->second;
    if (e->ndim != 2 || e->shape[1] != td || e->shape[0] != h->cfg.num_train_timesteps)
        return fail(SPDM_ERR_INVALID, "pos_encoding.pos_encoding is (%d, %d): the handle needs (num_train_timesteps = %d, time_dim = %d) "
                    "-- create it with num_train_timesteps equal to the buffer's row count", e->shape[0], e->ndim > 1 ? e->shape[1] : 0,
                    h->cfg.num_train_timesteps, td);
    const long long pe = L.at("pos_encoding.pos_encoding", {h->cfg.num_train_timesteps, td});
    if (pe < 0) return L.err;
    h->time_table.assign(L.blob + pe, L.blob + pe + (size_t)h->cfg.num_train_timesteps * td);
    return SPDM_OK;
}

// UNet_Film / UNet_Film_noAttention state_dict
static int load_film(spdm_handle* h, Loader& L, int t3) {
    h->w_inc_first = L.conv_in("inc.first.weight", 64);
    h->inc.second = L.conv("inc.second.weight", 64, 64, 9);
    h->inc.gamma = L.vec("inc.norm.weight", 64);
    h->inc.beta = L.vec("inc.norm.bias", 64);
    h->down[0] = L.resample("down1", 64, 128, 9);
    h->down[1] = L.resample("down2", 128, 256, 9);
    h->down[2] = L.resample("down3", 256, 256, t3);
    h->bot[0] = L.dconv("bot1", 256, 512, t3);
    h->bot[1] = L.dconv("bot2", 512, 512, t3);
    h->bot[2] = L.dconv("bot3", 512, 256, t3);
    h->up[0] = L.resample("up1", 512, 128, 9);
    h->up[1] = L.resample("up2", 256, 64, 9);
    h->up[2] = L.resample("up3", 128, 64, 9);
    if (h->cfg.attention) {
        static const int sc[6] = {128, 256, 256, 128, 64, 64};
        for (int i = 0; i < 6; ++i) h->sa[i] = L.attn("sa" + std::to_string(i + 1), sc[i]);
    }
    L.outc();
    return L.err;
}

extern "C" int spdm_load_weights(spdm_handle* h, const float* blob, size_t n, const spdm_tensor_index* index,
                                 int32_t n_index) {
    if (!h || !blob || !index || n_index <= 0) return fail(SPDM_ERR_INVALID, "null argument");
    if (h->weights_loaded) return fail(SPDM_ERR_STATE, "weights already loaded on this handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    Loader L(h, blob, n, index, n_index);
    // level-3 maps are (Hp/8) x 1: a 3x3 kernel only ever multiplies its centre column there
    const int t3 = (h->Wp >> 3) == 1 ? 3 : 9;
    auto walk = [&]() { return h->simple ? load_simple(h, L, t3) : load_film(h, L, t3); };
    DevBlob db;                            // the blob on the device, once; the range checks run on it
    int rc = db.upload(blob, n);
    if (rc == SPDM_OK) rc = L.both_passes(db.p, walk);
    if (rc != SPDM_OK) { h->wt.clear(); return rc; }      // (a corrected blob may be loaded into this handle)
    h->demoted = (int)L.demoted.size();
    h->blob_floats = n;
    if (h->train) {
        h->grad_off.clear();
        h->grad_floats = n;
        for (const auto& kv : L.idx) h->grad_off[kv.first] = (size_t)kv.second->offset;
    }
    // time-embedding tables (one per resample block), filled lazily on the first evaluation
    ResampleW* blocks[6] = {&h->down[0], &h->down[1], &h->down[2], &h->up[0], &h->up[1], &h->up[2]};
    for (ResampleW* r : blocks)
        SPDM_TRY(dev_alloc(h, (void**)&r->temb_table, sizeof(float) * (size_t)h->cfg.num_train_timesteps * r->emb.out));
    SPDM_TRY(dev_alloc(h, (void**)&h->d_time_silu, sizeof(float) * (size_t)h->cfg.num_train_timesteps * h->cfg.time_dim));
    h->weights_loaded = true;
    h->temb_ready = false;
    if (h->demoted > 0) {
        // Some layers left the kernels the workspace was sized for (create() planned by shape only): plan again with the
        // weights known and grow the slab if this plan needs more.
        SPDM_TRY(replan_arena(h));
    }
    return SPDM_OK;
}

extern "C" int spdm_update_weights(spdm_handle* h, const float* d_blob, size_t n, void* stream) {
    if (!h || !d_blob) return fail(SPDM_ERR_INVALID, "null argument");
    if (!h->weights_loaded) return fail(SPDM_ERR_STATE, "spdm_load_weights has not been called");
    if (n != h->blob_floats) return fail(SPDM_ERR_INVALID, "blob has %zu floats; the loaded one had %zu", n, h->blob_floats);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> oor;
    float ob = 0.f;
    SPDM_TRY(h->wt.check_ranges(d_blob, s, &oor, &ob));
    for (size_t i = 0; i < oor.size(); ++i)
        if ((oor[i] != 0) != (h->wt.oor[i] != 0))
            return fail(SPDM_ERR_STATE, "tensor '%s' %s the split format's range (|w| < 511): the workspace plan follows the set of "
                        "such tensors -- load these weights into a new handle", h->wt.slots[i].c_str(), oor[i] ? "left" : "came back into");
    SPDM_TRY(h->wt.relayout(d_blob, s));
    h->temb_ready = false;                 // the time-embedding tables and a session's FiLM / cond_emb projections are
    h->session = false;                    // functions of the old weights
    uint32_t a, b;
    memcpy(&a, &ob, 4);
    memcpy(&b, &h->outc_b, 4);
    if (a != b) {
        // outc's bias is an argument the captured step graph baked in (StepArgs::bias, SaCrop::outc_b): capture again next time
        h->outc_b = ob;
        if (h->step_exec || h->step_graph) {
            HIP_TRY(hipDeviceSynchronize());
            if (h->step_exec) (void)hipGraphExecDestroy(h->step_exec);
            if (h->step_graph) (void)hipGraphDestroy(h->step_graph);
            h->step_exec = nullptr;
            h->step_graph = nullptr;
        }
    }
    return SPDM_OK;
}

extern "C" int spdm_debug_weight_digest(const spdm_handle* h, uint64_t* out) {
    if (!h || !out) return fail(SPDM_ERR_INVALID, "null argument");
    if (!h->weights_loaded) return fail(SPDM_ERR_STATE, "spdm_load_weights has not been called");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    uint64_t x = 1469598103934665603ull;          // FNV-1a over 64-bit words
    auto mix = [&](const void* p, size_t bytes) {
        const unsigned char* c = (const unsigned char*)p;
        size_t i = 0;
        for (; i + 8 <= bytes; i += 8) { uint64_t w; memcpy(&w, c + i, 8); x = (x ^ w) * 1099511628211ull; }
        for (; i < bytes; ++i) x = (x ^ c[i]) * 1099511628211ull;
    };
    std::vector<unsigned char> buf;
    for (const WeightCopy& c : h->wt.copies) {
        buf.resize((size_t)c.count * sizeof(float));
        HIP_TRY(hipMemcpy(buf.data(), c.dst, buf.size(), hipMemcpyDeviceToHost));
        mix(buf.data(), buf.size());
    }
    mix(&h->outc_b, sizeof(float));
    for (size_t i = 0; i < h->wt.slots.size(); ++i)
        if (h->wt.oor[i]) mix(h->wt.slots[i].data(), h->wt.slots[i].size() + 1);
    *out = x;
    return SPDM_OK;
}

extern "C" int32_t spdm_demoted_tensors(const spdm_handle* h) { return h ? h->demoted : 0; }

extern "C" int spdm_set_switch(spdm_handle* h, const char* name, int32_t on) {
    if (!h || !name) return fail(SPDM_ERR_INVALID, "null argument");
    int n = 0;
    const SwitchName* t = switch_table(&n);
    for (int i = 0; i < n; ++i)
        if (strcmp(t[i].env, name) == 0) {
            h->sw = on ? (h->sw | t[i].bit) : (h->sw & ~t[i].bit);
            HIP_TRY(hipSetDevice(h->cfg.device));
            return replan_arena(h);      // the arena was sized for the previous selection (the unfused fallbacks allocate more)
        }
    return fail(SPDM_ERR_INVALID, "unknown switch '%s'", name);
}

extern "C" int spdm_set_time_table(spdm_handle* h, const float* tab, int32_t T) {
    if (!h || !tab) return fail(SPDM_ERR_INVALID, "null argument");
    if (T != h->cfg.num_train_timesteps) return fail(SPDM_ERR_INVALID, "time table has %d rows, handle was created for %d", T, h->cfg.num_train_timesteps);
    h->time_table.assign(tab, tab + (size_t)T * h->cfg.time_dim);
    h->temb_ready = false;
    return SPDM_OK;
}

static int install_schedule(spdm_handle* h, int kind, int n, const int* ts, const float* coef) {
    HIP_TRY(hipSetDevice(h->cfg.device));
    for (int i = 0; i < n; ++i)
        if (ts[i] < 0 || ts[i] >= h->cfg.num_train_timesteps)
            return fail(SPDM_ERR_INVALID, "timestep %d outside the handle's time table [0,%d)", ts[i], h->cfg.num_train_timesteps);
    if (n > h->n_steps || !h->d_coef) {
        SPDM_TRY(dev_alloc(h, (void**)&h->d_timesteps, sizeof(int) * n));
        SPDM_TRY(dev_alloc(h, (void**)&h->d_coef, sizeof(float) * 6 * n));
    }
    if (kind == SPDM_DPMPP_2M && !h->d_x0_prev) {
        const size_t nx = (size_t)h->cfg.max_batch * h->cfg.horizon * h->cfg.state_dim;
        SPDM_TRY(dev_alloc(h, (void**)&h->d_x0_prev, sizeof(float) * nx));
        SPDM_TRY(dev_alloc(h, (void**)&h->d_solver_eps, sizeof(float) * nx));
        SPDM_TRY(dev_alloc(h, (void**)&h->d_first, sizeof(int)));
    }
    HIP_TRY(hipMemcpy(h->d_timesteps, ts, sizeof(int) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->d_coef, coef, sizeof(float) * 6 * n, hipMemcpyHostToDevice));
    h->timesteps.assign(ts, ts + n);
    h->n_steps = n;
    h->sched_kind = kind;
    h->session = false;
    return SPDM_OK;
}

extern "C" int spdm_set_schedule(spdm_handle* h, int32_t kind, int32_t T, int32_t n, float b0, float b1) {
    if (!h) return fail(SPDM_ERR_INVALID, "null handle");
    if (T > h->cfg.num_train_timesteps) return fail(SPDM_ERR_INVALID, "T = %d exceeds the handle's time table (%d)", T, h->cfg.num_train_timesteps);
    std::vector<int> ts(std::max(n, 1));
    std::vector<float> coef((size_t)std::max(n, 1) * 6);
    SPDM_TRY(build_schedule(kind, T, n, b0, b1, ts.data(), coef.data()));
    return install_schedule(h, kind, n, ts.data(), coef.data());
}

extern "C" int spdm_set_schedule_tables(spdm_handle* h, int32_t kind, int32_t n, const int32_t* ts, const float* coef) {
    if (!h || !ts || !coef || n < 1) return fail(SPDM_ERR_INVALID, "bad argument");
    if (kind != SPDM_DDPM && kind != SPDM_DDIM && kind != SPDM_DPMPP_2M) return fail(SPDM_ERR_INVALID, "unknown scheduler kind %d", kind);
    return install_schedule(h, kind, n, ts, coef);
}

// -------------------------------------------------------------------------------------------------
// The arguments of one implicit-GEMM launch (launch_gemm): the one place where a layer becomes a launch.  The plan's
// convolutions (Ctx::conv_args) and Linear layers (linear_args), the time-embedding, FiLM and encoder Linears, spdm_bench_gemm
// and spdm_op_gemm all build their launches here.
//   M rows of N outputs from K input channels per tap, H x W maps (1 x 1: a Linear layer); geom_M > 0: choose the kernel as for
//   that many rows (GemmArgs::geom_M); partial: the split-K slabs (null: no split-K).
//   src: the input (leading dimension src.C) with its pending GroupNorm or LayerNorm (src.st.p null: none) for prologue `pro`.
//   skip (skip.x null: none): input channels [up_C, K) -- the skip half of PRO_UPCAT, which carries its own pending GroupNorm,
//   or of a two-source input, whose prologue is the skip's pending GroupNorm (src, the upsampled half, is finished).
static GemmArgs gemm_args(int M, int geom_M, int H, int W, int K, int N, int taps, int split, unsigned sw, float* partial,
                          int pro, const AffineSrc& src, int up_C, const AffineSrc& skip, const float* wgt, const float* wgt_frag,
                          float* dst, int dst_ld, int epi, double* epi_stats, const float* bias = nullptr,
                          const float* resid = nullptr, int resid_ld = 0, double* row_stats = nullptr) {
    GemmArgs a{};
    a.M = M; a.geom_M = geom_M; a.H = H; a.W = W; a.HW = H * W; a.K = K; a.N = N; a.taps = taps;
    a.split = split; a.sw = sw; a.partial = partial;
    a.src = src.x; a.src_ld = src.C; a.wgt = wgt; a.wgt_frag = wgt_frag;
    a.pro = pro;
    const AffineSrc& pending = (skip.x && pro != PRO_UPCAT) ? skip : src;
    if (pending.st.p) { a.pro_stats = pending.st; a.pro_gamma = pending.gamma; a.pro_beta = pending.beta; }
    if (skip.x) {
        a.up_C = up_C; a.skip = skip.x; a.skip_ld = skip.C;
        if (pro == PRO_UPCAT && skip.st.p) { a.skip_stats = skip.st; a.skip_gamma = skip.gamma; a.skip_beta = skip.beta; }
    }
    a.dst = dst; a.dst_ld = dst_ld;
    a.epi = epi; a.epi_stats = epi_stats; a.bias = bias; a.resid = resid; a.resid_ld = resid_ld; a.row_stats = row_stats;
    return a;
}
// One Linear layer: y[rows][N] = x[rows][K] @ W^T + b (+GELU | +resid, epi), the LayerNorm pending on x (x.st.p) in the load
// prologue; on the layer's split copy where the caller runs split precision and the layer has one
static GemmArgs linear_args(const AffineSrc& x, int rows, int geom_M, const LinW& w, bool split, unsigned sw, int epi, float* y,
                            const float* resid = nullptr, double* row_stats = nullptr) {
    const int sp = (split && w.ws) ? 1 : 0;
    return gemm_args(rows, geom_M, 1, 1, w.in, w.out, 1, sp, sw, nullptr, x.st.p ? PRO_GN : PRO_NONE, x, 0, AffineSrc{},
                     sp ? w.ws : w.w, nullptr, y, w.out, epi, nullptr, w.b, resid, w.out, row_stats);
}

// -------------------------------------------------------------------------------------------------
// plan helpers
// Statistics slots reserved per sample for a raw conv output [HW][C] whose own tiling writes `slots`: room for the finest
// tiling any batch size can select (gemm_geometry is batch-dependent, the dry run that sizes the arena is not): 128-row x
// 64-wide tiles, or the split-K combine kernel's row groups
static int stats_slots_reserved(int HW, int C, int slots) {
    return std::max(std::max(std::max(slots, stats_slots(HW, 128, std::max(1, C / 64))),   // (coarser tilings need fewer)
                             stats_slots(HW, combine_rows(HW, C), 1)),
                    std::max(stats_slots(HW, 16, std::max(1, C / 16)),              // conv_skinny's finest tiling
                             stats_slots(HW, std::max(HW / 4, 1), 1)));             // conv_in_kernel's four row parts
}

// launches of this process whose epilogue also wrote the MaxPool2d(2) of their output (host-side count:
// spdm_debug_pooled_epilogue_launches)
static int g_pooled_epilogue_launches = 0;
// fused conv_chain.hip launches of this process's plans (host-side count: spdm_debug_conv_chain_launches)
static int g_conv_chain_launches = 0;
// SPDM_TUNE25 where the environment does not set it: the sites (bit 0 down block 3, bit 1 the bottleneck) whose fused launch
// measured faster than their per-layer launches at B = 4096
constexpr int CHAIN_SITES_DEFAULT = 3;

// The kernel routes of one U-Net evaluation: Ctx::choose_routes fills them in before the walk (plan_unet), which then only
// allocates and launches; spdm_debug_plan_routes reports them field by field in this order (all int: 44 values).
enum { POOL_KERNEL = 0, POOL_READ_THROUGH = 1, POOL_BY_PRODUCER = 2 };   // pool_kernel | the consumer's PRO_POOL | the producer's epilogue
enum { UP_UPCAT = 0, UP_READ_THROUGH = 1, UP_TWO_SOURCE = 2 };           // upcat kernel | the consumer's PRO_UPCAT | upsample + two-source conv
enum { FILM_APPLY = 0, FILM_COEF = 1, FILM_LOCAL = 2 };                  // film_apply | film_coef | coefficients evaluated in the consumers
enum { SA_IN_GEMM = 0, SA_IN_QKV = 1, SA_IN_HEAD = 2 };                  // what feeds the attention core: in_proj GEMM | sa_qkv | sa_head (core included)
struct AttnRoute {
    int fused, crop, outc;     // sa_fused64 takes the whole block; ... for the tokens outc reads only (sa6); ... with outc in its epilogue
    int in, tail;              // otherwise: SA_IN_*, and sa_tail (1) or the three GEMMs (0) after the core -- decided independently
};
struct PlanRoutes {
    int pool[3];               // POOL_* of pool i + 1 (level i -> i + 1)
    int up[3];                 // UP_* of up block i + 1
    int film[6];               // FILM_* of the tail of down1..3, up1..3
    AttnRoute sa[6];           // sa1..6 (all zero without attention: nothing is launched)
    int chain[2];              // the level-3 convolutions of down block 3 / of the bottleneck as ONE conv_chain.hip launch each
};
// one layer of a fused chain: the convolution and the GroupNorm [-> GELU] pending on its input (gamma null: a finished input)
struct ChainStep { const ConvW* w; const float* gamma; const float* beta; int gelu; };

struct Ctx {
    spdm_handle* h;
    int B;
    hipStream_t s;
    bool dry;
    int err = SPDM_OK;
    // batch the launch geometry is chosen for: the call's, or -- SW_PIN_GEOMETRY -- always the handle's max_batch, so that a shard
    // of a larger batch selects exactly the kernels (tiles, split-K, small-grid kernel, fused sources) the whole batch would
    int Bg() const { return (h->sw & SW_PIN_GEOMETRY) ? h->cfg.max_batch : B; }
    int HWl(int l) const { return (h->Hp >> l) * (h->Wp >> l); }
    int Hl(int l) const { return h->Hp >> l; }
    int Wl(int l) const { return h->Wp >> l; }

    bool reserve(size_t bytes, size_t* off) {       // room in the slab; false, with err set, when it is exhausted
        if (h->arena.alloc(bytes, off)) return true;
        if (!err) err = fail(SPDM_ERR_NOMEM, "workspace exhausted (batch %d)", B);
        return false;
    }
    Tensor ralloc(int rows, int C, int level = -1) {       // [rows][C] scratch (attention path)
        Tensor t;
        t.C = C; t.level = level;
        size_t off = 0;
        if (!reserve(sizeof(float) * (size_t)rows * C, &off)) return t;
        t.off = off; t.p = (float*)(h->arena.base + off); t.valid = true;
        return t;
    }
    Tensor talloc(int C, int level) {
        const Tensor t = ralloc(B * HWl(level), C, level);
        if (t.valid && !dry && (h->sw & SW_ARENA_TRACE)) fprintf(stderr, "[spdm] level %d C %3d at %8.2f MiB (%.1f MiB)\n", level, C, t.off / 1048576.0, (double)B * HWl(level) * C * 4 / 1048576.0);
        return t;
    }
    StatsBuf salloc(int HW, int C, int m_tile, int n_tiles, int C_norm = 0) {     // C_norm > 0: real channels of padded storage
        StatsBuf sb;
        const int slots = stats_slots(HW, m_tile, n_tiles);
        const int slots_max = stats_slots_reserved(HW, C, slots);
        size_t off = 0;
        if (!reserve(sizeof(double) * 2 * (size_t)B * slots_max, &off)) return sb;
        sb.off = off; sb.p = (double*)(h->arena.base + off); sb.valid = true;
        sb.ref.p = sb.p; sb.ref.slots = slots; sb.ref.m_tile = m_tile; sb.ref.n_tiles = n_tiles; sb.ref.HW = HW;
        sb.ref.inv_count = 1.0 / ((double)(C_norm > 0 ? C_norm : C) * (double)HW);
        return sb;
    }
    void free(Tensor& t) { if (t.valid) { h->arena.release(t.off); t.valid = false; } }
    void free(StatsBuf& s2) { if (s2.valid) { h->arena.release(s2.off); s2.valid = false; } }
    void free(Value& v) { free(v.t); free(v.st); }
    void check(hipError_t e, const char* what) {
        if (e != hipSuccess && !err) err = fail(SPDM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    AffineSrc asrc(const Value& v) const {
        AffineSrc a{};
        a.x = v.t.p; a.C = v.t.C;
        if (v.pending_gn()) { a.st = v.st.ref; a.gamma = v.gamma; a.beta = v.beta; }
        else { a.st = StatsRef{}; a.st.p = nullptr; a.gamma = nullptr; a.beta = nullptr; }
        return a;
    }
    void tap(const char* name, const Tensor& t) {
        if (h->arena.keep && !dry) { h->taps[name] = t; h->tapB = B; }
    }

    // the launch of one statistics-epilogue convolution of this plan (out: null while only asking which kernel would take it);
    // h->d_partial non-null: launch_gemm may split K (small grids)
    GemmArgs conv_args(const ConvW& w, int level, int split, int pro, const AffineSrc& src, int up_C, const AffineSrc& skip,
                       const Value* out) const {
        const int HW = HWl(level);
        return gemm_args(B * HW, Bg() * HW, Hl(level), Wl(level), w.cin, w.cout, w.taps, split, h->sw, h->d_partial, pro, src, up_C,
                         skip, split ? w.ws : w.w, split ? w.wf : nullptr, out ? out->t.p : nullptr, w.cout, EPI_STATS,
                         out ? out->st.p : nullptr);
    }
    // workspace of a conv result: the raw output and its GroupNorm partial sums in the statistics layout of g
    Value conv_out(const ConvW& w, int level, const GemmGeom& g, const float* gamma, const float* beta, int C_norm = 0) {
        Value out;
        out.t = talloc(w.cout, level);
        out.st = salloc(HWl(level), w.cout, g.st_m_tile, g.st_n_tiles, C_norm);
        out.gamma = gamma; out.beta = beta;
        return out;
    }
    // the statistics layout the sizing pass reserves for a convolution reading through a resampling op (conv_fused, conv_two)
    GemmGeom dry_geometry(const ConvW& w, int level) const {
        return gemm_geometry(B * HWl(level), w.cout, w.cin, HWl(level), Wl(level), w.taps, (w.cin % 32 == 0) ? 1 : 0, h->sw, /*stats_epi=*/true);
    }
    // One implicit-GEMM launch of the plan.  Profiling (spdm_profile_*) times the statistics-epilogue convolutions with HIP events
    // on the launch stream.  Runs of CONSECUTIVE conv launches (the two DoubleConvolutions of a block: nothing else is launched in
    // between) share one event pair -- every event record is a queue barrier that costs the neighbouring kernels their overlap
    // (62 records per step were worth 0.25 ms), and the class average only needs total time / launches.
    void gemm(const GemmArgs& a, const char* what) {
        const bool prof = h->prof && a.epi == EPI_STATS;
        const bool solo = prof && h->prof_open < 0;
        if (solo) prof_begin();
        if (prof && h->prof_open >= 0) {
            h->prof_evts[h->prof_open].flops += gemm_flops(a);
            h->prof_evts[h->prof_open].launches += 1;
        }
        check(launch_gemm(a, s), what);
        if (solo) prof_end();
    }
    // one 3x3 conv: reads `in` (finishing its pending GroupNorm, + GELU if asked, in the load
    // prologue), writes the raw output and its GroupNorm partial sums
    // pool_out (POOL_BY_PRODUCER): the launch also writes the RAW MaxPool2d(2) map of its output there (GemmArgs::pool_dst);
    // pooled_of: `in` is such a map, and the GroupNorm pending on it is that of the finer level's value *pooled_of (PRO_GN_POOLED)
    Value conv(const Value& in, const ConvW& w, int level, bool gelu, const float* gamma, const float* beta,
               const Tensor* pool_out = nullptr, const Value* pooled_of = nullptr) {
        // by shape before the weights are known (the dry run at create); afterwards a tensor outside the split format's
        // range has no split copy and stays on the exact fp32 kernel (Loader::conv)
        const int split = (h->split && w.cin % 32 == 0 && (!h->weights_loaded || w.ws)) ? 1 : 0;
        const int pro = pooled_of ? PRO_GN_POOLED : in.pending_gn() ? (gelu ? PRO_GN_GELU : PRO_GN) : PRO_NONE;
        AffineSrc src = asrc(in);
        if (pooled_of) { src.st = pooled_of->st.ref; src.gamma = pooled_of->gamma; src.beta = pooled_of->beta; }
        auto args = [&](const Value* out) {
            GemmArgs a = conv_args(w, level, split, pro, src, 0, AffineSrc{}, out);
            if (pool_out && out) { a.pool_dst = pool_out->p; a.pool_ld = pool_out->C; a.pool_gamma = gamma; }
            return a;
        };
        Value out = conv_out(w, level, gemm_geometry(args(nullptr)), gamma, beta, w.cnorm);
        if (err || dry) return out;
        if ((split ? w.ws : w.w) == nullptr) { err = fail(SPDM_ERR_STATE, "plan: conv weights missing"); return out; }
        if (in.t.C != w.cin) { err = fail(SPDM_ERR_INVALID, "plan: conv input has %d channels, weight expects %d", in.t.C, w.cin); return out; }
        gemm(args(&out), "conv3x3 implicit GEMM");
        if (pool_out) ++g_pooled_epilogue_launches;
        return out;
    }
    // ---- the routes: every rule that picks between kernels, decided here, once, before the walk ----
    // A stand-in for a tensor of the walk in the kernel-selection queries: they read its width and the GroupNorm pending on it
    // (gn: the DoubleConvolution whose raw output at `level` it is), never its data (any non-null pointer; not dereferenced)
    AffineSrc route_src(int C, const DoubleConvW* gn = nullptr, int level = 0) const {
        AffineSrc a{h->d_x, C};
        if (gn) { a.st.p = (const double*)h->d_x; a.st.HW = HWl(level); a.gamma = gn->gamma; a.beta = gn->beta; }
        return a;
    }
    // A pure function of the handle (config, switches, which weight copies exist) and Bg().  The route of a resampling op depends
    // on the launch geometry, so on the batch: the sizing pass (dry_plan_all) passes each combination in as `sized`, which answers
    // in place of the geometry and the weight copies; a route whose other conditions fail falls to the op's own kernel.
    PlanRoutes choose_routes(const PlanRoutes* sized = nullptr) const {
        PlanRoutes r{};
        const bool loaded = h->weights_loaded, keep = h->arena.keep;
        const unsigned sw = h->sw;
        // -- SelfAttention.forward (models/Unet_FiLmLayer.py:71-82) and the FiLM tail in front of it --
        for (int b = 0; b < 6 && h->cfg.attention; ++b) {
            const AttnW& w = h->sa[b];
            const int level = b < 3 ? b + 1 : 5 - b, L = HWl(level), C = w.C;
            AttnRoute& a = r.sa[b];
            a.fused = h->split && sa_fused_supported(L, C) && !(sw & SW_NO_SA_FUSED) && (!loaded || w.fw[0]);
            // The last block (sa6) feeds only outc + unpad, which read the H0 x D tokens of the trajectory: sa_fused64 then computes
            // the block for those tokens only (SaCrop).  Not in debug runs (the a6 tap keeps its full meaning).
            a.crop = a.fused && b == 5 && !keep && !(sw & SW_NO_SA_CROP) && sa_crop_supported(L, C, h->cfg.horizon, h->cfg.state_dim);
            a.outc = a.crop && !(sw & SW_NO_SA_OUTC) && h->outc_w;
            const bool tail_kernels = h->split && sa_tail_supported(C, sw);       // sa_tail.hip: sa_qkv / sa_head / sa_tail
            // May the FiLM tail be folded into the block's loads (film_coef)?  Only the kernels that read the block input themselves
            // take the coefficients: sa_fused64 (the two-workgroup mode for longer sequences has no registers left) and the
            // sa_qkv / sa_tail pair.
            const bool fold = !keep && h->split && !(sw & SW_NO_FILM_FOLD) &&
                              (a.fused ? L <= 256 : tail_kernels && (!loaded || (w.qkv_wf && w.tail_wf[0])));
            // ... and may those kernels evaluate the coefficients themselves (no film_coef launch)?
            // Only at the smallest batches (every launch a single workgroup): measured on the whole step (same box, alternating,
            // graph replay), evaluating the coefficients inside the consumers saves 5 us per step at batch 1-4 (0.490 -> 0.485 ms) and
            // COSTS 8 us at batch 64, 10-30 us at 512, ~50 us at 4096 -- every workgroup of sa_qkv / sa_tail repeats the statistics
            // round trip and one barrier that the 5-us film_coef launch does once per sample.  SPDM_FILM_LOCAL=1 forces it on (tests).
            const bool local = fold && !(sw & SW_NO_FILM_LOCAL) && (Bg() <= 4 || (sw & SW_FILM_LOCAL)) &&
                               (a.fused || sa_tail_film_local(C, L));
            r.film[b] = local ? FILM_LOCAL : fold ? FILM_COEF : FILM_APPLY;
            if (a.fused) continue;
            // LayerNorm + in_proj + attention core in ONE kernel where the row tile holds whole samples (sa_head_kernel): q, k, v never
            // reach memory.
            // Only on large grids: a workgroup of the fused kernel is a 25-30 us chain (LayerNorm, twelve small products, four rounds of
            // q/k/v tiles -> scores -> softmax -> P v with two to four barriers each) at two workgroups per CU, so it needs many rounds
            // of workgroups to beat three launches that each fill the chip.  Measured (traced, same box; q/k/v + core launches -> fused):
            // B = 4096: sa1 281 -> 234 us, sa2 171 -> 164, sa4 75 -> 70, sa3 50 -> 52; B = 512: 35 -> 38, 34 -> 44, 19 -> 32, 17 -> 34;
            // B = 64: 13-17 -> 26-32 us each.  Rule: at least 2048 row tiles (SPDM_SA_HEAD=1 forces the fused kernel at any size: tests; SPDM_TUNE16: the threshold).
            const int TMh = 8192 / C;
            const bool head = tail_kernels && sa_head_supported(C, L, sw) && loaded && w.qkv_wf && (!local || sa_tail_film_local(C, L)) &&
                              ((Bg() * L + TMh - 1) / TMh) >= ((sw & SW_SA_HEAD) ? 1 : spdm_tune(16, 2048));
            a.in = head ? SA_IN_HEAD : (tail_kernels && (!loaded || w.qkv_wf)) ? SA_IN_QKV : SA_IN_GEMM;
            a.tail = tail_kernels && (!loaded || w.tail_wf[0]);
        }
        // -- the level-3 convolution chains (conv_chain.hip): the four convolutions of down block 3 and the six of the bottleneck
        //    as one launch each, the intermediate tensors never leaving LDS.  Only where the handle keeps no intermediate (no
        //    debug taps), every layer has its split copies, the shape rule holds (3-tap layers on a width-1 map) and the launch
        //    fills the chip: 64-row blocks, one per CU in a single round, so from 256 blocks on.  SPDM_TUNE25 (read once per
        //    process): bit 0 / 1 = the site, bit 2 = at any batch (tests).  The sizing pass asks for both states (sized->chain). --
        {
            const int tune = spdm_tune(25, CHAIN_SITES_DEFAULT);
            const int M3 = Bg() * HWl(3);
            const bool fills = M3 >= 256 * CHAIN_M_TILE || (tune & 4);
            const DoubleConvW* site[2][3] = {{&h->down[2].dc1, &h->down[2].dc2, nullptr}, {&h->bot[0], &h->bot[1], &h->bot[2]}};
            for (int i = 0; i < 2; ++i) {
                int chan[CHAIN_MAX_LAYERS + 1], n = 0;
                bool ok = h->split && !keep && ((tune >> i) & 1) && fills && (sized ? sized->chain[i] != 0 : loaded);
                chan[0] = site[i][0]->first.cin;
                ok = ok && chan[0] == (i ? h->down[2].cout : h->down[1].cout);
                for (int d = 0; d < 3 && site[i][d]; ++d)
                    for (const ConvW* w : {&site[i][d]->first, &site[i][d]->second}) {
                        ok = ok && w->taps == 3 && w->cin == chan[n] && (sized || (w->ws && w->wf));
                        chan[++n] = w->cout;
                    }
                // (both sites read a FINISHED tensor -- the pooled output of sa2's block tail, the output of sa3's -- which is what
                //  Ctx::conv_chain's first layer takes (no prologue) and checks; an encoder tail that left a GroupNorm pending on
                //  either would have to switch that site off here)
                r.chain[i] = ok && conv_chain_geometry(M3, HWl(3), Wl(3), 3, 1, n, chan);
            }
        }
        // -- the fused sources of a Down / UpSample block's first convolution (read-through, two-source) --
        const bool src_ok = h->split && !(sw & SW_NO_FUSED_SRC) && !keep;
        const int C_x1 = h->inc.second.cout;
        for (int i = 0; i < 3; ++i) {      // pool i + 1 (level i -> i + 1); consumer wn = the first convolution of down block i + 1
            const ConvW& wn = h->down[i].dc1.first;
            const int C_in = i ? h->down[i - 1].cout : C_x1;
            // MaxPool2d(2) read through by that convolution (PRO_POOL: conv_skinny at small batch; it keeps priority)
            // (not pool 3 in front of a fused down block 3: the chain reads a materialised map)
            const bool through = src_ok && h->d_partial != nullptr && C_in == wn.cin && !(i == 2 && r.chain[0]) &&
                (sized ? sized->pool[i] == POOL_READ_THROUGH
                       : loaded && wn.ws && wn.wf && gemm_takes_fused_source(conv_args(wn, i + 1, 1, PRO_POOL, AffineSrc{nullptr, C_in}, 0, AffineSrc{}, nullptr)));
            // MaxPool2d(2) written by the epilogue of the kernel that produces the tensor being pooled: no pool_kernel launch, the
            // tensor is not read back.  SPDM_TUNE23 (read once per process): bit i = pool i + 1; default 7, 0 = pool_kernel everywhere
            bool by_producer = h->split && !keep && ((spdm_tune(23, 7) >> i) & 1) && !(Hl(i) & 1) && !(Wl(i) & 1) && !through &&
                               (sized ? sized->pool[i] == POOL_BY_PRODUCER : loaded);
            if (i == 0) {
                // pool 1: inc's second convolution (w, level 0) on conv_reg.hip at width 8 writes the RAW pooled map (the GroupNorm
                // pending on x1 stays pending on it), and down1's first convolution, on conv_reg.hip too, applies it on load
                // (PRO_GN_POOLED)
                const ConvW& w = h->inc.second;
                const AffineSrc none{};
                by_producer = by_producer && Wl(0) == 8 && w.cout == wn.cin &&
                    (sized || (w.ws && w.wf && wn.ws && wn.wf &&
                               gemm_geometry(conv_args(w, 0, 1, PRO_GN_GELU, none, 0, none, nullptr)).reg &&
                               gemm_geometry(conv_args(wn, 1, 1, PRO_GN_POOLED, none, 0, none, nullptr)).reg &&
                               pooled_stats_serial(StatsRef{nullptr, 0, 64, 1, HWl(0), 0.0})));       // (x1's slots, one per 64-row wave tile)
            } else {
                // pools 2 and 3: the block output (sa1, sa2) is finished, so sa_tail's epilogue writes its plain MaxPool2d(2) --
                // where every window lies inside one workgroup's rows
                const AttnRoute& a = r.sa[i - 1];
                by_producer = by_producer && h->cfg.attention && !a.fused && a.tail && sa_tail_pools(h->sa[i - 1].C, HWl(i), Wl(i), B * HWl(i));
            }
            r.pool[i] = by_producer ? POOL_BY_PRODUCER : through ? POOL_READ_THROUGH : POOL_KERNEL;
        }
        for (int i = 0; i < 3; ++i) {      // up block i + 1 (level 3 - i -> 2 - i): cat([upsample x2 of src, skip]) into w
            const ConvW& w = h->up[i].dc1.first;
            const int lout = 2 - i;
            // src: x5 (its GroupNorm pending), then the up blocks' outputs; skip: x3, x2, then x1 (pending)
            const AffineSrc src = i ? route_src(h->up[i - 1].cout) : route_src(h->bot[2].second.cout, &h->bot[2], 3);
            const AffineSrc skip = i < 2 ? route_src(h->down[1 - i].cout) : route_src(C_x1, &h->inc, 0);
            const bool fits = src_ok && src.C + skip.C == w.cin, copies = loaded && w.ws && w.wf;
            // upsample + concat read through by the convolution (PRO_UPCAT: conv_skinny, or conv_wide's whole-sample tiles) ...
            const bool through = fits && h->d_partial != nullptr &&
                (sized ? sized->up[i] == UP_READ_THROUGH : copies && gemm_takes_fused_source(conv_args(w, lout, 1, PRO_UPCAT, src, src.C, skip, nullptr)));
            // ... or upsample only: the convolution reads [upsampled | skip] from the two tensors (conv_wide.hip TWO)
            const bool two = !through && fits &&
                (sized ? sized->up[i] == UP_TWO_SOURCE : copies && gemm_takes_two_sources(two_args(src.x, skip, w, lout, nullptr)));
            r.up[i] = through ? UP_READ_THROUGH : two ? UP_TWO_SOURCE : UP_UPCAT;
        }
        return r;
    }
    void prof_begin() {
        if (!h->prof || h->prof_open >= 0 || dry || err) return;
        ProfEvt e{};
        bool have = false;
        if (!h->prof_pool.empty()) {
            e = h->prof_pool.back();
            h->prof_pool.pop_back();
            e.flops = 0.0; e.launches = 0;
            have = true;
        } else {
            have = hipEventCreate(&e.a) == hipSuccess && hipEventCreate(&e.b) == hipSuccess;
        }
        if (have) {
            h->prof_evts.push_back(e);
            h->prof_open = (int)h->prof_evts.size() - 1;
            (void)hipEventRecord(e.a, s);
        }
    }
    void prof_end() {
        if (h->prof_open < 0) return;
        (void)hipEventRecord(h->prof_evts[h->prof_open].b, s);
        h->prof_open = -1;
    }
    // DoubleConvolution.forward, models/Unet_FiLmLayer.py:108-115.  Consumes `in`.
    Value double_conv(Value& in, const DoubleConvW& w, int level, bool keep_in = false) {
        Value mid = conv(in, w.first, level, /*gelu=*/false, w.gamma, w.beta);
        if (!keep_in) free(in);
        Value out = conv(mid, w.second, level, /*gelu=*/true, w.gamma, w.beta);
        free(mid);
        return out;
    }
    // A list of level-3 convolutions as ONE launch (conv_chain.hip; routes.chain): reads the finished tensor `in`, writes the last
    // layer's raw output and its GroupNorm partials (out_gamma / out_beta pending on it) -- what the per-layer launches leave
    // behind, without their intermediate tensors.  Inside prof_begin / prof_end it counts as one launch of the layers' FLOPs.
    Value conv_chain(const Value& in, const ChainStep* st, int n, const float* out_gamma, const float* out_beta, int level) {
        GemmGeom g{};
        g.st_m_tile = CHAIN_M_TILE; g.st_n_tiles = 1;
        Value out = conv_out(*st[n - 1].w, level, g, out_gamma, out_beta);
        if (err || dry) return out;
        ChainArgs a{};
        a.src = in.t.p; a.src_ld = in.t.C; a.dst = out.t.p; a.dst_ld = out.t.C; a.stats = out.st.p; a.slots = out.st.ref.slots;
        a.M = B * HWl(level); a.HW = HWl(level); a.n_layers = n;
        for (int i = 0; i < n; ++i) {
            if (st[i].w->wf == nullptr) { err = fail(SPDM_ERR_STATE, "plan: conv chain weights missing"); return out; }
            a.layer[i] = ChainLayer{st[i].w->wf, st[i].gamma, st[i].beta, st[i].w->cin, st[i].w->cout, st[i].gelu};
        }
        if (in.t.C != a.layer[0].K || in.pending_gn()) { err = fail(SPDM_ERR_INVALID, "plan: conv chain reads a finished tensor of %d channels", a.layer[0].K); return out; }
        const bool solo = h->prof && h->prof_open < 0;
        if (solo) prof_begin();
        if (h->prof && h->prof_open >= 0) {
            h->prof_evts[h->prof_open].flops += conv_chain_flops(a);
            h->prof_evts[h->prof_open].launches += 1;
        }
        check(launch_conv_chain(a, s), "conv3x1 chain");
        if (solo) prof_end();
        ++g_conv_chain_launches;
        return out;
    }
    // The FIRST convolution of a Down / UpSample block reading its input THROUGH the resampling op (GemmArgs "fused sources":
    // PRO_POOL: MaxPool2d(2) of src0, the finer level's value; PRO_UPCAT: cat([upsample x2 of src0 (coarser level), skip])) --
    // no pooled / concatenated tensor is written or read back, and one launch less.  Where the route says so (POOL_READ_THROUGH,
    // UP_READ_THROUGH: choose_routes asked gemm_takes_fused_source about these very arguments).
    Value conv_fused(int mode, const Value& src0, const Value* skip, const DoubleConvW& dc, int level) {
        auto args = [&](const Value* out) {
            return conv_args(dc.first, level, 1, mode, asrc(src0), skip ? src0.t.C : 0, skip ? asrc(*skip) : AffineSrc{}, out);
        };
        return conv_first(dc, level, args, "conv3x3 implicit GEMM (fused source)");
    }
    // ... on the launch args(out) builds: the output in that launch's statistics layout (sizing pass: by shape), then the launch
    template <class Args> Value conv_first(const DoubleConvW& dc, int level, Args args, const char* what) {
        Value out = conv_out(dc.first, level, dry ? dry_geometry(dc.first, level) : gemm_geometry(args(nullptr)), dc.gamma, dc.beta);
        if (!err && !dry) gemm(args(&out), what);
        return out;
    }
    // The first convolution of an UpSample block with a TWO-SOURCE input (conv_wide.hip TWO): channels [0, C_up) from `up2x`, the
    // upsampled tensor (finished), the rest from the skip connection, whose pending GroupNorm is the load prologue.  torch.cat
    // (models/Unet_FiLmLayer.py:218) is never materialised.  Where the route is UP_TWO_SOURCE (choose_routes asked
    // gemm_takes_two_sources BEFORE the upsample is launched).
    Value conv_two(const Tensor& up2x, const Value& skip, const DoubleConvW& dc, int level) {
        return conv_first(dc, level, [&](const Value* out) { return two_args(up2x.p, asrc(skip), dc.first, level, out); },
                          "conv3x3 implicit GEMM (two-source input)");
    }
    // conv_two's launch: input channels [0, C_up) from `up` (finished), the rest from the skip connection, whose pending GroupNorm
    // is the load prologue
    GemmArgs two_args(const float* up, const AffineSrc& skip, const ConvW& w, int level, const Value* out) const {
        const int C_up = w.cin - skip.C;
        return conv_args(w, level, 1, skip.st.p ? PRO_GN : PRO_NONE, AffineSrc{up, C_up}, C_up, skip, out);
    }
    // y[rows][N] = x[rows][K] @ W^T + b  (+GELU | +resid)
    // per-token LayerNorm statistics buffer: [rows][n_tiles][2] fp64 (StatsRef with HW = 1: "sample" = row)
    StatsBuf row_stats_alloc(int rows, int C, int n_tiles) {
        StatsBuf sb;
        size_t off = 0;
        if (!reserve(sizeof(double) * 2 * (size_t)rows * std::max(n_tiles, C / 64), &off)) return sb;   // finest tiling
        sb.off = off; sb.p = (double*)(h->arena.base + off); sb.valid = true;
        sb.ref.p = sb.p; sb.ref.slots = n_tiles; sb.ref.m_tile = 1 << 30; sb.ref.n_tiles = n_tiles; sb.ref.HW = 1;
        sb.ref.inv_count = 1.0 / (double)C;
        return sb;
    }
    void linear(const float* x, int ld, int rows, const LinW& w, float* y, int epi, const float* resid,
                const StatsBuf* ln = nullptr, const float* ln_g = nullptr, const float* ln_b = nullptr,
                double* row_stats_out = nullptr) {
        if (err || dry) return;
        const AffineSrc src = ln ? AffineSrc{x, ld, ln->ref, ln_g, ln_b} : AffineSrc{x, ld};    // LayerNorm in the load prologue
        gemm(linear_args(src, rows, (rows / B) * Bg(), w, h->split, h->sw, epi, y, resid, row_stats_out), "linear GEMM");
    }
    // SelfAttention.forward, models/Unet_FiLmLayer.py:71-82.  Consumes x (and its per-token LayerNorm
    // statistics xs, produced by film_apply), returns the block output.  Both LayerNorms run as the load
    // prologue of the GEMM that consumes them: self.ln -> in_proj, ff_self[0] -> ff_self[1].  The launches: routes.sa[blk].
    // ab (optional): x is the RAW conv output and the block input is ab-affine of it (film_coef); consumed here.
    // fs (optional, instead of ab): the kernels evaluate those coefficients themselves (FilmSpec, kernels.h)
    // pool_out (POOL_BY_PRODUCER of the next pool): sa_tail also writes the MaxPool2d(2) of the block output, reserved here
    Tensor attention(Tensor& x, StatsBuf& xs, int blk, int level, Tensor* ab, const FilmSpec* fs, Tensor* pool_out) {
        const AttnW& w = h->sa[blk];
        const AttnRoute& route = routes.sa[blk];
        const int L = HWl(level), rows = B * L, C = w.C;
        const float* abp = (ab && ab->valid) ? ab->p : nullptr;
        if (route.fused) {                   // whole block in one kernel (sa_fused.hip)
            // (cropped: the same tensor is reserved -- the dry run sizes both routes alike -- and holds the block output at the
            //  query tokens only, or, with outc folded in, eps [B][H0][D] at its start)
            Tensor out = talloc(C, level);
            const bool oc = route.outc;
            const SaCrop crop{h->cfg.horizon, h->cfg.state_dim, h->Wp, h->lh, h->lw, oc ? h->outc_w : nullptr, oc ? h->outc_b : 0.f, oc ? out.p : nullptr};
            if (!err && !dry)
                check(launch_sa_fused64(x.p, out.p, B, L, w.ln_g, w.ln_b, w.ff_ln_g, w.ff_ln_b, w.fw, w.in_proj.b,
                                        w.out_proj.b, w.ff1.b, w.ff2.b, abp, h->sw, s, fs, route.crop ? &crop : nullptr),
                      "fused attention block");
            free(x);
            free(xs);
            if (ab) free(*ab);
            return out;
        }
        Tensor qkv = ralloc(rows, 3 * C);
        // (SA_IN_HEAD: the workspace operations stay those of the three-launch path -- qkv is reserved and released unused -- so the
        // slab sized by the dry run fits whichever path a call takes.)
        const bool head = route.in == SA_IN_HEAD;
        if (route.in == SA_IN_QKV && !err && !dry)       // LayerNorm + in_proj in one 64-row kernel (sa_tail.hip)
            check(launch_sa_qkv(C, x.p, qkv.p, rows, w.qkv_wf, w.in_proj.b, w.ln_g, w.ln_b, abp, L, s, fs), "attention in_proj");
        if (route.in == SA_IN_GEMM) linear(x.p, C, rows, w.in_proj, qkv.p, EPI_BIAS, nullptr, &xs, w.ln_g, w.ln_b);
        free(xs);
        Tensor att = ralloc(rows, C);
        if (!err && !dry) {
            if (head) check(launch_sa_head(C, x.p, att.p, rows, w.qkv_wf, w.in_proj.b, w.ln_g, w.ln_b, abp, L, s, fs), "attention in_proj + core");
            else check(launch_attention_auto(qkv.p, att.p, B, L, C, 4, h->sw, s), "attention core");
        }
        free(qkv);
        if (route.tail) {
            // out_proj + residual + LayerNorm + ff_self + residual in one kernel (sa_tail.hip)
            Tensor out = talloc(C, level);
            float* pool = nullptr;
            if (pool_out) {             // (reserved here, after `out`: the order of the workspace operations decides the offsets)
                *pool_out = talloc(C, level + 1);
                pool = pool_out->p;
            }
            if (!err && !dry) {
                check(launch_sa_tail(C, att.p, x.p, out.p, rows, w.tail_wf[0], w.tail_wf[1], w.tail_wf[2], w.out_proj.b, w.ff1.b,
                                        w.ff2.b, w.ff_ln_g, w.ff_ln_b, abp, L, s, fs, nullptr, pool, Wl(level)), "attention tail");
                if (pool) ++g_pooled_epilogue_launches;
            }
            free(att);
            free(x);
            if (ab) free(*ab);
            return out;
        }
        Tensor av = talloc(C, level);
        const int nt_av = gemm_geometry((rows / B) * Bg(), C, C, 1, 1, 1, (h->split && w.out_proj.ws) ? 1 : 0, h->sw).n_tiles;   // n-tiles of the out_proj GEMM
        StatsBuf avs = row_stats_alloc(rows, C, nt_av);
        linear(att.p, C, rows, w.out_proj, av.p, EPI_BIAS_RESID, x.p, nullptr, nullptr, nullptr, avs.p);
        free(att);
        free(x);
        Tensor f1 = ralloc(rows, C);
        linear(av.p, C, rows, w.ff1, f1.p, EPI_BIAS_GELU, nullptr, &avs, w.ff_ln_g, w.ff_ln_b);
        free(avs);
        Tensor out = talloc(C, level);
        linear(f1.p, C, rows, w.ff2, out.p, EPI_BIAS_RESID, av.p);
        free(f1);
        free(av);
        return out;
    }
    FilmSpec film_spec(const Value& v, const ResampleW& w, int blk, bool use_cond) const {
        FilmSpec f{};
        if (v.pending_gn()) { f.st = v.st.ref; f.gamma = v.gamma; f.beta = v.beta; }
        f.temb = w.temb_table; f.t_dev = h->d_t; f.t_count = h_tcount;
        f.film = (use_cond && h->cfg.cond_dim > 0) ? h->d_film[blk] : nullptr;
        f.C = w.cout; f.on = 1;
        return f;
    }
    // the FiLM tail as coefficients (film_coef_kernel): returns the RAW conv tensor of v (its statistics are released),
    // *ab receives [B][2 C]
    Tensor film_coef(Value& v, const ResampleW& w, int blk, bool use_cond, Tensor* ab) {
        *ab = ralloc(B, 2 * w.cout);
        if (!err && !dry)
            check(launch_film_coef(asrc(v), w.temb_table, h->d_t, (h_tcount), (use_cond && h->cfg.cond_dim > 0) ? h->d_film[blk] : nullptr,
                                   ab->p, B, s), "film_coef");
        Tensor raw = v.t;
        v.t.valid = false;
        free(v);
        return raw;
    }
    // tail of DownSample/UpSample.forward: + time embedding, FiLM.  Consumes v.
    Tensor film_tail(Value& v, const ResampleW& w, int blk, int level, bool use_cond, StatsBuf* row_stats) {
        Tensor y = talloc(w.cout, level);
        if (row_stats) *row_stats = row_stats_alloc(B * HWl(level), w.cout, 1);
        if (!err && !dry)
            check(launch_film_apply(asrc(v), w.temb_table, h->d_t, (h_tcount), (use_cond && h->cfg.cond_dim > 0) ? h->d_film[blk] : nullptr,
                                    y.p, row_stats ? row_stats->p : nullptr, B, HWl(level), s), "film_apply");
        free(v);
        return y;
    }
    // the block tail (film_tail; tap `name` where it is materialised) and the SelfAttention block sa[blk] after it.  The attention
    // kernels finish the tail themselves from the raw tensor (FILM_LOCAL), take it as coefficients on load (FILM_COEF), or
    // read the materialised tensor.  Consumes v.  pool_out: see attention.
    Tensor film_attention(Value& v, const ResampleW& w, int blk, int level, bool use_cond, const char* name, Tensor* pool_out = nullptr) {
        const bool local = routes.film[blk] == FILM_LOCAL;
        const FilmSpec fs = local ? film_spec(v, w, blk, use_cond) : FilmSpec{};
        StatsBuf ys;
        Tensor y, ab;
        if (local) {
            y = v.t;
            v.t.valid = false;
        } else if (routes.film[blk] == FILM_COEF) {
            y = film_coef(v, w, blk, use_cond, &ab);
        } else {
            y = film_tail(v, w, blk, level, use_cond, (h->cfg.attention && !routes.sa[blk].fused) ? &ys : nullptr);
            tap(name, y);
        }
        if (h->cfg.attention) y = attention(y, ys, blk, level, &ab, local ? &fs : nullptr, pool_out);
        if (local) free(v);                        // (its statistics: released after the last launch that reads them is enqueued)
        return y;
    }
    // the network's first convolution (1 -> 64 stored channels, C_norm > 0 real ones) on the zero-padded trajectory x
    Value conv_in(const float* x, int C_norm = 0) {
        Value v0;
        v0.t = talloc(64, 0);
        v0.st = salloc(HWl(0), 64, HWl(0) / conv_in_parts(h->Hp, h->Wp, Bg()), 1, C_norm);
        v0.gamma = h->inc.gamma; v0.beta = h->inc.beta;
        if (!err && !dry)
            check(launch_conv_in(x, h->w_inc_first, v0.t.p, v0.st.p, B, h->cfg.horizon, h->cfg.state_dim, h->Hp, h->Wp,
                                 h->lh, h->lw, h->d_step, h->d_t, h->d_timesteps, h->n_steps, adv, s, Bg()), "conv_in");
        return v0;
    }
    // debug runs (arena.keep): the finished tensor of a value with a pending GroupNorm, as tap `name`
    void tap_gn(const char* name, const Value& v, int level) {
        if (!h->arena.keep) return;
        Tensor m = talloc(v.t.C, level);
        if (!dry && !err) check(launch_gn_apply(asrc(v), m.p, B, HWl(level), s), "gn_apply");
        tap(name, m);
    }
    int h_tcount = 1;
    PlanRoutes routes{};   // of this evaluation (plan_unet: choose_routes); routes.sa[5].outc: the plan's final tensor holds eps
                           // [B][H0][D] (outc applied by sa6's epilogue): StepArgs::eps_in
    int adv = -2;          // loop bookkeeping done by conv_in_kernel: -2 none, -1 advance, >= 0 set
};

// one U-Net evaluation on h->d_x... : x (B,H0,D) -> feat (B, Hp*Wp, 64)
static int plan_unet(Ctx& c, const float* x, bool use_cond, Tensor* feat_out, const PlanRoutes* sized) {
    spdm_handle* h = c.h;
    const int B = c.B;
    const PlanRoutes& r = c.routes = c.choose_routes(sized);       // every choice between kernels: the walk allocates and launches
    // ---- inc = DoubleConvolution(1, 64) on the zero-padded trajectory (:286-288) ----
    Value v0 = c.conv_in(x);
    // (pooled[i]: the input of down block i where its producer wrote it -- reserved before that launch)
    Tensor pooled[3];
    const bool pool1 = r.pool[0] == POOL_BY_PRODUCER;
    if (pool1) pooled[0] = c.talloc(64, 1);
    Value x1 = c.conv(v0, h->inc.second, 0, /*gelu=*/true, h->inc.gamma, h->inc.beta, pool1 ? &pooled[0] : nullptr);   // x1 = GN(raw), pending
    c.free(v0);
    c.tap_gn("x1", x1, 0);

    // ---- encoder: down1..3 (+ sa1..3) ----
    Value skips[3];            // x1 (pending GN), x2, x3 (materialised)
    skips[0] = x1;
    Value cur = x1;
    static const char* dn[3] = {"d1", "d2", "d3"};
    static const char* xn[3] = {"x2", "x3", "x4"};
    for (int i = 0; i < 3; ++i) {
        const int lin = i, lout = i + 1;
        // `cur` stays alive: it is a skip connection
        const DoubleConvW& dc1 = h->down[i].dc1;
        Value mid, fused;      // the block's first convolution, of MaxPool2d(2)(cur); or (routes.chain) all four of the block
        if (r.pool[i] == POOL_READ_THROUGH) {        // read through by that convolution (small grids)
            mid = c.conv_fused(PRO_POOL, cur, nullptr, dc1, lout);
            c.prof_begin();
        } else {
            // written by cur's producer -- raw with cur's GroupNorm pending (pool 1), or finished (pools 2 and 3) -- or by pool_kernel
            const bool by_producer = r.pool[i] == POOL_BY_PRODUCER;
            Value p;
            p.t = by_producer ? pooled[i] : c.talloc(cur.t.C, lout);
            if (!by_producer && !c.err && !c.dry)
                c.check(launch_pool(c.asrc(cur), p.t.p, B, c.Hl(lin), c.Wl(lin), c.s), "maxpool");
            c.prof_begin();
            if (i == 2 && r.chain[0]) {           // down block 3's four convolutions as one launch
                const DoubleConvW& dc2 = h->down[i].dc2;
                const ChainStep st[4] = {{&dc1.first, nullptr, nullptr, 0}, {&dc1.second, dc1.gamma, dc1.beta, 1},
                                         {&dc2.first, dc1.gamma, dc1.beta, 0}, {&dc2.second, dc2.gamma, dc2.beta, 1}};
                fused = c.conv_chain(p, st, 4, dc2.gamma, dc2.beta, lout);
            } else {
                mid = c.conv(p, dc1.first, lout, /*gelu=*/false, dc1.gamma, dc1.beta, nullptr, (by_producer && cur.pending_gn()) ? &cur : nullptr);
            }
            c.free(p);
        }
        Value b2;
        if (i == 2 && r.chain[0]) {
            b2 = fused;
        } else {
            Value a = c.conv(mid, dc1.second, lout, /*gelu=*/true, dc1.gamma, dc1.beta);
            c.free(mid);
            b2 = c.double_conv(a, h->down[i].dc2, lout);
        }
        c.prof_end();
        const Tensor y = c.film_attention(b2, h->down[i], i, lout, use_cond, dn[i],
                                          (i < 2 && r.pool[i + 1] == POOL_BY_PRODUCER) ? &pooled[i + 1] : nullptr);
        c.tap(xn[i], y);
        cur = Value{};             // (finished: nothing pending)
        cur.t = y;
        if (i < 2) skips[i + 1] = cur;
    }
    // ---- bottleneck (:297-299) ----
    c.prof_begin();
    Value x5;                                           // pending GN
    if (r.chain[1]) {                                   // the six convolutions as one launch
        const DoubleConvW* b = h->bot;
        const ChainStep st[6] = {{&b[0].first, nullptr, nullptr, 0}, {&b[0].second, b[0].gamma, b[0].beta, 1},
                                 {&b[1].first, b[0].gamma, b[0].beta, 0}, {&b[1].second, b[1].gamma, b[1].beta, 1},
                                 {&b[2].first, b[1].gamma, b[1].beta, 0}, {&b[2].second, b[2].gamma, b[2].beta, 1}};
        x5 = c.conv_chain(cur, st, 6, b[2].gamma, b[2].beta, 3);
        c.free(cur);
    } else {
        Value b1 = c.double_conv(cur, h->bot[0], 3);
        Value b2 = c.double_conv(b1, h->bot[1], 3);
        x5 = c.double_conv(b2, h->bot[2], 3);
    }
    c.prof_end();
    c.tap_gn("x5", x5, 3);
    // ---- decoder: up1..3 (+ sa4..6) ----
    static const char* un[3] = {"u1", "u2", "u3"};
    static const char* an[3] = {"a4", "a5", "a6"};
    cur = x5;
    for (int i = 0; i < 3; ++i) {
        const int lin = 3 - i, lout = 2 - i;
        Value& skip = skips[2 - i];
        const DoubleConvW& dc1 = h->up[i].dc1;
        Value mid;             // the block's first convolution, of cat([upsample x2 of cur, skip])
        if (r.up[i] == UP_READ_THROUGH) {
            mid = c.conv_fused(PRO_UPCAT, cur, &skip, dc1, lout);
            c.free(cur);         // upsample + concat read through by that convolution: released once its launch is enqueued
            c.free(skip);
            c.prof_begin();
        } else if (r.up[i] == UP_TWO_SOURCE) {
            // upsample only; the first conv reads [upsampled | skip] from the two tensors (no copy of the skip half)
            Tensor u2 = c.talloc(cur.t.C, lout);
            AffineSrc none{};
            if (!c.err && !c.dry) c.check(launch_upcat(c.asrc(cur), none, u2.p, B, c.Hl(lin), c.Wl(lin), c.s), "upsample");
            c.free(cur);
            c.prof_begin();
            mid = c.conv_two(u2, skip, dc1, lout);
            c.free(u2);
            c.free(skip);
        } else {
            Value cat;
            cat.t = c.talloc(cur.t.C + skip.t.C, lout);
            if (!c.err && !c.dry)
                c.check(launch_upcat(c.asrc(cur), c.asrc(skip), cat.t.p, B, c.Hl(lin), c.Wl(lin), c.s), "upsample+concat");
            c.free(cur);
            c.free(skip);
            c.prof_begin();
            mid = c.conv(cat, dc1.first, lout, /*gelu=*/false, dc1.gamma, dc1.beta);
            c.free(cat);
        }
        Value a = c.conv(mid, dc1.second, lout, /*gelu=*/true, dc1.gamma, dc1.beta);
        c.free(mid);
        Value b3 = c.double_conv(a, h->up[i].dc2, lout);
        c.prof_end();
        const Tensor y = c.film_attention(b3, h->up[i], 3 + i, lout, use_cond, un[i]);
        c.tap(an[i], y);
        cur = Value{};
        cur.t = y;
    }
    *feat_out = cur.t;
    return c.err;
}

// one evaluation of models/simple_Unet.py's UNet.forward (:282-300, y given; eval mode: no dropout on pe[t]) in channel-padded
// storage (ChanMap): x (B,H0,D) -> feat (B, Hp*Wp, 64) = up3's 32 channels + its 32 conditioning channels, what outc reads.
// Every resampling op is materialised (launch_pool / launch_upcat on finished tensors); the convolutions are launch_gemm's.
static int plan_simple(Ctx& c, const float* x, Tensor* feat_out) {
    spdm_handle* h = c.h;
    const int B = c.B;
    // DoubleConvolution.forward (:106-121) on the finished tensor `in`: two convs (GN + GELU of the first applied in the second's
    // load prologue), then y = GELU(GN(raw) + in) (residual) or GELU(GN(raw)).  Consumes `in`.
    auto dconv = [&](Tensor& in, const DoubleConvW& w, int level, bool residual) {
        Value vin;
        vin.t = in;
        Value raw = c.double_conv(vin, w, level, /*keep_in=*/true);
        Tensor y = c.talloc(raw.t.C, level);
        if (!c.err && !c.dry) c.check(launch_dc_finish(c.asrc(raw), residual ? in.p : nullptr, y.p, B, c.HWl(level), c.s), "dc_finish");
        c.free(raw);
        c.free(in);
        return y;
    };
    // DownSample / UpSample body after the resampling op (:160-176, :209-224).  Consumes `in`.
    auto block = [&](Tensor& in, int k, int level) {
        ResampleW& r = simple_block(h, k);
        Tensor a = dconv(in, r.dc1, level, /*residual=*/true);
        Value va;
        va.t = a;
        Value raw = c.double_conv(va, r.dc2, level);
        Tensor y = c.talloc(simple_out_width(k), level);
        if (!c.err && !c.dry)
            c.check(launch_simple_tail(c.asrc(raw), r.cout, r.temb_table, r.emb.out, h->d_t, c.h_tcount, h->d_cemb + SIMPLE_COND_CH * k,
                                       h->cemb.out, y.p, y.C, B, c.HWl(level), c.s), "simple block tail");
        c.free(raw);
        return y;
    };
    // ---- input_conv = DoubleConvolution(1, 16) on pad_to(x, 8) (:284,289) ----
    Value v0 = c.conv_in(x, /*C_norm=*/16);
    Value r0 = c.conv(v0, h->inc.second, 0, /*gelu=*/true, h->inc.gamma, h->inc.beta);
    c.free(v0);
    Tensor x1 = c.talloc(64, 0);
    if (!c.err && !c.dry) c.check(launch_dc_finish(c.asrc(r0), nullptr, x1.p, B, c.HWl(0), c.s), "dc_finish");
    c.free(r0);
    c.tap("x1", x1);
    // ---- down1..3 (:290-292): MaxPool2d(2) of the finished skip tensor, then the block ----
    static const char* xn[3] = {"x2", "x3", "x4"};
    Tensor skips[3] = {x1, Tensor{}, Tensor{}};
    Tensor cur = x1;
    for (int i = 0; i < 3; ++i) {
        Tensor p = c.talloc(cur.C, i + 1);
        Value vc;
        vc.t = cur;
        if (!c.err && !c.dry) c.check(launch_pool(c.asrc(vc), p.p, B, c.Hl(i), c.Wl(i), c.s), "maxpool");
        cur = block(p, i, i + 1);
        c.tap(xn[i], cur);
        if (i < 2) skips[i + 1] = cur;
    }
    // ---- up1..3 (:294-296): cat([Upsample(x2, bilinear, align_corners=True)(x), skip]), then the block ----
    static const char* un[3] = {"u1", "u2", "u3"};
    for (int i = 0; i < 3; ++i) {
        const int lin = 3 - i, lout = 2 - i;
        Tensor& skip = skips[2 - i];
        Tensor cat = c.talloc(cur.C + skip.C, lout);
        Value vu, vs;
        vu.t = cur;
        vs.t = skip;
        if (!c.err && !c.dry) c.check(launch_upcat(c.asrc(vu), c.asrc(vs), cat.p, B, c.Hl(lin), c.Wl(lin), c.s), "upsample+concat");
        c.free(cur);
        c.free(skip);
        cur = block(cat, 3 + i, lout);
        c.tap(un[i], cur);
    }
    *feat_out = cur;
    return c.err;
}

// sized: the sizing pass's combination of resampling routes (Ctx::choose_routes); null in a real run
static int plan_net(Ctx& c, const float* x, bool use_cond, Tensor* feat_out, const PlanRoutes* sized = nullptr) {
    return c.h->simple ? plan_simple(c, x, feat_out) : plan_unet(c, x, use_cond, feat_out, sized);
}

// The sizing pass: dry runs of the plan at max_batch for every combination of routes of the three pools and the three up blocks
// (3^6 walks: which one a real run takes depends on its batch); arena.peak ends as the largest of them (arena.dry must be set
// by the caller)
static int dry_plan_all(spdm_handle* h) {
    size_t peak = 0;
    // ... and, where the handle has fused level-3 chains (both sites switch at the same batch), with them on and off
    for (int k = 0; k < (h->simple ? 1 : 2 * 729); ++k) {     // (plan_simple materialises every resampling op)
        PlanRoutes want{};
        for (int op = 0, digits = k % 729; op < 6; ++op, digits /= 3) (op < 3 ? want.pool[op] : want.up[op - 3]) = digits % 3;
        want.chain[0] = want.chain[1] = k / 729;
        Ctx c{h, h->cfg.max_batch, nullptr, h->arena.dry};
        if (k >= 729) {
            const PlanRoutes got = c.choose_routes(&want);
            if (!got.chain[0] && !got.chain[1]) break;         // no site on this handle: the walks above cover it
        }
        h->arena.peak = 0;
        h->arena.reset();
        Tensor feat;
        const int rc = plan_net(c, h->d_x, /*use_cond=*/true, &feat, &want);
        if (rc != SPDM_OK) return rc;
        peak = std::max(peak, h->arena.peak);
    }
    h->arena.peak = peak;
    return SPDM_OK;
}

// time-embedding tables: Linear(SiLU(pos_encoding(t))) for every t (models/Unet_FiLmLayer.py:136-142)
static int ensure_temb(spdm_handle* h, hipStream_t s) {
    if (h->temb_ready) return SPDM_OK;
    const int T = h->cfg.num_train_timesteps, dim = h->cfg.time_dim;
    float* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, sizeof(float) * (size_t)T * dim));
    hipError_t e = hipMemcpyAsync(tmp, h->time_table.data(), sizeof(float) * (size_t)T * dim, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = launch_silu(tmp, h->d_time_silu, (size_t)T * dim, s);
    if (e == hipSuccess && h->d_time_pe)          // (SPDM_FLAG_TRAIN_SIMPLE: the raw rows the dropout multiplier scales)
        e = hipMemcpyAsync(h->d_time_pe, tmp, sizeof(float) * (size_t)T * dim, hipMemcpyDeviceToDevice, s);
    ResampleW* blocks[6] = {&h->down[0], &h->down[1], &h->down[2], &h->up[0], &h->up[1], &h->up[2]};
    for (int i = 0; i < 6 && e == hipSuccess; ++i)      // (N: cout, padded for simple_Unet.py)
        e = launch_gemm(linear_args(AffineSrc{h->d_time_silu, dim}, T, 0, blocks[i]->emb, h->split, h->sw, EPI_BIAS, blocks[i]->temb_table), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(SPDM_ERR_HIP, "time-embedding tables: %s", hipGetErrorString(e));
    h->temb_ready = true;
    return SPDM_OK;
}

// FiLM projections [scale | bias] = Linear(Mish(flatten(cond))) for the six resample blocks
// (models/Unet_FiLmLayer.py:149-154,171-175).  Step-invariant: hoisted out of the denoise loop.
static int compute_film(spdm_handle* h, int B, const float* d_cond, hipStream_t s) {
    h->have_film = false;
    if (!d_cond || h->cfg.cond_dim <= 0) return SPDM_OK;
    const AffineSrc condm{h->d_condm, h->film_kp};
    const int geom_M = (h->sw & SW_PIN_GEOMETRY) ? h->cfg.max_batch : 0;
    if (h->simple) {
        // models/simple_Unet.py: the six cond_emb_layer projections Linear(SiLU(flatten(cond))) (:146-150, :197-201) in ONE
        // GEMM over the stacked weights -> d_cemb [B][6 x 32]; step-invariant, hoisted out of the denoise loop like FiLM
        hipError_t e = launch_silu_pad(d_cond, h->d_condm, B, h->cfg.cond_dim, h->film_kp, s);
        if (e == hipSuccess) e = launch_gemm(linear_args(condm, B, geom_M, h->cemb, h->split, h->sw, EPI_BIAS, h->d_cemb), s);
        if (e != hipSuccess) return fail(SPDM_ERR_HIP, "conditioning projections: %s", hipGetErrorString(e));
        h->have_film = true;
        return SPDM_OK;
    }
    hipError_t e = launch_mish_pad(d_cond, h->d_condm, B, h->cfg.cond_dim, h->film_kp, s);
    ResampleW* blocks[6] = {&h->down[0], &h->down[1], &h->down[2], &h->up[0], &h->up[1], &h->up[2]};
    for (int i = 0; i < 6 && e == hipSuccess; ++i)
        e = launch_gemm(linear_args(condm, B, geom_M, blocks[i]->film, h->split, h->sw, EPI_BIAS, h->d_film[i]), s);
    if (e != hipSuccess) return fail(SPDM_ERR_HIP, "FiLM projections: %s", hipGetErrorString(e));
    h->have_film = true;
    return SPDM_OK;
}

static int check_ready(spdm_handle* h, int B) {
    if (!h) return fail(SPDM_ERR_INVALID, "null handle");
    if (!h->weights_loaded) return fail(SPDM_ERR_STATE, "spdm_load_weights has not been called");
    if (B < 1 || B > h->cfg.max_batch) return fail(SPDM_ERR_INVALID, "batch %d outside [1, max_batch = %d]", B, h->cfg.max_batch);
    return SPDM_OK;
}

static StepArgs step_args(spdm_handle* h, int B, const Tensor& feat, bool eps_ready) {
    StepArgs a{};
    a.feat = feat.p; a.w = h->outc_w; a.bias = h->outc_b; a.x = h->d_x; a.eps_out = nullptr;
    a.eps_in = eps_ready ? feat.p : nullptr;
    a.coef = h->d_coef; a.step_dev = h->d_step; a.kind = h->sched_kind;
    a.noise = h->s_noise; a.rng_dev = h->d_rng; a.flag_dev = h->d_step + 2;
    a.inpaint = h->s_inpaint; a.inp_h = h->s_inp_h; a.inpaint_per_sample = h->s_inp_per_sample;
    a.history = h->s_history;
    a.ptrs_dev = h->d_ptrs;
    a.B = B; a.H0 = h->cfg.horizon; a.D = h->cfg.state_dim; a.Hp = h->Hp; a.Wp = h->Wp; a.lh = h->lh; a.lw = h->lw;
    return a;
}

// spdm_unet_forward (h_t: the timesteps on the host, range-checked here) and spdm_unet_forward_dt (d_t: on the device, clamped
// into range by the kernel that copies them) are this one body; exactly one of h_t / d_t is set by the entries.
static int unet_forward(spdm_handle* h, int32_t B, const float* d_x, const int32_t* h_t, const int32_t* d_t, int32_t t_count,
                        const float* d_cond, float* d_eps, void* stream) {
    SPDM_TRY(check_ready(h, B));
    if (!d_x || (!h_t && !d_t) || !d_eps) return fail(SPDM_ERR_INVALID, "null argument");
    if (t_count != 1 && t_count != B) return fail(SPDM_ERR_INVALID, "t_count must be 1 or B");
    for (int i = 0; h_t && i < t_count; ++i)
        if (h_t[i] < 0 || h_t[i] >= h->cfg.num_train_timesteps) return fail(SPDM_ERR_INVALID, "t = %d outside [0,%d)", h_t[i], h->cfg.num_train_timesteps);
    if (h->simple && !d_cond) return fail(SPDM_ERR_INVALID, "d_cond is null: models/simple_Unet.py's UNet needs its conditioning");
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(ensure_temb(h, s));
    if (h_t) HIP_TRY(hipMemcpyAsync(h->d_t, h_t, sizeof(int) * t_count, hipMemcpyHostToDevice, s));
    else HIP_TRY(launch_copy_t_clamped(d_t, t_count, h->cfg.num_train_timesteps, h->d_t, s));
    HIP_TRY(hipMemsetAsync(h->d_step + 2, 0, sizeof(int), s));
    HIP_TRY(hipMemcpyAsync(h->d_x, d_x, sizeof(float) * (size_t)B * h->cfg.horizon * h->cfg.state_dim, hipMemcpyDeviceToDevice, s));
    SPDM_TRY(compute_film(h, B, d_cond, s));
    h->taps.clear();
    Ctx c{h, B, s, false};
    c.h_tcount = t_count;
    h->arena.reset();
    Tensor feat;
    SPDM_TRY(plan_net(c, h->d_x, d_cond != nullptr, &feat));
    StepArgs a = step_args(h, B, feat, c.routes.sa[5].outc);
    a.eps_out = d_eps;
    a.ptrs_dev = nullptr;
    HIP_TRY(launch_out_step(a, s));
    h->session = false;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int spdm_unet_forward(spdm_handle* h, int32_t B, const float* d_x, const int32_t* h_t, int32_t t_count,
                                 const float* d_cond, float* d_eps, void* stream) {
    return unet_forward(h, B, d_x, h_t, nullptr, t_count, d_cond, d_eps, stream);
}

extern "C" int spdm_unet_forward_dt(spdm_handle* h, int32_t B, const float* d_x, const int32_t* d_t, int32_t t_count,
                                    const float* d_cond, float* d_eps, void* stream) {
    return unet_forward(h, B, d_x, nullptr, d_t, t_count, d_cond, d_eps, stream);
}

extern "C" int spdm_sample_begin(spdm_handle* h, int32_t B, const float* d_cond, const float* d_inpaint, int32_t inp_h,
                                 int32_t inpaint_per_sample, const float* d_xT, const float* d_noise, uint64_t seed,
                                 uint64_t sample_offset, float* d_history, void* stream) {
    SPDM_TRY(check_ready(h, B));
    if (h->sched_kind < 0) return fail(SPDM_ERR_STATE, "no schedule set (spdm_set_schedule)");
    if (!d_xT) return fail(SPDM_ERR_INVALID, "d_xT is null");
    if (h->simple && !d_cond) return fail(SPDM_ERR_INVALID, "d_cond is null: models/simple_Unet.py's UNet needs its conditioning");
    if (inp_h < 0 || inp_h > h->cfg.horizon) return fail(SPDM_ERR_INVALID, "inpaint horizon %d outside [0,%d]", inp_h, h->cfg.horizon);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(ensure_temb(h, s));
    const size_t nx = (size_t)B * h->cfg.horizon * h->cfg.state_dim;
    HIP_TRY(hipMemcpyAsync(h->d_x, d_xT, sizeof(float) * nx, hipMemcpyDeviceToDevice, s));
    if (d_history) HIP_TRY(hipMemcpyAsync(d_history, d_xT, sizeof(float) * nx, hipMemcpyDeviceToDevice, s));
    SPDM_TRY(compute_film(h, B, d_cond, s));
    h->sB = B;
    h->s_inpaint = (inp_h > 0) ? d_inpaint : nullptr;
    h->s_inp_h = (d_inpaint != nullptr) ? inp_h : 0;
    h->s_inp_per_sample = inpaint_per_sample;
    h->s_noise = d_noise;
    h->s_history = d_history;
    h->s_seed = seed;
    h->s_offset = sample_offset;
    {   // the noise stream's key lives on the device (read by out_step_kernel), so a new seed does not change the step's launches
        const unsigned long long rng[2] = {seed, sample_offset};
        HIP_TRY(hipMemcpyAsync(h->d_rng, rng, sizeof(rng), hipMemcpyHostToDevice, s));
        const void* ptrs[4] = {h->s_inpaint, h->s_noise, h->s_history, nullptr};
        HIP_TRY(hipMemcpyAsync(h->d_ptrs, ptrs, sizeof(ptrs), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(h->d_step + 2, 0, sizeof(int), s));
    }
    h->session = true;
    h->s_last_step = -2;         // SPDM_DPMPP_2M: nothing of an earlier session's x0 is read
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

// one denoise iteration on stream s: loop bookkeeping (explicit index i >= 0, or "advance by one" for i < 0 --
// the form a captured graph replays), U-Net, fused 1x1 conv + scheduler update + inpainting
static int enqueue_step(spdm_handle* h, int i, hipStream_t s) {
    Ctx c{h, h->sB, s, false};
    c.h_tcount = 1;
    c.adv = (i >= 0) ? i : -1;          // the step's first kernel (conv_in_kernel) does the bookkeeping
    h->arena.reset();
    Tensor feat;
    SPDM_TRY(plan_net(c, h->d_x, h->have_film, &feat));
    StepArgs a = step_args(h, h->sB, feat, c.routes.sa[5].outc);
    if (h->sched_kind == SPDM_DPMPP_2M) {
        // the two-history-term update is a launch of its own: in out_step's place where sa6's epilogue has eps ready, after
        // out_step in its eps-only mode elsewhere
        SolverStepArgs v{};
        v.eps = a.eps_in;
        if (!c.routes.sa[5].outc) {
            a.eps_out = h->d_solver_eps;
            HIP_TRY(launch_out_step(a, s));
            v.eps = h->d_solver_eps;
        }
        v.x = h->d_x; v.x0_prev = h->d_x0_prev; v.coef = h->d_coef; v.step_dev = h->d_step; v.first_dev = h->d_first;
        v.flag_dev = h->d_step + 2; v.inp_h = h->s_inp_h; v.inpaint_per_sample = h->s_inp_per_sample; v.ptrs_dev = h->d_ptrs;
        v.B = h->sB; v.H0 = h->cfg.horizon; v.D = h->cfg.state_dim;
        HIP_TRY(launch_solver_step(v, s));
        return SPDM_OK;
    }
    HIP_TRY(launch_out_step(a, s));
    return SPDM_OK;
}

// Capture one step into a hipGraph (the step's ~70 launches take the same arguments in every iteration: the loop
// counter, the timestep and the noise offset live on the device).  Returns false -- with the stream usable and no
// error state left behind -- when the runtime refuses; the caller then stays on plain launches.
static bool build_step_graph(spdm_handle* h, hipStream_t s) {
    if (h->step_exec) { (void)hipDeviceSynchronize(); (void)hipGraphExecDestroy(h->step_exec); h->step_exec = nullptr; }
    if (h->step_graph) { (void)hipGraphDestroy(h->step_graph); h->step_graph = nullptr; }
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int rc = enqueue_step(h, -1, s);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc != SPDM_OK || e != hipSuccess || g == nullptr) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return false;
    }
    hipGraphExec_t ge = nullptr;
    if (hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) != hipSuccess || ge == nullptr) {
        (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return false;
    }
    h->step_graph = g;
    h->step_exec = ge;
    ++h->graph_captures;
    return true;
}

extern "C" int spdm_sample_run(spdm_handle* h, int32_t step_begin, int32_t step_end, void* stream) {
    if (!h || !h->session) return fail(SPDM_ERR_STATE, "spdm_sample_begin has not been called");
    if (step_begin < 0 || step_end > h->n_steps || step_begin > step_end)
        return fail(SPDM_ERR_INVALID, "step range [%d,%d) outside [0,%d]", step_begin, step_end, h->n_steps);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    // Graph replay (default; SPDM_NO_GRAPH=1 disables): not while the per-launch profiler or the debug taps are on.
    const bool graphs_on = !(h->sw & SW_NO_GRAPH);
    bool use_graph = graphs_on && !h->prof && !h->arena.keep && step_end - step_begin >= 3;
    if (use_graph && s == nullptr) {
        // the legacy NULL stream cannot be captured: run on a blocking stream of our own (implicitly ordered with
        // NULL-stream work on both sides) and keep the contract "NULL stream => complete on return"
        if (!h->gstream && hipStreamCreate(&h->gstream) != hipSuccess) { (void)hipGetLastError(); h->gstream = nullptr; use_graph = false; }
        if (use_graph) s = h->gstream;
    }
    if (h->sched_kind == SPDM_DPMPP_2M && step_begin < step_end) {
        // the first step of this range is first order unless the session has just completed the step before it: a device
        // word, written in stream order ahead of the launches, so that the captured step does not depend on the range
        const int first = (step_begin > 0 && h->s_last_step == step_begin - 1) ? -1 : step_begin;
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)h->d_first, first, 1, s));
        h->s_last_step = -2;     // (until every launch of the range has been enqueued)
    }
    int i = step_begin;
    if (use_graph) {
        SPDM_TRY(enqueue_step(h, i, s));         // first step: explicit index; also makes sure every kernel has been launched once
        ++i;
        spdm_handle::StepGraphKey key;
        key.B = h->sB; key.inp_h = h->s_inp_h; key.per_sample = h->s_inp_per_sample; key.have_film = h->have_film ? 1 : 0;
        key.sched_kind = h->sched_kind; key.n_steps = h->n_steps;
        key.env = h->sw;          // the captured launches depend on the kernel-selection switches (spdm_set_switch)
        if (!(h->step_exec && key == h->graph_key)) {
            if (build_step_graph(h, s)) h->graph_key = key;
            else use_graph = false;
        }
        if (use_graph)
            for (; i < step_end; ++i) HIP_TRY(hipGraphLaunch(h->step_exec, s));
    }
    for (; i < step_end; ++i) SPDM_TRY(enqueue_step(h, i, s));
    if (step_begin < step_end) h->s_last_step = step_end - 1;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int spdm_sample_result(spdm_handle* h, float* d_out, void* stream) {
    if (!h || !h->session) return fail(SPDM_ERR_STATE, "spdm_sample_begin has not been called");
    if (!d_out) return fail(SPDM_ERR_INVALID, "d_out is null");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(d_out, h->d_x, sizeof(float) * (size_t)h->sB * h->cfg.horizon * h->cfg.state_dim,
                           hipMemcpyDeviceToDevice, s));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int64_t spdm_graph_captures(const spdm_handle* h) { return h ? h->graph_captures : 0; }

extern "C" int spdm_nonfinite(spdm_handle* h, int32_t* flag_out, void* stream) {
    if (!h || !flag_out) return fail(SPDM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(h->cfg.device));
    int v = 0;
    HIP_TRY(hipMemcpyAsync(&v, h->d_step + 2, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *flag_out = v;
    return SPDM_OK;
}

extern "C" int spdm_sample(spdm_handle* h, int32_t B, const float* d_cond, const float* d_inpaint, int32_t inp_h,
                           int32_t inpaint_per_sample, const float* d_xT, const float* d_noise, uint64_t seed,
                           uint64_t sample_offset, float* d_out, float* d_history, void* stream) {
    // the three pieces run asynchronously on the caller's stream (or on a private one for NULL)
    hipStream_t s = (hipStream_t)stream;
    hipStream_t own = nullptr;
    if (!s) {
        if (h) (void)hipSetDevice(h->cfg.device);
        HIP_TRY(hipStreamCreate(&own));
        s = own;
    }
    int rc = spdm_sample_begin(h, B, d_cond, d_inpaint, inp_h, inpaint_per_sample, d_xT, d_noise, seed, sample_offset, d_history, s);
    if (rc == SPDM_OK) rc = spdm_sample_run(h, 0, h->n_steps, s);
    if (rc == SPDM_OK) rc = spdm_sample_result(h, d_out, s);
    if (own) {
        hipError_t e = hipStreamSynchronize(own);
        (void)hipStreamDestroy(own);
        if (rc == SPDM_OK && e != hipSuccess) rc = fail(SPDM_ERR_HIP, "stream sync: %s", hipGetErrorString(e));
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// Training-loss gradient of UNet_Film_noAttention (SPDM_FLAG_TRAIN, spdm_train_loss_grad), and of UNet_Film
// with SPDM_FLAG_TRAIN_ATTENTION (the SelfAttention blocks after each block tail: sa_fwd / sa_bwd, section 8.3).
// The forward half materialises every tensor the backward half reads -- each convolution's input (after GroupNorm + GELU, the
// pool or the upsample + concat), its raw output and the per-sample GroupNorm statistics -- in the handle's training workspace,
// a bump allocation whose size a dry run at max_batch fixed at create.  Convolutions and Linear layers are launches of the
// plan's implicit-GEMM kernels (gemm_args) on the exact fp32 path, the data gradients with the flipped (ConvW::wt) /
// transposed (LinW::wt) weight copies.  Training is exact-fp32 on any handle.  Weight gradients: launch_wgrad (train.hip).
struct TrainPass {
    spdm_handle* h;
    int B, t_count;
    bool use_cond, dry;
    hipStream_t s;
    float* d_grad;
    size_t used = 0;
    int err = SPDM_OK;
    static constexpr size_t WGRAD_BUDGET = (size_t)16 << 20;   // floats of weight-gradient partial slabs (64 MiB)
    float* partial = nullptr;
    int* iota = nullptr;                   // 0 .. B-1: the per-sample rows of temb[] (t_dev of the tail kernels)
    float* temb[6] = {};                   // Linear(SiLU(pos_encoding(t_b))) of the call, [B][C], exact fp32 path
    float* film[6] = {};                   // Linear(Mish(cond)) of the call, [B][2C], exact fp32 path
    const float* tscale = nullptr;         // SPDM_FLAG_TRAIN_SIMPLE: (B, time_dim) multiplier of pe[t_b] (spdm_train_set_time_scale)

    unsigned sw() const { return h->sw | SW_NO_SKINNY | SW_NO_REG64 | SW_NO_WIDE | SW_NO_SPLITK; }   // plain-epilogue launches: conv_gemm
    int Hl(int l) const { return h->Hp >> l; }
    int Wl(int l) const { return h->Wp >> l; }
    int HWl(int l) const { return Hl(l) * Wl(l); }
    float* alloc(size_t n) {
        float* p = dry ? nullptr : h->tws + used;
        used += align_up(std::max<size_t>(n, 1), 64);
        if (!dry && used > h->tws_floats && !err) err = fail(SPDM_ERR_NOMEM, "training workspace exhausted (batch %d)", B);
        return err ? nullptr : p;
    }
    bool run() const { return !dry && !err; }
    void chk(hipError_t e, const char* what) {
        if (e != hipSuccess && !err) err = fail(SPDM_ERR_HIP, "train: %s: %s", what, hipGetErrorString(e));
    }
    float* G(const std::string& name) {
        if (dry || err) return nullptr;
        auto it = h->grad_off.find(name);
        if (it == h->grad_off.end()) { err = fail(SPDM_ERR_MISSING, "train: tensor '%s' not in the loaded index", name.c_str()); return nullptr; }
        return d_grad + it->second;
    }

    // y = conv(x, w) on the exact fp32 path (the gradient is only as continuous as the MaxPool choices)
    void conv_fwd(const ConvW& w, const float* x, int level, float* y) {
        if (!run()) return;
        chk(launch_gemm(gemm_args(B * HWl(level), 0, Hl(level), Wl(level), w.cin, w.cout, w.taps, 0, sw(), nullptr, PRO_NONE,
                                  AffineSrc{x, w.cin}, 0, AffineSrc{}, w.w, nullptr, y, w.cout, EPI_PLAIN, nullptr), s),
            "conv forward");
    }
    // dx = conv(dy, rot180(w)^T): the forward kernels on the exact path
    void conv_dgrad(const ConvW& w, const float* dy, int level, float* dx) {
        if (!run()) return;
        if (!w.wt) { err = fail(SPDM_ERR_STATE, "train: flipped weights missing"); return; }
        chk(launch_gemm(gemm_args(B * HWl(level), 0, Hl(level), Wl(level), w.cout, w.cin, w.taps, 0, sw(), nullptr, PRO_NONE,
                                  AffineSrc{dy, w.cout}, 0, AffineSrc{}, w.wt, nullptr, dx, w.cin, EPI_PLAIN, nullptr), s),
            "conv data gradient");
    }
    void wgrad(const float* dy, int ldy, const float* x, int ldx, long long M, int level, int taps, int Co, int Ci, int conv9,
               float* dst) {
        if (!run() || !dst) return;
        chk(launch_wgrad(dy, ldy, x, ldx, M, taps == 1 ? 1 : Hl(level), taps == 1 ? 1 : Wl(level), taps, Co, Ci, conv9, partial,
                         WGRAD_BUDGET, dst, s), "weight gradient");
    }

    struct DC {                  // one DoubleConvolution's saved tensors
        const float* x0 = nullptr; int cin = 0, C = 0, level = 0;
        float *y1 = nullptr, *a1 = nullptr, *y2 = nullptr, *z = nullptr;
        float *m1 = nullptr, *r1 = nullptr, *m2 = nullptr, *r2 = nullptr;
    };
    DC dc_fwd(const DoubleConvW& d, const float* x0, int level, bool inc) {
        DC a;
        a.x0 = x0; a.cin = d.first.cin; a.C = d.first.cout; a.level = level;
        const size_t n = (size_t)B * HWl(level) * a.C;
        a.y1 = alloc(n); a.a1 = alloc(n); a.y2 = alloc(n); a.z = alloc(n);
        a.m1 = alloc(B); a.r1 = alloc(B); a.m2 = alloc(B); a.r2 = alloc(B);
        if (!run()) return a;
        const int HW = HWl(level);
        if (inc) chk(launch_conv_in_plain(x0, h->w_inc_first, B, Hl(level), Wl(level), a.y1, s), "inc.first");
        else conv_fwd(d.first, x0, level, a.y1);
        if (!run()) return a;
        chk(launch_gn_stats(a.y1, B, HW * a.C, a.m1, a.r1, s), "GroupNorm statistics");
        chk(launch_gn_act(a.y1, a.m1, a.r1, d.gamma, d.beta, B, HW, a.C, 1, a.a1, s), "GroupNorm + GELU");
        conv_fwd(d.second, a.a1, level, a.y2);
        if (!run()) return a;
        chk(launch_gn_stats(a.y2, B, HW * a.C, a.m2, a.r2, s), "GroupNorm statistics");
        chk(launch_gn_act(a.y2, a.m2, a.r2, d.gamma, d.beta, B, HW, a.C, 0, a.z, s), "GroupNorm");
        return a;
    }
    // dz: gradient of the block output; dx0 (null: not wanted) receives the gradient of its input
    void dc_bwd(const DC& a, const DoubleConvW& d, const std::string& p, const float* dz, float* dx0) {
        const int HW = HWl(a.level);
        const long long M = (long long)B * HW;
        const size_t n = (size_t)M * a.C;
        float* dy2 = alloc(n);
        float* da1 = alloc(n);
        float* dy1 = alloc(n);
        float* dgb2 = alloc((size_t)B * a.C * 2);
        float* dgb1 = alloc((size_t)B * a.C * 2);
        if (!run()) return;
        const int taps = d.second.taps;
        chk(launch_gn_bwd(a.y2, a.m2, a.r2, d.gamma, d.beta, dz, 0, B, HW, a.C, dy2, dgb2, s), "GroupNorm backward");
        wgrad(dy2, a.C, a.a1, a.C, M, a.level, taps, a.C, a.C, 1, G(p + ".second.weight"));
        conv_dgrad(d.second, dy2, a.level, da1);
        if (!run()) return;
        chk(launch_gn_bwd(a.y1, a.m1, a.r1, d.gamma, d.beta, da1, 1, B, HW, a.C, dy1, dgb1, s), "GroupNorm + GELU backward");
        float* dg = G(p + ".norm.weight");
        float* db = G(p + ".norm.bias");
        if (!run()) return;
        chk(launch_gn_param(dgb2, dgb1, B, a.C, dg, db, s), "GroupNorm affine gradient");
        wgrad(dy1, a.C, a.x0, a.cin, M, a.level, d.first.taps, a.C, a.cin, 1, G(p + ".first.weight"));
        if (dx0) conv_dgrad(d.first, dy1, a.level, dx0);
    }

    struct Block {               // a Down / UpSample block
        DC dc1, dc2;
        const float* in = nullptr;   // pooled or upsampled + concatenated input (dc1.x0)
        float* out = nullptr;
    };
    // x + Linear(SiLU(temb)), then FiLM
    float* film_fwd(int i, const ResampleW& r, const DC& dc2, int level) {
        float* out = alloc((size_t)B * HWl(level) * r.cout);
        if (run())
            chk(launch_film_apply(AffineSrc{dc2.z, r.cout}, temb[i], iota, B, use_cond ? film[i] : nullptr, out, nullptr, B,
                                  HWl(level), s), "time embedding + FiLM");
        return out;
    }
    // backward of the block tail; returns the gradient of dc2's output.  tsilu: SiLU(pos_encoding(t)) rows; dm: this block's
    // [B][cond_dim padded to 64] gradient of Mish(cond)
    float* film_bwd(int i, const ResampleW& r, const DC& dc2, const std::string& p, const float* dout, const float* tsilu,
                    float* dm) {
        const int C = r.cout, level = dc2.level;
        float* dz = alloc((size_t)B * HWl(level) * C);
        float* de = alloc((size_t)B * C);
        float* df = use_cond ? alloc((size_t)B * 2 * C) : nullptr;
        if (!run()) return dz;
        chk(launch_film_bwd(dc2.z, temb[i], iota, B, use_cond ? film[i] : nullptr, dout, B, HWl(level), C, dz, de, df, s),
            "FiLM backward");
        const int td = h->cfg.time_dim;
        wgrad(de, C, tsilu, td, B, 0, 1, C, td, 0, G(p + ".emb_layer.1.weight"));
        if (float* gb = G(p + ".emb_layer.1.bias"); run()) chk(launch_colsum(de, C, B, C, gb, s), "bias gradient");
        if (use_cond) {
            const int cd = h->cfg.cond_dim, kp64 = (int)align_up(cd, 64);
            wgrad(df, 2 * C, h->d_condm, h->film_kp, B, 0, 1, 2 * C, cd, 0, G(p + ".cond_encoder.2.weight"));
            if (float* gb = G(p + ".cond_encoder.2.bias"); run()) chk(launch_colsum(df, 2 * C, B, 2 * C, gb, s), "bias gradient");
            if (!run()) return dz;
            if (!r.film.wt) { err = fail(SPDM_ERR_STATE, "train: transposed FiLM weights missing"); return dz; }
            chk(launch_gemm(gemm_args(B, 0, 1, 1, 2 * C, kp64, 1, 0, sw(), nullptr, PRO_NONE, AffineSrc{df, 2 * C}, 0, AffineSrc{},
                                      r.film.wt, nullptr, dm, kp64, EPI_PLAIN, nullptr), s), "FiLM data gradient");
        }
        return dz;
    }

    // ---- SelfAttention (SPDM_FLAG_TRAIN_ATTENTION; models/Unet_FiLmLayer.py:71-82) ----
    // The block's tokens are the rows of its [B * HW][C] input, token-major already.  LN -> in_proj -> attention core -> out_proj
    // + x -> LN -> ff1 -> GELU -> ff2 + a, the Linears on the exact fp32 GEMM path, the core on train_attn.hip's fp32 kernel.
    static constexpr int HEADS = 4;        // nn.MultiheadAttention(C, 4)
    struct SA {                  // one block's saved tensors
        const float* x = nullptr; int C = 0, level = 0;
        float *y1 = nullptr, *m1 = nullptr, *r1 = nullptr;     // LayerNorm 1 output and row statistics
        float *qkv = nullptr, *o = nullptr, *lse = nullptr;    // in_proj output, attention core output, its log-sum-exp
        float *a = nullptr, *y2 = nullptr, *m2 = nullptr, *r2 = nullptr;   // out_proj(o) + x, LayerNorm 2
        float *u = nullptr, *gl = nullptr, *out = nullptr;     // ff1 output, GELU(u), block output
    };
    void lin_fwd(const LinW& w, const float* x, long long M, int epi, float* y, const float* resid = nullptr) {
        if (!run()) return;
        chk(launch_gemm(linear_args(AffineSrc{x, w.in}, (int)M, 0, w, false, sw(), epi, y, resid), s), "attention Linear");
    }
    // dx = dy W: the forward kernels with the transposed copy
    void lin_dgrad(const LinW& w, const float* dy, long long M, float* dx) {
        if (!run()) return;
        if (!w.wt) { err = fail(SPDM_ERR_STATE, "train: transposed attention weights missing"); return; }
        chk(launch_gemm(gemm_args((int)M, 0, 1, 1, w.out, w.in, 1, 0, sw(), nullptr, PRO_NONE, AffineSrc{dy, w.out}, 0, AffineSrc{},
                                  w.wt, nullptr, dx, w.in, EPI_PLAIN, nullptr), s), "attention Linear data gradient");
    }
    void lin_wb(const float* dy, const float* x, long long M, int Co, int Ci, const std::string& wn, const std::string& bn) {
        wgrad(dy, Co, x, Ci, M, 0, 1, Co, Ci, 0, G(wn));
        if (float* gb = G(bn); run()) chk(launch_colsum(dy, Co, M, Co, gb, s), "bias gradient");
    }
    void ln_param(const float* part, int nblk, int C, const std::string& gn, const std::string& bn) {
        float* dg = G(gn);
        float* db = G(bn);
        if (!run()) return;
        chk(launch_colsum(part, 2 * C, nblk, C, dg, s), "LayerNorm affine gradient");
        chk(launch_colsum(part + C, 2 * C, nblk, C, db, s), "LayerNorm affine gradient");
    }
    SA sa_fwd(int i, const float* x, int level) {
        const AttnW& w = h->sa[i];
        SA a;
        a.x = x; a.C = w.C; a.level = level;
        const long long M = (long long)B * HWl(level);
        const size_t n = (size_t)M * a.C;
        a.y1 = alloc(n); a.m1 = alloc(M); a.r1 = alloc(M);
        a.qkv = alloc(3 * n); a.o = alloc(n); a.lse = alloc((size_t)M * HEADS);
        a.a = alloc(n); a.y2 = alloc(n); a.m2 = alloc(M); a.r2 = alloc(M);
        a.u = alloc(n); a.gl = alloc(n); a.out = alloc(n);
        if (!run()) return a;
        chk(launch_ln_fwd(x, w.ln_g, w.ln_b, M, a.C, a.y1, a.m1, a.r1, s), "LayerNorm");
        lin_fwd(w.in_proj, a.y1, M, EPI_BIAS, a.qkv);
        if (run()) chk(launch_attn_fwd_lse(a.qkv, a.o, a.lse, B, HWl(level), a.C, HEADS, s), "attention core");
        lin_fwd(w.out_proj, a.o, M, EPI_BIAS_RESID, a.a, x);
        if (run()) chk(launch_ln_fwd(a.a, w.ff_ln_g, w.ff_ln_b, M, a.C, a.y2, a.m2, a.r2, s), "LayerNorm");
        lin_fwd(w.ff1, a.y2, M, EPI_BIAS, a.u);
        if (run()) chk(launch_gelu(a.u, a.gl, n, s), "GELU");
        lin_fwd(w.ff2, a.gl, M, EPI_BIAS_RESID, a.out, a.a);
        return a;
    }
    // dout: the gradient of the block output; returns the gradient of its input
    float* sa_bwd(int i, const SA& a, const float* dout) {
        const AttnW& w = h->sa[i];
        const std::string p = "sa" + std::to_string(i + 1);
        const long long M = (long long)B * HWl(a.level);
        const size_t n = (size_t)M * a.C;
        const int C = a.C, nblk = ln_bwd_blocks(M);
        float* dgl = alloc(n);
        float* du = alloc(n);
        float* dy2 = alloc(n);
        float* da = alloc(n);
        float* dob = alloc(n);
        float* dqkv = alloc(3 * n);
        float* dy1 = alloc(n);
        float* dx = alloc(n);
        float* part = alloc((size_t)nblk * 2 * C);
        if (!run()) return dx;
        lin_wb(dout, a.gl, M, C, C, p + ".ff_self.3.weight", p + ".ff_self.3.bias");
        lin_dgrad(w.ff2, dout, M, dgl);
        if (run()) chk(launch_gelu_bwd(a.u, dgl, n, du, s), "GELU backward");
        lin_wb(du, a.y2, M, C, C, p + ".ff_self.1.weight", p + ".ff_self.1.bias");
        lin_dgrad(w.ff1, du, M, dy2);
        if (run()) chk(launch_ln_bwd(a.a, a.m2, a.r2, w.ff_ln_g, dy2, dout, M, C, da, part, s), "LayerNorm backward");   // + residual
        ln_param(part, nblk, C, p + ".ff_self.0.weight", p + ".ff_self.0.bias");
        lin_wb(da, a.o, M, C, C, p + ".attention.out_proj.weight", p + ".attention.out_proj.bias");
        lin_dgrad(w.out_proj, da, M, dob);
        if (run()) chk(launch_attn_bwd(a.qkv, a.o, dob, a.lse, dqkv, B, HWl(a.level), C, HEADS, s), "attention core backward");
        lin_wb(dqkv, a.y1, M, 3 * C, C, p + ".attention.in_proj_weight", p + ".attention.in_proj_bias");
        lin_dgrad(w.in_proj, dqkv, M, dy1);
        if (run()) chk(launch_ln_bwd(a.x, a.m1, a.r1, w.ln_g, dy1, da, M, C, dx, part, s), "LayerNorm backward");        // + residual
        ln_param(part, nblk, C, p + ".ln.weight", p + ".ln.bias");
        return dx;
    }

    // ---- models/simple_Unet.py (SPDM_FLAG_TRAIN_SIMPLE) in channel-padded storage ----
    // A DoubleConvolution whose output channels (and GroupNorm lanes) follow the map mo (device copy pos); the residual one
    // (doubleConv1) ends in GELU(GN(y2) + x0) and saves the pre-activation.
    struct SDC {
        DC d;
        ChanMap mo;
        const int* pos = nullptr; int nreal = 0;
        bool residual = false;
        float* pre = nullptr;        // residual: GN(y2) + x0
    };
    // inc: input_conv (x0 the padded map, conv_in layout); tail: the block tail reads y2 itself (d.z is not materialised)
    SDC sdc_fwd(const DoubleConvW& w, const float* x0, int level, bool inc, bool residual, bool tail, const ChanMap& mo,
                const int* pos) {
        SDC a;
        DC& d = a.d;
        a.mo = mo; a.pos = pos; a.nreal = mo.real(); a.residual = residual;
        const int nreal = a.nreal;
        d.x0 = x0; d.cin = inc ? 1 : w.first.cin; d.C = inc ? 64 : w.first.cout; d.level = level;
        const int HW = HWl(level);
        const size_t n = (size_t)B * HW * d.C;
        d.y1 = alloc(n); d.a1 = alloc(n); d.y2 = alloc(n);
        d.z = tail ? nullptr : alloc(n);
        a.pre = residual ? alloc(n) : nullptr;
        d.m1 = alloc(B); d.r1 = alloc(B); d.m2 = alloc(B); d.r2 = alloc(B);
        if (!run()) return a;
        if (inc) chk(launch_conv_in_plain(x0, h->w_inc_first, B, Hl(level), Wl(level), d.y1, s), "input_conv.first");
        else conv_fwd(w.first, x0, level, d.y1);
        if (!run()) return a;
        chk(launch_gn_stats_real(d.y1, B, HW * d.C, HW * nreal, d.m1, d.r1, s), "GroupNorm statistics");
        chk(launch_gn_act(d.y1, d.m1, d.r1, w.gamma, w.beta, B, HW, d.C, 1, d.a1, s), "GroupNorm + GELU");
        conv_fwd(w.second, d.a1, level, d.y2);
        if (!run()) return a;
        chk(launch_gn_stats_real(d.y2, B, HW * d.C, HW * nreal, d.m2, d.r2, s), "GroupNorm statistics");
        if (residual) chk(launch_gn_res(d.y2, d.m2, d.r2, w.gamma, w.beta, x0, B, HW, d.C, a.pre, d.z, s), "GroupNorm + residual + GELU");
        else if (!tail) chk(launch_gn_act(d.y2, d.m2, d.r2, w.gamma, w.beta, B, HW, d.C, 1, d.z, s), "GroupNorm + GELU");
        return a;
    }
    // weight gradient of a padded 3x3 / 3x1 layer into its torch tensor: identity maps (real channels first) contract the real
    // channels only; a concatenation's map goes through launch_wgrad_mapped
    void wgrad_map(const float* dy, const float* x, int level, int taps, const ChanMap& mo, const int* po, const ChanMap& mi,
                   const int* pi, float* dst) {
        if (!run() || !dst) return;
        const long long M = (long long)B * HWl(level);
        auto ident = [](const ChanMap& m) { return m.pos.back() == m.real() - 1; };
        if (ident(mo) && ident(mi)) { wgrad(dy, mo.width, x, mi.width, M, level, taps, mo.real(), mi.real(), 1, dst); return; }
        chk(launch_wgrad_mapped(dy, x, M, Hl(level), Wl(level), taps, mo.width, mi.width, po, mo.real(), pi, mi.real(), partial,
                                WGRAD_BUDGET, dst, s), "weight gradient");
    }
    // dz: gradient of the DoubleConvolution's output (residual) or of GELU(GN(y2)) (otherwise); mi / pi: the map of its input.
    // dx0 (null: not wanted) receives the gradient of its input, the residual branch included.
    void sdc_bwd(const SDC& a, const DoubleConvW& w, const std::string& p, const float* dz, const ChanMap& mi, const int* pi,
                 float* dx0, bool inc = false) {
        const DC& d = a.d;
        const int HW = HWl(d.level);
        const long long M = (long long)B * HW;
        const size_t n = (size_t)M * d.C;
        const ChanMap& mo = a.mo;
        float* gpre = a.residual ? alloc(n) : nullptr;
        float* dy2 = alloc(n);
        float* da1 = alloc(n);
        float* dy1 = alloc(n);
        float* dgb2 = alloc((size_t)B * d.C * 2);
        float* dgb1 = alloc((size_t)B * d.C * 2);
        if (!run()) return;
        if (a.residual) {
            chk(launch_gelu_bwd(a.pre, dz, n, gpre, s), "residual GELU backward");
            chk(launch_gn_bwd_mapped(d.y2, d.m2, d.r2, w.gamma, w.beta, gpre, 0, B, HW, d.C, a.pos, a.nreal, dy2, dgb2, s),
                "GroupNorm backward");
        } else {
            chk(launch_gn_bwd_mapped(d.y2, d.m2, d.r2, w.gamma, w.beta, dz, 1, B, HW, d.C, a.pos, a.nreal, dy2, dgb2, s),
                "GroupNorm + GELU backward");
        }
        wgrad_map(dy2, d.a1, d.level, w.second.taps, mo, a.pos, mo, a.pos, G(p + ".second.weight"));
        conv_dgrad(w.second, dy2, d.level, da1);
        if (!run()) return;
        chk(launch_gn_bwd_mapped(d.y1, d.m1, d.r1, w.gamma, w.beta, da1, 1, B, HW, d.C, a.pos, a.nreal, dy1, dgb1, s),
            "GroupNorm + GELU backward");
        float* dg = G(p + ".norm.weight");
        float* db = G(p + ".norm.bias");
        if (!run()) return;
        chk(launch_gn_param_mapped(dgb2, dgb1, B, d.C, a.pos, a.nreal, dg, db, s), "GroupNorm affine gradient");
        if (inc) wgrad(dy1, d.C, d.x0, 1, M, d.level, 9, a.nreal, 1, 1, G(p + ".first.weight"));
        else wgrad_map(dy1, d.x0, d.level, w.first.taps, mo, a.pos, mi, pi, G(p + ".first.weight"));
        if (!dx0) return;
        conv_dgrad(w.first, dy1, d.level, dx0);
        if (a.residual && run()) chk(launch_add_cols(gpre, d.C, 0, M, d.C, dx0, s), "residual gradient");
    }
};

static const char* const kDown[3] = {"down1", "down2", "down3"};
static const char* const kUp[3] = {"up1", "up2", "up3"};
static const char* const kBot[3] = {"bot1", "bot2", "bot3"};

static int train_pass(TrainPass& T, const float* d_x, const float* d_cond, const float* d_noise, float* d_loss, float* d_eps,
                      float* d_grad_cond) {
    spdm_handle* h = T.h;
    const int B = T.B, H0 = h->cfg.horizon, D = h->cfg.state_dim;
    const long long M0 = (long long)B * T.HWl(0);
    T.partial = T.alloc(TrainPass::WGRAD_BUDGET);
    // time-embedding and FiLM projections of the call on the exact path (the sampling plan's tables follow the handle's
    // precision: a split-fp16 perturbation of 1e-6 already moves near-tie MaxPool choices)
    const int td = h->cfg.time_dim;
    float* tsilu = T.alloc((size_t)B * td);
    T.iota = (int*)T.alloc((size_t)B);
    if (T.run()) {
        std::vector<int> iota(B);
        for (int b = 0; b < B; ++b) iota[b] = b;
        T.chk(hipMemcpyAsync(T.iota, iota.data(), sizeof(int) * B, hipMemcpyHostToDevice, T.s), "iota");
        T.chk(hipStreamSynchronize(T.s), "iota");
        T.chk(launch_gather_rows(h->d_time_silu, h->d_t, T.t_count, B, td, tsilu, T.s), "time rows");
    }
    ResampleW* blocks[6] = {&h->down[0], &h->down[1], &h->down[2], &h->up[0], &h->up[1], &h->up[2]};
    for (int i = 0; i < 6; ++i) {
        const ResampleW& r = *blocks[i];
        T.temb[i] = T.alloc((size_t)B * r.cout);
        T.film[i] = T.use_cond ? T.alloc((size_t)B * 2 * r.cout) : nullptr;
        if (T.run())
            T.chk(launch_gemm(linear_args(AffineSrc{tsilu, td}, B, 0, r.emb, false, T.sw(), EPI_BIAS, T.temb[i]), T.s), "time embedding");
        if (T.run() && T.use_cond)
            T.chk(launch_gemm(linear_args(AffineSrc{h->d_condm, h->film_kp}, B, 0, r.film, false, T.sw(), EPI_BIAS, T.film[i]), T.s),
                  "FiLM projection");
    }
    // ---- forward ----
    float* xp = T.alloc((size_t)M0);
    if (T.run()) T.chk(launch_pad(d_x, B, H0, D, h->Hp, h->Wp, h->lh, h->lw, xp, T.s), "pad");
    const TrainPass::DC inc = T.dc_fwd(h->inc, xp, 0, true);
    const float* skips[4] = {inc.z, nullptr, nullptr, nullptr};     // x1 x2 x3 x4
    int skipC[4] = {64, 0, 0, 0};
    TrainPass::Block down[3], up[3];
    TrainPass::SA sa[6];                              // SPDM_FLAG_TRAIN_ATTENTION: sa1 .. sa6
    const bool attn = h->train_attn;
    for (int k = 0; k < 3; ++k) {
        const ResampleW& r = h->down[k];
        const int cin = r.dc1.first.cin, lv = k + 1;
        float* p = T.alloc((size_t)B * T.HWl(lv) * cin);
        if (T.run()) T.chk(launch_pool(AffineSrc{skips[k], cin}, p, B, T.Hl(k), T.Wl(k), T.s), "max pool");
        down[k].in = p;
        down[k].dc1 = T.dc_fwd(r.dc1, p, lv, false);
        down[k].dc2 = T.dc_fwd(r.dc2, down[k].dc1.z, lv, false);
        down[k].out = T.film_fwd(k, r, down[k].dc2, lv);
        if (attn) sa[k] = T.sa_fwd(k, down[k].out, lv);
        skips[k + 1] = attn ? sa[k].out : down[k].out;
        skipC[k + 1] = r.cout;
    }
    TrainPass::DC bot[3];
    const float* xb = skips[3];
    for (int k = 0; k < 3; ++k) { bot[k] = T.dc_fwd(h->bot[k], xb, 3, false); xb = bot[k].z; }
    const float* xin = xb;      // x5, then u1, u2
    int cu = 256;
    for (int k = 0; k < 3; ++k) {
        const ResampleW& r = h->up[k];
        const int lv = 2 - k, cs = skipC[2 - k], cin = r.dc1.first.cin;
        if (cu + cs != cin && !T.err) T.err = fail(SPDM_ERR_STATE, "train: up block %d has %d + %d input channels, weight expects %d", k, cu, cs, cin);
        float* c = T.alloc((size_t)B * T.HWl(lv) * cin);
        if (T.run()) T.chk(launch_upcat(AffineSrc{xin, cu}, AffineSrc{skips[2 - k], cs}, c, B, T.Hl(lv + 1), T.Wl(lv + 1), T.s), "upsample + concat");
        up[k].in = c;
        up[k].dc1 = T.dc_fwd(r.dc1, c, lv, false);
        up[k].dc2 = T.dc_fwd(r.dc2, up[k].dc1.z, lv, false);
        up[k].out = T.film_fwd(3 + k, r, up[k].dc2, lv);
        if (attn) sa[3 + k] = T.sa_fwd(3 + k, up[k].out, lv);
        xin = attn ? sa[3 + k].out : up[k].out;
        cu = r.cout;
    }
    float* eps_pad = T.alloc((size_t)M0);
    float* deps = T.alloc((size_t)M0);
    if (T.run()) T.chk(launch_outc(xin, h->outc_w, h->outc_b, M0, eps_pad, T.s), "outc");
    if (T.run()) T.chk(launch_mse(eps_pad, d_noise, B, H0, D, h->Hp, h->Wp, h->lh, h->lw, d_loss, deps, d_eps, T.s), "MSE loss");
    // ---- backward ----
    const int kp64 = (int)align_up(std::max(h->cfg.cond_dim, 1), 64);
    float* dm = T.alloc((size_t)6 * B * kp64);
    float* dskip[4];                                  // gradients of x1 .. x4 (accumulated: the pool and the skip both read them)
    for (int k = 0; k < 4; ++k) dskip[k] = T.alloc((size_t)B * T.HWl(k) * skipC[k]);
    float* dup[3];                                    // gradients of x5, u1, u2 (the coarse input of up block k)
    const int upC[3] = {256, h->up[0].cout, h->up[1].cout};
    for (int k = 0; k < 3; ++k) dup[k] = T.alloc((size_t)B * T.HWl(3 - k) * upC[k]);
    float* du3 = T.alloc((size_t)M0 * 64);
    if (T.run()) {
        T.chk(hipMemsetAsync(T.d_grad, 0, sizeof(float) * h->grad_floats, T.s), "memset");
        T.chk(hipMemsetAsync(dm, 0, sizeof(float) * 6 * B * kp64, T.s), "memset");
        for (int k = 0; k < 4; ++k) T.chk(hipMemsetAsync(dskip[k], 0, sizeof(float) * B * T.HWl(k) * skipC[k], T.s), "memset");
        for (int k = 0; k < 3; ++k) T.chk(hipMemsetAsync(dup[k], 0, sizeof(float) * B * T.HWl(3 - k) * upC[k], T.s), "memset");
        T.chk(launch_outc_bwd(deps, h->outc_w, M0, du3, T.s), "outc backward");
    }
    T.wgrad(deps, 1, xin, 64, M0, 0, 1, 1, 64, 0, T.G("outc.weight"));
    if (float* gb = T.G("outc.bias"); T.run()) T.chk(launch_colsum(deps, 1, M0, 1, gb, T.s), "bias gradient");
    const float* dout = du3;
    for (int k = 2; k >= 0; --k) {
        const ResampleW& r = h->up[k];
        const int lv = 2 - k, cs = skipC[2 - k], cin = r.dc1.first.cin, cuk = upC[k];
        const std::string p = kUp[k];
        if (attn) dout = T.sa_bwd(3 + k, sa[3 + k], dout);
        float* dz2 = T.film_bwd(3 + k, r, up[k].dc2, p, dout, tsilu, dm + (size_t)(3 + k) * B * kp64);
        float* dz1 = T.alloc((size_t)B * T.HWl(lv) * r.dc1.first.cout);
        float* dc = T.alloc((size_t)B * T.HWl(lv) * cin);
        T.dc_bwd(up[k].dc2, r.dc2, p + ".doubleConv2", dz2, dz1);
        T.dc_bwd(up[k].dc1, r.dc1, p + ".doubleConv1", dz1, dc);
        if (T.run()) {
            T.chk(launch_up_bwd(dc, cin, B, T.Hl(lv + 1), T.Wl(lv + 1), cuk, dup[k], T.s), "upsample backward");
            T.chk(launch_add_cols(dc, cin, cuk, (long long)B * T.HWl(lv), cs, dskip[2 - k], T.s), "concat backward");
        }
        dout = dup[k];
    }
    // dup[0] is the gradient of x5 = bot3's output
    const float* dbz = dup[0];
    for (int k = 2; k >= 0; --k) {
        float* dx = (k == 0) ? nullptr : T.alloc((size_t)B * T.HWl(3) * h->bot[k].first.cin);
        T.dc_bwd(bot[k], h->bot[k], kBot[k], dbz, k == 0 ? dskip[3] : dx);
        dbz = dx;
    }
    // bot1's input gradient went into dskip[3] -- which nothing else reads: copy semantics are enough (dskip[3] was zero)
    for (int k = 2; k >= 0; --k) {
        const ResampleW& r = h->down[k];
        const int lv = k + 1, cin = r.dc1.first.cin;
        const std::string p = kDown[k];
        const float* dfo = attn ? T.sa_bwd(k, sa[k], dskip[k + 1]) : dskip[k + 1];   // dskip[k + 1]: both readers of sa_{k+1}'s output
        float* dz2 = T.film_bwd(k, r, down[k].dc2, p, dfo, tsilu, dm + (size_t)k * B * kp64);
        float* dz1 = T.alloc((size_t)B * T.HWl(lv) * r.dc1.first.cout);
        float* dpool = T.alloc((size_t)B * T.HWl(lv) * cin);
        T.dc_bwd(down[k].dc2, r.dc2, p + ".doubleConv2", dz2, dz1);
        T.dc_bwd(down[k].dc1, r.dc1, p + ".doubleConv1", dz1, dpool);
        if (T.run()) T.chk(launch_pool_bwd(skips[k], dpool, B, T.Hl(k), T.Wl(k), cin, dskip[k], T.s), "max pool backward");
    }
    T.dc_bwd(inc, h->inc, "inc", dskip[0], nullptr);
    if (T.use_cond && d_grad_cond && T.run())
        T.chk(launch_mish_bwd(dm, 6, B, kp64, d_cond, h->cfg.cond_dim, d_grad_cond, T.s), "Mish backward");
    return T.err;
}

// Training-loss gradient of models/simple_Unet.py's UNet (SPDM_FLAG_TRAIN_SIMPLE), in the channel-padded storage
// of plan_simple: every saved tensor keeps exact zeros on its padded lanes, the GroupNorms count real channels
// only, and the weight gradients are gathered back to torch layout through the layers' channel maps.  The time rows are
// SiLU(pe[t_b] * scale_b) under spdm_train_set_time_scale (PositionalEncoding's dropout), the gathered SiLU(pe) rows otherwise.
static const char* const kSimpleNames[6] = {"down1", "down2", "down3", "up1", "up2", "up3"};

static int train_pass_simple(TrainPass& T, const float* d_x, const float* d_cond, const float* d_noise, float* d_loss,
                             float* d_eps, float* d_grad_cond) {
    spdm_handle* h = T.h;
    const int B = T.B, H0 = h->cfg.horizon, D = h->cfg.state_dim, td = h->cfg.time_dim, cd = h->cfg.cond_dim;
    const int NC = 6 * SIMPLE_COND_CH;
    const long long M0 = (long long)B * T.HWl(0);
    T.partial = T.alloc(TrainPass::WGRAD_BUDGET);
    // time rows, the six emb_layer projections and the stacked cond_emb_layer projection of the call, exact fp32
    float* tsilu = T.alloc((size_t)B * td);
    if (T.run()) {
        if (T.tscale) T.chk(launch_time_rows_scaled(h->d_time_pe, h->d_t, T.t_count, T.tscale, B, td, tsilu, T.s), "time rows");
        else T.chk(launch_gather_rows(h->d_time_silu, h->d_t, T.t_count, B, td, tsilu, T.s), "time rows");
    }
    for (int k = 0; k < 6; ++k) {       // (sized by the channel map: the dry run at create precedes spdm_load_weights)
        const ResampleW& r = simple_block(h, k);
        T.temb[k] = T.alloc((size_t)B * ChanMap::ident(kSimpleBlocks[k].cout).width);
        if (T.run() && r.emb.out != ChanMap::ident(kSimpleBlocks[k].cout).width)
            T.err = fail(SPDM_ERR_STATE, "train: emb_layer of block %d has %d outputs", k, r.emb.out);
        if (T.run())
            T.chk(launch_gemm(linear_args(AffineSrc{tsilu, td}, B, 0, r.emb, false, T.sw(), EPI_BIAS, T.temb[k]), T.s), "time embedding");
    }
    float* cemb = T.alloc((size_t)B * NC);            // [B][6 x 32]: block k's Linear(SiLU(cond)) at columns 32 k
    if (T.run())
        T.chk(launch_gemm(linear_args(AffineSrc{h->d_condm, h->film_kp}, B, 0, h->cemb, false, T.sw(), EPI_BIAS, cemb), T.s),
              "conditioning projection");
    // ---- forward ----
    struct SBlock { TrainPass::SDC dc1, dc2; float* out = nullptr; int aw = 0, bw = 0; };
    SBlock blk[6];
    const ChanMap c16 = ChanMap::ident(16);
    float* xp = T.alloc((size_t)M0);
    if (T.run()) T.chk(launch_pad(d_x, B, H0, D, h->Hp, h->Wp, h->lh, h->lw, xp, T.s), "pad");
    const TrainPass::SDC inc = T.sdc_fwd(h->inc, xp, 0, true, false, false, c16, h->d_pos16);
    const float* skips[4] = {inc.d.z, nullptr, nullptr, nullptr};     // x1 x2 x3 x4
    int skipW[4] = {c16.width, 0, 0, 0};
    auto block_fwd = [&](int k, const float* in, int lv) {
        const ResampleW& r = simple_block(h, k);
        const ChanMap mi = simple_in_map(k), mo = ChanMap::ident(kSimpleBlocks[k].cout);
        SBlock& b = blk[k];
        b.dc1 = T.sdc_fwd(r.dc1, in, lv, false, true, false, mi, h->d_pos_in[k]);
        b.dc2 = T.sdc_fwd(r.dc2, b.dc1.d.z, lv, false, false, true, mo, h->d_pos_out[k]);
        const int Wo = simple_out_width(k);
        b.out = T.alloc((size_t)B * T.HWl(lv) * Wo);
        if (T.run())
            T.chk(launch_simple_tail_fwd(b.dc2.d.y2, b.dc2.d.m2, b.dc2.d.r2, r.dc2.gamma, r.dc2.beta, mo.width, r.cout, T.temb[k],
                                         r.emb.out, cemb + SIMPLE_COND_CH * k, NC, B, T.HWl(lv), Wo, b.out, T.s), "block tail");
    };
    for (int k = 0; k < 3; ++k) {                     // down1..3: MaxPool2d(2), then the block
        const int lv = k + 1, w = simple_in_map(k).width;
        if (w != skipW[k] && !T.err) T.err = fail(SPDM_ERR_STATE, "train: down block %d reads %d channels, stored %d", k, w, skipW[k]);
        float* p = T.alloc((size_t)B * T.HWl(lv) * w);
        if (T.run()) T.chk(launch_pool(AffineSrc{skips[k], w}, p, B, T.Hl(k), T.Wl(k), T.s), "max pool");
        block_fwd(k, p, lv);
        skips[k + 1] = blk[k].out;
        skipW[k + 1] = simple_out_width(k);
    }
    const float* xin = skips[3];                      // x4, then u1, u2
    int xw = skipW[3];
    for (int k = 0; k < 3; ++k) {                     // up1..3: cat([Upsample(x), skip]), then the block
        const int lv = 2 - k, w = simple_in_map(3 + k).width;
        SBlock& b = blk[3 + k];
        b.aw = xw; b.bw = skipW[2 - k];
        if (b.aw + b.bw != w && !T.err) T.err = fail(SPDM_ERR_STATE, "train: up block %d has %d + %d input channels, map %d", k, b.aw, b.bw, w);
        float* c = T.alloc((size_t)B * T.HWl(lv) * w);
        if (T.run())
            T.chk(launch_upcat(AffineSrc{xin, b.aw}, AffineSrc{skips[2 - k], b.bw}, c, B, T.Hl(lv + 1), T.Wl(lv + 1), T.s), "upsample + concat");
        block_fwd(3 + k, c, lv);
        xin = b.out;
        xw = simple_out_width(3 + k);
    }
    if (xw != 64 && !T.err) T.err = fail(SPDM_ERR_STATE, "train: outc reads 64 channels, up3 stores %d", xw);
    float* eps_pad = T.alloc((size_t)M0);
    float* deps = T.alloc((size_t)M0);
    if (T.run()) T.chk(launch_outc(xin, h->outc_w, h->outc_b, M0, eps_pad, T.s), "outc");
    if (T.run()) T.chk(launch_mse(eps_pad, d_noise, B, H0, D, h->Hp, h->Wp, h->lh, h->lw, d_loss, deps, d_eps, T.s), "MSE loss");
    // ---- backward ----
    float* dcemb = T.alloc((size_t)B * NC);
    float* dskip[4];                                  // gradients of x1 .. x4 (accumulated: the pool / upsample and the skip read them)
    for (int k = 0; k < 4; ++k) dskip[k] = T.alloc((size_t)B * T.HWl(k) * skipW[k]);
    float* dup[3] = {dskip[3], nullptr, nullptr};     // gradients of x4, u1, u2 (the coarse input of up block k)
    for (int k = 1; k < 3; ++k) dup[k] = T.alloc((size_t)B * T.HWl(3 - k) * simple_out_width(2 + k));
    float* du3 = T.alloc((size_t)M0 * 64);
    if (T.run()) {
        T.chk(hipMemsetAsync(T.d_grad, 0, sizeof(float) * h->grad_floats, T.s), "memset");
        for (int k = 0; k < 4; ++k) T.chk(hipMemsetAsync(dskip[k], 0, sizeof(float) * B * T.HWl(k) * skipW[k], T.s), "memset");
        for (int k = 1; k < 3; ++k)
            T.chk(hipMemsetAsync(dup[k], 0, sizeof(float) * B * T.HWl(3 - k) * simple_out_width(2 + k), T.s), "memset");
        T.chk(launch_outc_bwd(deps, h->outc_w, M0, du3, T.s), "outc backward");
    }
    T.wgrad(deps, 1, xin, 64, M0, 0, 1, 1, 64, 0, T.G("outc.weight"));
    if (float* gb = T.G("outc.bias"); T.run()) T.chk(launch_colsum(deps, 1, M0, 1, gb, T.s), "bias gradient");
    // one block backward: tail, doubleConv2, doubleConv1; dout the gradient of the block output, din receives its input's
    auto block_bwd = [&](int k, const float* dout, int lv, float* din) {
        const ResampleW& r = simple_block(h, k);
        const SBlock& b = blk[k];
        const std::string p = kSimpleNames[k];
        const ChanMap mi = simple_in_map(k);
        const int Cz = b.dc2.mo.width, Cr = r.cout;
        const long long M = (long long)B * T.HWl(lv);
        float* dz2 = T.alloc((size_t)M * Cz);
        float* dtemb = T.alloc((size_t)B * Cr);
        float* dz1 = T.alloc((size_t)M * mi.width);
        if (T.run())
            T.chk(launch_simple_tail_bwd(dout, B, T.HWl(lv), simple_out_width(k), Cr, Cz, dz2, dtemb, dcemb + SIMPLE_COND_CH * k, NC, T.s),
                  "block tail backward");
        T.wgrad(dtemb, Cr, tsilu, td, B, 0, 1, Cr, td, 0, T.G(p + ".emb_layer.1.weight"));
        if (float* gb = T.G(p + ".emb_layer.1.bias"); T.run()) T.chk(launch_colsum(dtemb, Cr, B, Cr, gb, T.s), "bias gradient");
        T.sdc_bwd(b.dc2, r.dc2, p + ".doubleConv2", dz2, mi, h->d_pos_in[k], dz1);
        T.sdc_bwd(b.dc1, r.dc1, p + ".doubleConv1", dz1, mi, h->d_pos_in[k], din);
    };
    const float* dout = du3;
    for (int k = 2; k >= 0; --k) {
        const SBlock& b = blk[3 + k];
        const int lv = 2 - k, w = b.aw + b.bw;
        const long long M = (long long)B * T.HWl(lv);
        float* dc = T.alloc((size_t)M * w);
        block_bwd(3 + k, dout, lv, dc);
        if (T.run()) {
            T.chk(launch_up_bwd(dc, w, B, T.Hl(lv + 1), T.Wl(lv + 1), b.aw, dup[k], T.s), "upsample backward");
            T.chk(launch_add_cols(dc, w, b.aw, M, b.bw, dskip[2 - k], T.s), "concat backward");
        }
        dout = dup[k];
    }
    for (int k = 2; k >= 0; --k) {                    // dskip[k + 1] is complete: both readers of the block output are done
        const int lv = k + 1, w = skipW[k];
        float* dpool = T.alloc((size_t)B * T.HWl(lv) * w);
        block_bwd(k, dskip[k + 1], lv, dpool);
        if (T.run()) T.chk(launch_pool_bwd(skips[k], dpool, B, T.Hl(k), T.Wl(k), w, dskip[k], T.s), "max pool backward");
    }
    T.sdc_bwd(inc, h->inc, "input_conv", dskip[0], c16, h->d_pos16, nullptr, /*inc=*/true);
    // ---- conditioning: the six cond_emb_layer Linears on SiLU(cond), then d cond through the SiLU ----
    const int kp64 = (int)align_up((size_t)cd, 64);
    float* dsilu = T.alloc((size_t)B * kp64);
    for (int k = 0; k < 6; ++k) {
        const std::string p = kSimpleNames[k];
        T.wgrad(dcemb + SIMPLE_COND_CH * k, NC, h->d_condm, h->film_kp, B, 0, 1, SIMPLE_COND_CH, cd, 0, T.G(p + ".cond_emb_layer.1.weight"));
        if (float* gb = T.G(p + ".cond_emb_layer.1.bias"); T.run())
            T.chk(launch_colsum(dcemb + SIMPLE_COND_CH * k, NC, B, SIMPLE_COND_CH, gb, T.s), "bias gradient");
    }
    if (d_grad_cond && T.run()) {
        if (!h->cemb.wt) return T.err = fail(SPDM_ERR_STATE, "train: transposed conditioning weights missing");
        T.chk(launch_gemm(gemm_args(B, 0, 1, 1, NC, kp64, 1, 0, T.sw(), nullptr, PRO_NONE, AffineSrc{dcemb, NC}, 0, AffineSrc{},
                                    h->cemb.wt, nullptr, dsilu, kp64, EPI_PLAIN, nullptr), T.s), "conditioning data gradient");
        if (T.run()) T.chk(launch_silu_bwd(dsilu, kp64, d_cond, B, cd, d_grad_cond, T.s), "SiLU backward");
    }
    return T.err;
}

static size_t train_workspace_floats(spdm_handle* h) {
    TrainPass T{h, h->cfg.max_batch, 1, h->cfg.cond_dim > 0, true, nullptr, nullptr};
    if (h->train_simple) (void)train_pass_simple(T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    else (void)train_pass(T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return T.used;
}

// spdm_train_loss_grad (h_t: the timesteps on the host, range-checked here) and spdm_train_loss_grad_dt (d_t: on the device,
// clamped into range by the kernel that copies them) are this one body; exactly one of h_t / d_t is set by the entries.
static int train_loss_grad(spdm_handle* h, int32_t B, const float* d_x, const int32_t* h_t, const int32_t* d_t, int32_t t_count,
                           const float* d_cond, const float* d_noise, float* d_loss, float* d_eps, float* d_grad,
                           float* d_grad_cond, void* stream) {
    if (!h) return fail(SPDM_ERR_INVALID, "null handle");
    const float* tscale = h->t_scale;     // spdm_train_set_time_scale: consumed by this call, whatever its outcome
    const int tscale_B = h->t_scale_B;
    h->t_scale = nullptr;
    h->t_scale_B = 0;
    if (!h->train) return fail(SPDM_ERR_STATE, "spdm_train_loss_grad needs a handle created with SPDM_FLAG_TRAIN");
    SPDM_TRY(check_ready(h, B));
    if (!d_x || (!h_t && !d_t) || !d_noise || !d_loss || !d_grad) return fail(SPDM_ERR_INVALID, "null argument");
    if (h->simple && !d_cond) return fail(SPDM_ERR_INVALID, "SPDM_FLAG_SIMPLE_UNET: d_cond is required (simple_Unet.py's UNet is only defined with conditioning)");
    if (tscale && tscale_B != B)
        return fail(SPDM_ERR_INVALID, "spdm_train_set_time_scale was given %d rows, this call has B = %d", tscale_B, B);
    if (t_count != 1 && t_count != B) return fail(SPDM_ERR_INVALID, "t_count must be 1 or B");
    for (int i = 0; h_t && i < t_count; ++i)
        if (h_t[i] < 0 || h_t[i] >= h->cfg.num_train_timesteps) return fail(SPDM_ERR_INVALID, "t = %d outside [0,%d)", h_t[i], h->cfg.num_train_timesteps);
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(ensure_temb(h, s));
    if (h_t) HIP_TRY(hipMemcpyAsync(h->d_t, h_t, sizeof(int) * t_count, hipMemcpyHostToDevice, s));
    else HIP_TRY(launch_copy_t_clamped(d_t, t_count, h->cfg.num_train_timesteps, h->d_t, s));
    SPDM_TRY(compute_film(h, B, d_cond, s));
    TrainPass T{h, B, t_count, d_cond != nullptr && h->cfg.cond_dim > 0, false, s, d_grad};
    T.tscale = tscale;
    SPDM_TRY(h->train_simple ? train_pass_simple(T, d_x, d_cond, d_noise, d_loss, d_eps, d_grad_cond)
                             : train_pass(T, d_x, d_cond, d_noise, d_loss, d_eps, d_grad_cond));
    h->session = false;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int spdm_train_loss_grad(spdm_handle* h, int32_t B, const float* d_x, const int32_t* h_t, int32_t t_count,
                                    const float* d_cond, const float* d_noise, float* d_loss, float* d_eps, float* d_grad,
                                    float* d_grad_cond, void* stream) {
    return train_loss_grad(h, B, d_x, h_t, nullptr, t_count, d_cond, d_noise, d_loss, d_eps, d_grad, d_grad_cond, stream);
}

extern "C" int spdm_train_loss_grad_dt(spdm_handle* h, int32_t B, const float* d_x, const int32_t* d_t, int32_t t_count,
                                       const float* d_cond, const float* d_noise, float* d_loss, float* d_eps, float* d_grad,
                                       float* d_grad_cond, void* stream) {
    return train_loss_grad(h, B, d_x, nullptr, d_t, t_count, d_cond, d_noise, d_loss, d_eps, d_grad, d_grad_cond, stream);
}

// The forward (noising) process of a training step in one launch (include/spdm.h, train_noise.hip).  Stateless, like spdm_adam_step.
extern "C" int spdm_train_forward_process(int32_t device, const spdm_forward_process_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "forward_process: null argument");
    if (a->B < 1 || a->H < 1 || a->D < 1 || a->T < 1)
        return fail(SPDM_ERR_INVALID, "forward_process: B, H, D, T = %d, %d, %d, %d must all be >= 1", a->B, a->H, a->D, a->T);
    if ((long long)a->H * a->D > 0x7fffffffLL - 3)       // the kernel rounds H x D up to whole quads in int
        return fail(SPDM_ERR_INVALID, "forward_process: H x D does not fit 31 bits");
    if (a->d_time_scale && a->time_dim > 0x7fffffff - 3) return fail(SPDM_ERR_INVALID, "forward_process: time_dim does not fit 31 bits");
    if (a->inp_h < 0 || a->inp_h > a->H) return fail(SPDM_ERR_INVALID, "forward_process: inp_h = %d outside [0, H = %d]", a->inp_h, a->H);
    if (!a->d_x0 || !a->d_sqrt_abar || !a->d_sqrt_1m_abar || !a->d_x_noisy) return fail(SPDM_ERR_INVALID, "forward_process: null pointer");
    if ((a->inp_h > 0) != (a->d_inpaint != nullptr)) return fail(SPDM_ERR_INVALID, "forward_process: d_inpaint must be NULL exactly when inp_h == 0");
    if (!a->d_t_in && !a->d_t) return fail(SPDM_ERR_INVALID, "forward_process: d_t is required when the timesteps are drawn");
    if (!a->d_noise_in && !a->d_noise) return fail(SPDM_ERR_INVALID, "forward_process: d_noise is required when the noise is drawn");
    if (a->d_time_scale && a->time_dim < 1) return fail(SPDM_ERR_INVALID, "forward_process: time_dim = %d with d_time_scale set", a->time_dim);
    if (!(a->dropout_p >= 0.f && a->dropout_p < 1.f)) return fail(SPDM_ERR_INVALID, "forward_process: dropout_p = %g outside [0, 1)", (double)a->dropout_p);
    ForwardProcessArgs k = {};
    k.B = a->B; k.H = a->H; k.D = a->D; k.inp_h = a->inp_h; k.T = a->T;
    k.x0 = a->d_x0; k.inpaint = a->d_inpaint; k.sqrt_abar = a->d_sqrt_abar; k.sqrt_1m_abar = a->d_sqrt_1m_abar;
    k.seed = a->seed; k.sample_offset = a->sample_offset; k.step = a->step;
    k.t_in = a->d_t_in; k.noise_in = a->d_noise_in; k.t_out = a->d_t; k.noise_out = a->d_noise; k.x_noisy = a->d_x_noisy;
    k.time_scale = a->d_time_scale; k.time_dim = a->d_time_scale ? a->time_dim : 0;
    k.dropout_p = a->dropout_p;
    k.keep_scale = (float)(1.0 / (1.0 - (double)a->dropout_p));
    k.clamped = a->d_clamped;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_forward_process(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// A training batch gathered from device-resident stores in one launch (include/spdm.h, dataset.hip).  Stateless.
extern "C" int spdm_dataset_gather(int32_t device, const spdm_dataset_gather_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "dataset_gather: null argument");
    if (a->T < 1 || a->n_windows < 1 || a->B < 1 || a->seq_len < 1 || a->step_size < 1)
        return fail(SPDM_ERR_INVALID, "dataset_gather: T, n_windows, B, seq_len, step_size = %d, %d, %d, %d, %d must all be >= 1",
                    a->T, a->n_windows, a->B, a->seq_len, a->step_size);
    if (a->n_frames < 0 || a->n_frames > a->seq_len)
        return fail(SPDM_ERR_INVALID, "dataset_gather: n_frames = %d outside [0, seq_len = %d]", a->n_frames, a->seq_len);
    if (a->img_dtype != 0 && a->img_dtype != 1) return fail(SPDM_ERR_INVALID, "dataset_gather: img_dtype = %d is neither 0 (uint8) nor 1 (float32)", a->img_dtype);
    const long long span = (long long)(a->seq_len - 1) * a->step_size;       // rows between a window's first and last
    if (span >= a->T) return fail(SPDM_ERR_INVALID, "dataset_gather: a window spans %lld rows, the stores hold T = %d", span + 1, a->T);
    const long long max_start = a->T - 1 - span;
    if ((long long)a->B * a->seq_len > 0x7fffffffLL || (long long)a->B * a->n_frames * 3 > 0x7fffffffLL - 0x800000)
        return fail(SPDM_ERR_INVALID, "dataset_gather: B x seq_len does not fit 31 bits");
    if (!a->d_window_id) return fail(SPDM_ERR_INVALID, "dataset_gather: d_window_id is NULL");
    if ((a->n_frames > 0) != (a->d_image_out != nullptr)) return fail(SPDM_ERR_INVALID, "dataset_gather: d_image_out must be NULL exactly when n_frames == 0");
    if (a->d_image_out && !a->d_img) return fail(SPDM_ERR_INVALID, "dataset_gather: d_img is NULL");
    if (a->d_image_out && (((uintptr_t)a->d_img | (uintptr_t)a->d_image_out) & 15))
        return fail(SPDM_ERR_INVALID, "dataset_gather: d_img and d_image_out must be 16-byte aligned");
    if ((a->d_position_out || a->d_translation_out) && !a->d_position) return fail(SPDM_ERR_INVALID, "dataset_gather: d_position is NULL");
    if (a->d_velocity_out && !a->d_velocity) return fail(SPDM_ERR_INVALID, "dataset_gather: d_velocity is NULL");
    if (a->d_action_out && !a->d_action) return fail(SPDM_ERR_INVALID, "dataset_gather: d_action is NULL");
    if ((a->d_window_start != nullptr) != (a->h_window_start != nullptr))
        return fail(SPDM_ERR_INVALID, "dataset_gather: d_window_start and its host copy h_window_start go together");
    if (a->h_window_start) {
        for (int i = 0; i < a->n_windows; ++i)
            if (a->h_window_start[i] < 0 || a->h_window_start[i] > max_start)
                return fail(SPDM_ERR_INVALID, "dataset_gather: window %d starts at row %d: it must lie in [0, %lld] to end inside T = %d rows",
                            i, a->h_window_start[i], max_start, a->T);
    } else if (a->n_windows - 1 > max_start) {
        return fail(SPDM_ERR_INVALID, "dataset_gather: without a table window i starts at row i: n_windows = %d must be <= %lld", a->n_windows, max_start + 1);
    }
    DatasetGatherArgs k = {};
    k.n_windows = a->n_windows; k.B = a->B; k.seq_len = a->seq_len; k.step_size = a->step_size; k.n_frames = a->n_frames;
    k.img_dtype = a->img_dtype; k.max_start = (int)max_start;
    k.img = a->d_img; k.position = a->d_position; k.velocity = a->d_velocity; k.action = a->d_action;
    k.window_start = a->d_window_start; k.window_id = a->d_window_id; k.pos_min = a->pos_min; k.pos_max = a->pos_max;
    k.image_out = a->d_image_out; k.position_out = a->d_position_out; k.velocity_out = a->d_velocity_out; k.action_out = a->d_action_out;
    k.translation_out = a->d_translation_out; k.start_out = a->d_start_out; k.bad = a->d_bad;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_dataset_gather(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// Errors of sampled trajectories against their windows in one launch (include/spdm.h, evaluation.hip).  Stateless.
extern "C" int spdm_eval_errors(int32_t device, const spdm_eval_errors_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "eval_errors: null argument");
    if (a->B < 1 || a->P < 1 || a->runs < 1 || a->n_slots < 1 || a->seq < 1)
        return fail(SPDM_ERR_INVALID, "eval_errors: B, P, runs, n_slots, seq = %d, %d, %d, %d, %d must all be >= 1", a->B, a->P, a->runs,
                    a->n_slots, a->seq);
    if (a->obs_h < 0 || a->inp_h < 0) return fail(SPDM_ERR_INVALID, "eval_errors: obs_h = %d and inp_h = %d must be >= 0", a->obs_h, a->inp_h);
    if (a->inp_h > a->obs_h) return fail(SPDM_ERR_INVALID, "eval_errors: inp_h = %d exceeds obs_h = %d", a->inp_h, a->obs_h);
    if ((long long)a->H != (long long)a->inp_h + a->P) return fail(SPDM_ERR_INVALID, "eval_errors: H = %d is not inp_h + P = %d + %d", a->H, a->inp_h, a->P);
    if (a->D < 2 || (a->d_act_err && a->D < 5))
        return fail(SPDM_ERR_INVALID, "eval_errors: D = %d holds no %s", a->D, a->D < 2 ? "position (2 columns)" : "action (columns 2..4)");
    if ((long long)a->seq < (long long)a->obs_h + a->P) return fail(SPDM_ERR_INVALID, "eval_errors: seq = %d is shorter than obs_h + P = %d + %d", a->seq, a->obs_h, a->P);
    if ((long long)a->B * a->P > 0x7fffffffLL) return fail(SPDM_ERR_INVALID, "eval_errors: B x P does not fit 31 bits");
    if (!a->d_pred || !a->d_truth_pos || !a->d_translation || !a->d_pos_err) return fail(SPDM_ERR_INVALID, "eval_errors: null pointer");
    if (a->d_act_err && !a->d_truth_act) return fail(SPDM_ERR_INVALID, "eval_errors: d_act_err needs d_truth_act");
    if (a->first_traj < 0 || a->first_traj > INT64_MAX - a->B) return fail(SPDM_ERR_INVALID, "eval_errors: first_traj = %lld is negative or overflows", (long long)a->first_traj);
    const long long lo = a->first_traj / a->runs - a->window_base, hi = (a->first_traj + a->B - 1) / a->runs - a->window_base;
    if (lo < 0 || hi >= a->n_slots)
        return fail(SPDM_ERR_INVALID, "eval_errors: rows [%lld, %lld) at %d runs from window %d read slots [%lld, %lld], outside [0, n_slots = %d)",
                    (long long)a->first_traj, (long long)a->first_traj + a->B, a->runs, a->window_base, lo, hi, a->n_slots);
    EvalErrorsArgs k = {};
    k.B = a->B; k.H = a->H; k.D = a->D; k.seq = a->seq; k.obs_h = a->obs_h; k.inp_h = a->inp_h; k.P = a->P; k.runs = a->runs;
    k.first_traj = a->first_traj; k.window_base = a->window_base;
    k.pred = a->d_pred; k.truth_pos = a->d_truth_pos; k.truth_act = a->d_act_err ? a->d_truth_act : nullptr; k.translation = a->d_translation;
    k.pos_min = a->pos_min; k.pos_max = a->pos_max;
    for (int c = 0; c < 3; ++c) { k.act_min[c] = a->act_min[c]; k.act_max[c] = a->act_max[c]; }
    k.pos_err = a->d_pos_err; k.act_err = a->d_act_err;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_eval_errors(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

extern "C" size_t spdm_eval_reduce_workspace_doubles(int64_t N, int32_t C) {
    return (N < 1 || C < 1) ? 0 : (size_t)eval_reduce_blocks(N) * (size_t)C;
}

// Statistics of an error buffer per window and over all rows (include/spdm.h, evaluation.hip).  Stateless.
extern "C" int spdm_eval_reduce(int32_t device, const spdm_eval_reduce_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "eval_reduce: null argument");
    if (a->N < 1 || a->C < 1 || a->runs < 1)
        return fail(SPDM_ERR_INVALID, "eval_reduce: N, C, runs = %lld, %d, %d must all be >= 1", (long long)a->N, a->C, a->runs);
    if (a->N % a->runs != 0) return fail(SPDM_ERR_INVALID, "eval_reduce: N = %lld is not a multiple of runs = %d", (long long)a->N, a->runs);
    if (a->C > 65535) return fail(SPDM_ERR_INVALID, "eval_reduce: C = %d exceeds 65535", a->C);
    if (a->N > (1LL << 40)) return fail(SPDM_ERR_INVALID, "eval_reduce: N = %lld exceeds 2^40 rows", (long long)a->N);
    if (!a->d_err || !a->d_window_mean || !a->d_window_std || !a->d_mean || !a->d_std || !a->d_workspace)
        return fail(SPDM_ERR_INVALID, "eval_reduce: null pointer");
    const size_t need = spdm_eval_reduce_workspace_doubles(a->N, a->C);
    if (a->workspace_doubles < need)
        return fail(SPDM_ERR_INVALID, "eval_reduce: workspace of %llu doubles, %zu needed", (unsigned long long)a->workspace_doubles, need);
    EvalReduceArgs k = {};
    k.N = a->N; k.windows = a->N / a->runs; k.C = a->C; k.runs = a->runs;
    k.err = a->d_err; k.window_mean = a->d_window_mean; k.window_std = a->d_window_std; k.mean = a->d_mean; k.std = a->d_std;
    k.workspace = a->d_workspace;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_eval_reduce(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// Uniform noise on up to four observation tensors in one launch (include/spdm.h, obs_noise.hip).  Stateless.
extern "C" int spdm_obs_noise(int32_t device, const spdm_obs_noise_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "obs_noise: null argument");
    if (a->n_rows < 1) return fail(SPDM_ERR_INVALID, "obs_noise: n_rows = %lld must be >= 1", (long long)a->n_rows);
    if (a->n_tensors < 1 || a->n_tensors > OBS_NOISE_MAX_TENSORS)
        return fail(SPDM_ERR_INVALID, "obs_noise: n_tensors = %d outside [1, %d]", a->n_tensors, OBS_NOISE_MAX_TENSORS);
    if (a->row_offset < 0 || a->row_offset > (1LL << 32) || a->n_rows > (1LL << 32) - a->row_offset)
        return fail(SPDM_ERR_INVALID, "obs_noise: rows [%lld, %lld + %lld) do not fit 32 bits", (long long)a->row_offset,
                    (long long)a->row_offset, (long long)a->n_rows);
    if (!(a->alpha >= 0.f && a->alpha <= 3.402823466e+38f)) return fail(SPDM_ERR_INVALID, "obs_noise: alpha = %g must be finite and >= 0", (double)a->alpha);
    ObsNoiseArgs k = {};
    k.n_rows = (unsigned long long)a->n_rows; k.row_offset = (unsigned long long)a->row_offset; k.seed = a->seed; k.draw = a->draw;
    k.alpha = a->alpha; k.n_tensors = a->n_tensors;
    for (int i = 0; i < a->n_tensors; ++i) {
        const spdm_obs_noise_tensor& t = a->tensors[i];
        if (t.inner < 0) return fail(SPDM_ERR_INVALID, "obs_noise: tensor %d: inner = %lld is negative", i, (long long)t.inner);
        if (t.src_stride < t.inner || t.dst_stride < t.inner)
            return fail(SPDM_ERR_INVALID, "obs_noise: tensor %d: strides %lld and %lld are below inner = %lld", i, (long long)t.src_stride,
                        (long long)t.dst_stride, (long long)t.inner);
        if (t.inner / 4 + 1 > 0xffffffffLL) return fail(SPDM_ERR_INVALID, "obs_noise: tensor %d: inner = %lld holds more than 2^32 - 2 quads", i, (long long)t.inner);
        if (t.inner > 0 && (!t.d_src || !t.d_dst)) return fail(SPDM_ERR_INVALID, "obs_noise: tensor %d: null pointer", i);
        k.t[i].src = t.d_src; k.t[i].dst = t.d_dst; k.t[i].inner = t.inner; k.t[i].src_stride = t.src_stride; k.t[i].dst_stride = t.dst_stride;
    }
    if (!plan_obs_noise(k)) return fail(SPDM_ERR_INVALID, "obs_noise: the launch would exceed 2^31 - 1 workgroups of %d quads", OBS_NOISE_ITEMS);
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_obs_noise(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// One observation per environment into the history rings in one launch (include/spdm.h, policy.hip).  Stateless.
extern "C" int spdm_policy_push(int32_t device, const spdm_policy_push_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "policy_push: null argument");
    if (a->E < 1 || a->L < 1) return fail(SPDM_ERR_INVALID, "policy_push: E, L = %d, %d must both be >= 1", a->E, a->L);
    if ((long long)a->E * a->L > 0x7fffffffLL) return fail(SPDM_ERR_INVALID, "policy_push: E x L does not fit 31 bits");
    if (a->n < 0) return fail(SPDM_ERR_INVALID, "policy_push: n = %lld is negative", (long long)a->n);
    if (a->img_dtype != 0 && a->img_dtype != 1) return fail(SPDM_ERR_INVALID, "policy_push: img_dtype = %d is neither 0 (uint8) nor 1 (float32)", a->img_dtype);
    if (!a->d_img_in || !a->d_pos_in || !a->d_vel_in || !a->d_act_in || !a->d_fill || !a->d_ring_img || !a->d_ring_pos || !a->d_ring_vel ||
        !a->d_ring_act)
        return fail(SPDM_ERR_INVALID, "policy_push: null pointer");
    if (((uintptr_t)a->d_img_in | (uintptr_t)a->d_ring_img) & 15) return fail(SPDM_ERR_INVALID, "policy_push: d_img_in and d_ring_img must be 16-byte aligned");
    PolicyPushArgs k = {};
    k.E = a->E; k.L = a->L; k.img_dtype = a->img_dtype; k.slot = (int)(a->n % a->L);
    k.img_in = a->d_img_in; k.pos_in = a->d_pos_in; k.vel_in = a->d_vel_in; k.act_in = a->d_act_in; k.fill = a->d_fill;
    k.ring_img = a->d_ring_img; k.ring_pos = a->d_ring_pos; k.ring_vel = a->d_ring_vel; k.ring_act = a->d_ring_act;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_push(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// The conditioning batch of the observation history in one launch (include/spdm.h, policy.hip).  Stateless.
extern "C" int spdm_policy_window(int32_t device, const spdm_policy_window_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "policy_window: null argument");
    if (a->E < 1 || a->L < 1 || a->obs_h < 1 || a->step_size < 1)
        return fail(SPDM_ERR_INVALID, "policy_window: E, L, obs_h, step_size = %d, %d, %d, %d must all be >= 1", a->E, a->L, a->obs_h, a->step_size);
    if ((long long)(a->obs_h - 1) * a->step_size >= a->L)
        return fail(SPDM_ERR_INVALID, "policy_window: %d entries %d slots apart do not fit a ring of L = %d", a->obs_h, a->step_size, a->L);
    if ((long long)a->E * a->L > 0x7fffffffLL || (long long)a->E * a->obs_h * 3 > 0x7fffffffLL - 0x800000)
        return fail(SPDM_ERR_INVALID, "policy_window: E x L or E x obs_h does not fit 31 bits");
    if (a->n < 1) return fail(SPDM_ERR_INVALID, "policy_window: n = %lld: nothing has been pushed", (long long)a->n);
    if (a->img_dtype != 0 && a->img_dtype != 1) return fail(SPDM_ERR_INVALID, "policy_window: img_dtype = %d is neither 0 (uint8) nor 1 (float32)", a->img_dtype);
    if (a->stats_f32 < 0 || a->stats_f32 > 3) return fail(SPDM_ERR_INVALID, "policy_window: stats_f32 = %d outside [0, 3]", a->stats_f32);
    if (!a->d_image_out && !a->d_position_out && !a->d_velocity_out && !a->d_action_out && !a->d_translation_out)
        return fail(SPDM_ERR_INVALID, "policy_window: no output requested");
    if (a->d_image_out && !a->d_ring_img) return fail(SPDM_ERR_INVALID, "policy_window: d_ring_img is NULL");
    if (a->d_image_out && (((uintptr_t)a->d_ring_img | (uintptr_t)a->d_image_out) & 15))
        return fail(SPDM_ERR_INVALID, "policy_window: d_ring_img and d_image_out must be 16-byte aligned");
    if ((a->d_position_out || a->d_translation_out) && !a->d_ring_pos) return fail(SPDM_ERR_INVALID, "policy_window: d_ring_pos is NULL");
    if (a->d_velocity_out && !a->d_ring_vel) return fail(SPDM_ERR_INVALID, "policy_window: d_ring_vel is NULL");
    if (a->d_action_out && !a->d_ring_act) return fail(SPDM_ERR_INVALID, "policy_window: d_ring_act is NULL");
    PolicyWindowArgs k = {};
    k.E = a->E; k.L = a->L; k.obs_h = a->obs_h; k.step_size = a->step_size; k.img_dtype = a->img_dtype; k.first = (int)(a->n % a->L);
    k.vel_f32 = a->stats_f32 & 1; k.act_f32 = (a->stats_f32 >> 1) & 1;
    k.ring_img = a->d_ring_img; k.ring_pos = a->d_ring_pos; k.ring_vel = a->d_ring_vel; k.ring_act = a->d_ring_act;
    k.pos_min = a->pos_min; k.pos_max = a->pos_max;
    for (int c = 0; c < 2; ++c) { k.vel_min[c] = a->vel_min[c]; k.vel_max[c] = a->vel_max[c]; }
    for (int c = 0; c < 3; ++c) { k.act_min[c] = a->act_min[c]; k.act_max[c] = a->act_max[c]; }
    k.image_out = a->d_image_out; k.position_out = a->d_position_out; k.velocity_out = a->d_velocity_out; k.action_out = a->d_action_out;
    k.translation_out = a->d_translation_out;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_window(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// The sampler's x_0 as way-points and actions in the dataset's units in one launch (include/spdm.h, policy.hip).  Stateless.
extern "C" int spdm_policy_unnormalize(int32_t device, const spdm_policy_unnormalize_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "policy_unnormalize: null argument");
    if (a->E < 1) return fail(SPDM_ERR_INVALID, "policy_unnormalize: E = %d must be >= 1", a->E);
    if (a->inp_h < 0 || a->H <= a->inp_h) return fail(SPDM_ERR_INVALID, "policy_unnormalize: inp_h = %d outside [0, H = %d)", a->inp_h, a->H);
    if (a->D < 2 || (a->d_actions && a->D < 5))
        return fail(SPDM_ERR_INVALID, "policy_unnormalize: D = %d holds no %s", a->D, a->D < 2 ? "position (2 columns)" : "action (columns 2..4)");
    if ((long long)a->E * (a->H - a->inp_h) > 0x7fffffffLL) return fail(SPDM_ERR_INVALID, "policy_unnormalize: E x P does not fit 31 bits");
    if (!a->d_x0 || !a->d_translation || !a->d_waypoints) return fail(SPDM_ERR_INVALID, "policy_unnormalize: null pointer");
    PolicyUnnormalizeArgs k = {};
    k.E = a->E; k.H = a->H; k.D = a->D; k.inp_h = a->inp_h; k.x0 = a->d_x0; k.translation = a->d_translation;
    k.pos_min = a->pos_min; k.pos_max = a->pos_max;
    for (int c = 0; c < 3; ++c) { k.act_min[c] = a->act_min[c]; k.act_max[c] = a->act_max[c]; }
    k.waypoints = a->d_waypoints; k.actions = a->d_actions;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_unnormalize(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// The starting iterate of a warm-started plan in one launch (include/spdm.h, policy.hip).  Stateless.
extern "C" int spdm_policy_warm_start(int32_t device, const spdm_policy_warm_start_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "policy_warm_start: null argument");
    if (a->E < 1 || a->H < 1 || a->step_size < 1)
        return fail(SPDM_ERR_INVALID, "policy_warm_start: E, H, step_size = %d, %d, %d must all be >= 1", a->E, a->H, a->step_size);
    if (a->D < 2) return fail(SPDM_ERR_INVALID, "policy_warm_start: D = %d holds no position (2 columns)", a->D);
    if (a->inp_h < 0 || a->inp_h > a->H) return fail(SPDM_ERR_INVALID, "policy_warm_start: inp_h = %d outside [0, H = %d]", a->inp_h, a->H);
    if ((a->d_inpaint != nullptr) != (a->inp_h > 0))
        return fail(SPDM_ERR_INVALID, "policy_warm_start: d_inpaint must be NULL exactly when inp_h == 0 (inp_h = %d)", a->inp_h);
    if (a->delta < 0) return fail(SPDM_ERR_INVALID, "policy_warm_start: delta = %lld is negative", (long long)a->delta);
    if ((long long)a->H * a->D > 0x7fffffffLL || (long long)a->E * a->H * a->D > 0x7fffffffLL)
        return fail(SPDM_ERR_INVALID, "policy_warm_start: E x H x D does not fit 31 bits");
    if (!(fabsf(a->sa) <= 3.402823466e+38f) || !(fabsf(a->sb) <= 3.402823466e+38f))
        return fail(SPDM_ERR_INVALID, "policy_warm_start: sa, sb = %g, %g must be finite", (double)a->sa, (double)a->sb);
    if (!a->d_prev_x0 || !a->d_prev_translation || !a->d_translation || !a->d_x) return fail(SPDM_ERR_INVALID, "policy_warm_start: null pointer");
    PolicyWarmStartArgs k = {};
    k.E = a->E; k.H = a->H; k.D = a->D; k.inp_h = a->inp_h; k.step_size = a->step_size;
    const long long q = a->delta / a->step_size;         // rows the old plan is ahead; from H - 1 on every row is the held last one
    k.q = (int)(q < a->H - 1 ? q : a->H - 1);
    k.f = (int)(a->delta % a->step_size);
    k.sa = a->sa; k.sb = a->sb; k.seed = a->seed; k.env_offset = a->env_offset; k.draw = a->draw;
    k.prev_x0 = a->d_prev_x0; k.prev_translation = a->d_prev_translation; k.translation = a->d_translation;
    k.inpaint = a->d_inpaint; k.noise_in = a->d_noise_in; k.x = a->d_x; k.guess = a->d_guess; k.noise = a->d_noise;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_warm_start(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// One of K candidate plans per environment, its index, the scores and the spread in one launch (include/spdm.h, policy.hip).
// Stateless.
extern "C" int spdm_policy_select(int32_t device, const spdm_policy_select_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "policy_select: null argument");
    if (a->E < 1) return fail(SPDM_ERR_INVALID, "policy_select: E = %d must be >= 1", a->E);
    if (a->K < 1 || a->K > POLICY_SELECT_MAX_K) return fail(SPDM_ERR_INVALID, "policy_select: K = %d outside [1, %d]", a->K, POLICY_SELECT_MAX_K);
    if (a->inp_h < 0 || a->H <= a->inp_h) return fail(SPDM_ERR_INVALID, "policy_select: inp_h = %d outside [0, H = %d)", a->inp_h, a->H);
    if (a->D < 2) return fail(SPDM_ERR_INVALID, "policy_select: D = %d holds no position (2 columns)", a->D);
    if (a->cols < 2 || a->cols > a->D) return fail(SPDM_ERR_INVALID, "policy_select: cols = %d outside [2, D = %d]", a->cols, a->D);
    if (a->mode != SPDM_SELECT_MEDOID && a->mode != SPDM_SELECT_COHERENT)
        return fail(SPDM_ERR_INVALID, "policy_select: mode = %d is neither SPDM_SELECT_MEDOID nor SPDM_SELECT_COHERENT", a->mode);
    if (a->mode == SPDM_SELECT_COHERENT) {
        if (!a->d_guess) return fail(SPDM_ERR_INVALID, "policy_select: COHERENT needs d_guess: null pointer");
        if (a->rows < 1 || a->rows > a->H - a->inp_h)
            return fail(SPDM_ERR_INVALID, "policy_select: rows = %d outside [1, H - inp_h = %d]", a->rows, a->H - a->inp_h);
        if (a->guess_row_stride < 1)
            return fail(SPDM_ERR_INVALID, "policy_select: guess_row_stride = %lld must be >= 1", (long long)a->guess_row_stride);
    } else if (a->d_guess || a->rows != 0) {
        return fail(SPDM_ERR_INVALID, "policy_select: MEDOID takes no d_guess and rows = 0 (rows = %d)", a->rows);
    }
    if (a->d_spread && !a->d_translation) return fail(SPDM_ERR_INVALID, "policy_select: d_spread needs d_translation");
    const long long HD = (long long)a->H * a->D, EK = (long long)a->E * a->K;      // each < 2^62
    if (HD > 0x7fffffffLL || EK > 0x7fffffffLL || EK * HD > 0x7fffffffLL)
        return fail(SPDM_ERR_INVALID, "policy_select: E x K x H x D does not fit 31 bits");
    if (!a->d_x0 || !a->d_chosen || !a->d_x0_out) return fail(SPDM_ERR_INVALID, "policy_select: null pointer");
    const uintptr_t in0 = (uintptr_t)a->d_x0, in1 = in0 + (uintptr_t)(EK * HD) * sizeof(float);
    const uintptr_t out0 = (uintptr_t)a->d_x0_out, out1 = out0 + (uintptr_t)((long long)a->E * HD) * sizeof(float);
    if (out0 < in1 && in0 < out1) return fail(SPDM_ERR_INVALID, "policy_select: d_x0_out overlaps d_x0");
    PolicySelectArgs k = {};
    k.E = a->E; k.K = a->K; k.H = a->H; k.D = a->D; k.inp_h = a->inp_h; k.cols = a->cols; k.mode = a->mode; k.rows = a->rows;
    k.guess_row_stride = a->guess_row_stride;
    k.x0 = a->d_x0; k.guess = a->d_guess; k.translation = a->d_translation; k.pos_min = a->pos_min; k.pos_max = a->pos_max;
    k.chosen = a->d_chosen; k.x0_out = a->d_x0_out; k.scores = a->d_scores; k.spread = a->d_spread;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_policy_select(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// One DPM-Solver++ (2M) update on the caller's buffers (include/spdm.h, elementwise.hip): the launch the SPDM_DPMPP_2M loop
// makes after every noise prediction.  Stateless.
extern "C" int spdm_solver_step(int32_t device, const spdm_solver_step_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "solver_step: null argument");
    if (a->B < 1 || a->H < 1 || a->D < 1 || a->n_steps < 1)
        return fail(SPDM_ERR_INVALID, "solver_step: B, H, D, n_steps = %d, %d, %d, %d must all be >= 1", a->B, a->H, a->D, a->n_steps);
    if ((long long)a->H * a->D > 0x7fffffffLL || (long long)a->B * a->H * a->D > 0x7fffffffLL)
        return fail(SPDM_ERR_INVALID, "solver_step: B x H x D does not fit 31 bits");
    if (a->inp_h < 0 || a->inp_h > a->H) return fail(SPDM_ERR_INVALID, "solver_step: inp_h = %d outside [0, H = %d]", a->inp_h, a->H);
    if ((a->d_inpaint != nullptr) != (a->inp_h > 0))
        return fail(SPDM_ERR_INVALID, "solver_step: d_inpaint must be NULL exactly when inp_h == 0 (inp_h = %d)", a->inp_h);
    if (a->inpaint_per_sample != 0 && a->inpaint_per_sample != 1)
        return fail(SPDM_ERR_INVALID, "solver_step: inpaint_per_sample = %d must be 0 or 1", a->inpaint_per_sample);
    if (a->step < 0 || a->step >= a->n_steps) return fail(SPDM_ERR_INVALID, "solver_step: step %d outside [0, n_steps = %d)", a->step, a->n_steps);
    if (a->first < -1 || a->first >= a->n_steps) return fail(SPDM_ERR_INVALID, "solver_step: first = %d outside [-1, n_steps = %d)", a->first, a->n_steps);
    if (!a->d_eps || !a->d_x || !a->d_x0_prev || !a->d_coef || !a->d_words) return fail(SPDM_ERR_INVALID, "solver_step: null pointer");
    SolverStepArgs k{};
    k.eps = a->d_eps; k.x = a->d_x; k.x0_prev = a->d_x0_prev; k.coef = a->d_coef;
    k.step_dev = a->d_words; k.first_dev = a->d_words + 1; k.flag_dev = a->d_words + 2;
    k.inpaint = a->d_inpaint; k.inp_h = a->inp_h; k.inpaint_per_sample = a->inpaint_per_sample; k.history = a->d_history;
    k.B = a->B; k.H0 = a->H; k.D = a->D;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)a->d_words, a->step, 1, s));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(a->d_words + 1), a->first, 1, s));
    HIP_TRY(launch_solver_step(k, s));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// The per-sample terms of a validation pass's loss in one launch (include/spdm.h, train_metrics.hip).  Stateless.
extern "C" int spdm_loss_terms(int32_t device, const spdm_loss_terms_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "loss_terms: null argument");
    if (a->B < 1 || a->H < 1 || a->D < 1) return fail(SPDM_ERR_INVALID, "loss_terms: B, H, D = %d, %d, %d must all be >= 1", a->B, a->H, a->D);
    if ((long long)a->H * a->D > 0x7fffffffLL - 64) return fail(SPDM_ERR_INVALID, "loss_terms: H x D does not fit 31 bits");
    if (!a->d_eps || !a->d_noise || !a->d_terms) return fail(SPDM_ERR_INVALID, "loss_terms: null pointer");
    if (a->slot_offset < 0) return fail(SPDM_ERR_INVALID, "loss_terms: slot_offset = %lld is negative", (long long)a->slot_offset);
    if (a->n_slots < a->B || a->slot_offset > a->n_slots - a->B)
        return fail(SPDM_ERR_INVALID, "loss_terms: slots [%lld, %lld + %d) lie outside [0, n_slots = %lld)", (long long)a->slot_offset,
                    (long long)a->slot_offset, a->B, (long long)a->n_slots);
    if ((a->d_t_in != nullptr) != (a->d_slot_t != nullptr)) return fail(SPDM_ERR_INVALID, "loss_terms: d_t_in and d_slot_t go together");
    LossTermsArgs k = {};
    k.B = a->B; k.n = a->H * a->D; k.slot_offset = a->slot_offset;
    k.eps = a->d_eps; k.noise = a->d_noise; k.terms = a->d_terms; k.t_in = a->d_t_in; k.slot_t = a->d_slot_t;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_loss_terms(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// The per-frame reconstruction error of a validation batch in one launch (include/spdm.h, train_metrics.hip).  Stateless.
extern "C" int spdm_recon_terms(int32_t device, const spdm_recon_terms_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "recon_terms: null argument");
    if (a->n < 1) return fail(SPDM_ERR_INVALID, "recon_terms: n = %d must be >= 1", a->n);
    if (!a->d_recon || !a->d_target || !a->d_terms) return fail(SPDM_ERR_INVALID, "recon_terms: null pointer");
    if (((uintptr_t)a->d_recon | (uintptr_t)a->d_target) & 15)
        return fail(SPDM_ERR_INVALID, "recon_terms: d_recon and d_target must be 16-byte aligned");
    if (a->slot_offset < 0) return fail(SPDM_ERR_INVALID, "recon_terms: slot_offset = %lld is negative", (long long)a->slot_offset);
    if (a->n_slots < a->n || a->slot_offset > a->n_slots - a->n)
        return fail(SPDM_ERR_INVALID, "recon_terms: slots [%lld, %lld + %d) lie outside [0, n_slots = %lld)", (long long)a->slot_offset,
                    (long long)a->slot_offset, a->n, (long long)a->n_slots);
    ReconTermsArgs k = {};
    k.n = a->n; k.slot_offset = a->slot_offset; k.recon = a->d_recon; k.target = a->d_target; k.terms = a->d_terms;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_recon_terms(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// Planar fp32 frames to uint8 tiles of a contact sheet in one launch (include/spdm.h, dataset.hip).  Stateless.
extern "C" int spdm_frames_to_bytes(int32_t device, const spdm_frames_to_bytes_args* a, void* stream) {
    if (!a) return fail(SPDM_ERR_INVALID, "frames_to_u8: null argument");
    if (a->n < 1 || a->cols < 1 || a->n_tiles < 1)
        return fail(SPDM_ERR_INVALID, "frames_to_u8: n, cols, n_tiles = %d, %d, %lld must all be >= 1", a->n, a->cols, (long long)a->n_tiles);
    if ((long long)a->n * 3 > 0x7fffffffLL) return fail(SPDM_ERR_INVALID, "frames_to_u8: n = %d frames do not fit one launch", a->n);
    if (!a->d_frames || !a->d_out) return fail(SPDM_ERR_INVALID, "frames_to_u8: null pointer");
    if (((uintptr_t)a->d_frames | (uintptr_t)a->d_out) & 15)
        return fail(SPDM_ERR_INVALID, "frames_to_u8: d_frames and d_out must be 16-byte aligned");
    if (a->tile_offset < 0) return fail(SPDM_ERR_INVALID, "frames_to_u8: tile_offset = %lld is negative", (long long)a->tile_offset);
    if (a->n_tiles < a->n || a->tile_offset > a->n_tiles - a->n)
        return fail(SPDM_ERR_INVALID, "frames_to_u8: tiles [%lld, %lld + %d) lie outside [0, n_tiles = %lld)", (long long)a->tile_offset,
                    (long long)a->tile_offset, a->n, (long long)a->n_tiles);
    FramesToU8Args k = {};
    k.n = a->n; k.cols = a->cols; k.tile_offset = a->tile_offset; k.frames = a->d_frames; k.out = a->d_out;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_frames_to_u8(k, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

extern "C" int spdm_train_set_time_scale(spdm_handle* h, const float* d_scale, int32_t B) {
    if (!h) return fail(SPDM_ERR_INVALID, "null handle");
    if (!h->train_simple) return fail(SPDM_ERR_STATE, "spdm_train_set_time_scale needs a handle created with SPDM_FLAG_TRAIN_SIMPLE");
    if (d_scale && (B < 1 || B > h->cfg.max_batch)) return fail(SPDM_ERR_INVALID, "batch %d outside [1, max_batch = %d]", B, h->cfg.max_batch);
    h->t_scale = d_scale;
    h->t_scale_B = d_scale ? B : 0;
    return SPDM_OK;
}

extern "C" int spdm_debug_tensor(spdm_handle* h, const char* name, float* d_out, size_t cap, int32_t shape[4]) {
    if (!h || !name || !shape) return fail(SPDM_ERR_INVALID, "null argument");
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(SPDM_ERR_MISSING, "no intermediate named '%s' (handle needs SPDM_FLAG_DEBUG_KEEP and a prior spdm_unet_forward)", name);
    const Tensor& t = it->second;
    const int l = t.level;
    shape[0] = h->tapB; shape[1] = h->Hp >> l; shape[2] = h->Wp >> l; shape[3] = t.C;
    const size_t n = (size_t)shape[0] * shape[1] * shape[2] * shape[3];
    if (d_out) {
        if (cap < n) return fail(SPDM_ERR_INVALID, "buffer too small: need %zu floats", n);
        HIP_TRY(hipMemcpy(d_out, t.p, n * sizeof(float), hipMemcpyDeviceToDevice));
    }
    return SPDM_OK;
}

extern "C" int spdm_profile_enable(spdm_handle* h, int32_t on) {
    if (!h) return fail(SPDM_ERR_INVALID, "null handle");
    // on = 2: prepare only -- create the events a few instrumented steps need, instrument nothing yet (bench.py does this
    // before its timed region and flips to 1 inside it)
    h->prof = on == 1;
    for (auto& e : h->prof_evts) h->prof_pool.push_back(e);
    h->prof_evts.clear();
    h->prof_open = -1;
    h->prof_launches = 0; h->prof_ms = 0.0; h->prof_flops = 0.0;
    if (on == 2) {
        HIP_TRY(hipSetDevice(h->cfg.device));
        while (h->prof_pool.size() < 256) {
            ProfEvt e{};
            if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) break;
            h->prof_pool.push_back(e);
        }
    }
    return SPDM_OK;
}

extern "C" int spdm_profile_read(spdm_handle* h, int64_t* launches, double* total_ms, double* total_flops) {
    if (!h) return fail(SPDM_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    for (auto& e : h->prof_evts) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            h->prof_ms += ms; h->prof_flops += e.flops; h->prof_launches += e.launches;
        }
        h->prof_pool.push_back(e);
    }
    h->prof_evts.clear();
    if (launches) *launches = h->prof_launches;
    if (total_ms) *total_ms = h->prof_ms;
    if (total_flops) *total_flops = h->prof_flops;
    return SPDM_OK;
}

// -------------------------------------------------------------------------------------------------
// What the entry points off the product path share (spdm_bench_gemm below, the op-level test hooks at the end of the file).
// OpDev: the device allocations of one call, freed on every return.
struct OpDev {
    std::vector<void*> owned;
    OpDev() = default;
    OpDev(const OpDev&) = delete;
    OpDev& operator=(const OpDev&) = delete;
    ~OpDev() { for (void* p : owned) (void)hipFree(p); }
    template <class T>
    int alloc(T** p, size_t bytes) {
        HIP_TRY(hipMalloc((void**)p, bytes));
        owned.push_back(*p);
        return SPDM_OK;
    }
    template <class T>
    int upload(const void* host, size_t bytes, const T** dev) {      // (nothing to upload: *dev stays null)
        T* p = nullptr;
        if (!bytes) return SPDM_OK;
        SPDM_TRY(alloc(&p, bytes));
        HIP_TRY(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
        *dev = p;
        return SPDM_OK;
    }
    int upload_ints(const int32_t* host, int64_t n, const int** dev) { return upload(host, sizeof(int) * (size_t)n, dev); }
    int nan_scratch(uint64_t floats, float** dev) {                   // an unwritten partial reads as NaN
        if (!floats) return SPDM_OK;
        SPDM_TRY(alloc(dev, sizeof(float) * (size_t)floats));
        HIP_TRY(hipMemset(*dev, 0xff, sizeof(float) * (size_t)floats));
        return SPDM_OK;
    }
};

// OwnWeights: weights as the loader lays them out, from a torch-layout tensor of the caller's: the blob of a table of its own.
// walk() records through R as the Loader's walkers do and returns R.err; a split copy it comes back without is outside().
struct OwnWeights {
    DevBlob db;
    WeightTable wt;
    Recorder R;
    explicit OwnWeights(size_t blob_floats, const spdm_tensor_index* index = nullptr, int n_index = 0) : R(wt, blob_floats, index, n_index) {}
    template <class Walk>
    int lay_out(const float* host_blob, Walk walk) {
        SPDM_TRY(db.upload(host_blob, R.n));
        return R.both_passes(db.p, walk);
    }
    static int outside(const char* who, const char* what, const char* instead) {
        return fail(SPDM_ERR_INVALID, "%s: %s outside the split format's range (%s)", who, what, instead);
    }
};

// Micro-benchmark of one implicit-GEMM launch shape on synthetic data (tools/bench_gemm.py); not on
// the product path.  Returns the average device time per launch in *ms_out (HIP events).
extern "C" int spdm_bench_gemm(int32_t device, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t taps,
                               int32_t pro, int32_t epi, int32_t split, int32_t iters, int32_t debug, double* ms_out) {
    if (!ms_out || iters < 1) return fail(SPDM_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(device));
    const int HW = H * W, M = B * HW;
    const unsigned sw = switches_from_env();
    const bool may_splitk = split && epi == EPI_STATS && !(sw & SW_NO_SPLITK);
    const GemmGeom g = gemm_geometry(M, Cout, Cin, HW, W, taps, split, sw, may_splitk);
    float *src = nullptr, *wgt = nullptr, *wgt32 = nullptr, *dst = nullptr, *dst2 = nullptr, *gb = nullptr, *resid = nullptr, *wfrag = nullptr;
    const size_t nsrc = (size_t)M * Cin, nw = (size_t)taps * Cout * Cin, ndst = (size_t)M * Cout;
    OwnWeights ow(nw);                     // wgt32, wgt and wfrag: freed with it
    OpDev dev;                             // every other buffer: freed with it
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    double *st_in = nullptr, *st_out = nullptr, *st_out2 = nullptr;
    SPDM_TRY(dev.alloc(&src, nsrc * 4));
    SPDM_TRY(dev.alloc(&dst2, ndst * 4));
    SPDM_TRY(dev.alloc(&dst, ndst * 4));
    SPDM_TRY(dev.alloc(&resid, ndst * 4));
    SPDM_TRY(dev.alloc(&gb, (size_t)(Cin + Cout) * 2 * 4));
    const bool row_ln = (taps == 1 && pro != 0);           // Linear with a LayerNorm prologue: statistics per ROW
    SPDM_TRY(dev.alloc(&st_in, (size_t)(row_ln ? M : B) * 2 * 8));
    SPDM_TRY(dev.alloc(&st_out, (size_t)B * g.slots * 2 * 8));
    HIP_TRY(hipMemset(st_out, 0, (size_t)B * g.slots * 2 * 8));
    const GemmGeom g2 = gemm_geometry(M, Cout, Cin, HW, W, taps, 0, sw);
    SPDM_TRY(dev.alloc(&st_out2, (size_t)B * g2.slots * 2 * 8));
    HIP_TRY(hipMemset(st_out2, 0, (size_t)B * g2.slots * 2 * 8));
    {   // deterministic pseudo-random fill (values ~U(-1,1)); the weights are laid out as at load time
        std::vector<float> hsrc(nsrc), hw(nw), hgb((size_t)(Cin + Cout) * 2), hres(ndst);
        unsigned x = 12345u;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return ((x >> 8) * (1.0f / 8388608.0f)) - 1.0f; };
        for (auto& v : hsrc) v = rnd();
        for (auto& v : hw) v = rnd() * 0.05f;
        for (auto& v : hgb) v = 1.0f + 0.1f * rnd();
        for (auto& v : hres) v = rnd();           // a non-zero residual: EPI_BIAS_RESID adds something
        // generated in [taps][Cout][Cin] order: a dense source for the copies Loader::conv makes
        Recorder& R = ow.R;
        auto walk = [&]() {
            const WeightCopy v = Recorder::dense(0, taps, Cout, Cin);
            wgt32 = R.f32(v);
            wgt = split ? R.split(v, Cin, "weight") : wgt32;
            wfrag = (split && wgt && (taps == 9 || taps == 3) && Cout % 64 == 0) ? R.frag(v, taps, Cout, Cin) : nullptr;
            return R.err;
        };
        SPDM_TRY(ow.lay_out(hw.data(), walk));
        if (!wgt) return OwnWeights::outside("bench_gemm", "weights", "run such a layer with split = 0");
        std::vector<double> hst((size_t)(row_ln ? M : B) * 2);
        for (size_t b = 0; b < hst.size() / 2; ++b) { hst[2 * b] = 0.0; hst[2 * b + 1] = (double)Cin * (row_ln ? 1 : HW) / 3.0; }
        HIP_TRY(hipMemcpy(src, hsrc.data(), nsrc * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(gb, hgb.data(), hgb.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(st_in, hst.data(), hst.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(resid, hres.data(), ndst * 4, hipMemcpyHostToDevice));
    }
    float* d_part = nullptr;
    if (may_splitk) SPDM_TRY(dev.alloc(&d_part, SPLITK_WORKSPACE_BYTES));
    // (row_ln: like Ctx::linear, every row is its own LayerNorm "sample")
    const StatsRef st_ref{st_in, 1, row_ln ? (1 << 30) : HW, 1, row_ln ? 1 : HW, 1.0 / ((double)Cin * (row_ln ? 1 : HW))};
    GemmArgs a = gemm_args(M, 0, row_ln ? 1 : H, row_ln ? 1 : W, Cin, Cout, taps, split, sw, d_part, pro,
                           AffineSrc{src, Cin, st_ref, gb, gb + Cin}, 0, AffineSrc{}, wgt, wfrag, dst, Cout, epi, st_out,
                           gb + 2 * Cin, resid, Cout);
    a.debug = debug;
    unsigned long long* d_stamps = nullptr;
    if (debug & DBG_STAMP) {
        SPDM_TRY(dev.alloc(&d_stamps, (size_t)65536 * 8 * 8));             // conv_wide: 8 stamps per workgroup
        HIP_TRY(hipMemset(d_stamps, 0, (size_t)65536 * 8 * 8));
        a.stamps = d_stamps;
    }
    hipEvent_t &e0 = ev.a, &e1 = ev.b;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    hipError_t e = launch_gemm(a, nullptr);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch_gemm(a, nullptr);
    if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_gemm(a, nullptr);
    if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    double maxdiff = -1.0, statdiff = -1.0;
    if (e == hipSuccess && debug == 0) {      // self-check: same data through the exact fp32-MFMA configuration
        GemmArgs b2 = a;
        b2.split = 0; b2.wgt = wgt32; b2.wgt_frag = nullptr; b2.dst = dst2; b2.epi_stats = st_out2;
        e = launch_gemm(b2, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        std::vector<float> h1(ndst), h2(ndst);
        if (e == hipSuccess) e = hipMemcpy(h1.data(), dst, ndst * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(h2.data(), dst2, ndst * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
            maxdiff = 0.0;
            for (size_t i = 0; i < ndst; ++i) maxdiff = std::max(maxdiff, (double)std::fabs(h1[i] - h2[i]));
        }
        if (e == hipSuccess && epi == EPI_STATS) {
            // GroupNorm partials of the launch under test against totals recomputed (fp64, host) from ITS OWN output:
            // checks the epilogue's slot bookkeeping and reductions independently of kernel-vs-kernel rounding
            std::vector<double> s1((size_t)B * g.slots * 2);
            e = hipMemcpy(s1.data(), st_out, s1.size() * 8, hipMemcpyDeviceToHost);
            if (e == hipSuccess) {
                statdiff = 0.0;
                const double n = (double)HW * Cout;
                for (int b = 0; b < B; ++b) {
                    double t1 = 0.0, t2 = 0.0, r1 = 0.0, r2 = 0.0;
                    for (int k = 0; k < g.slots; ++k) { t1 += s1[((size_t)b * g.slots + k) * 2]; t2 += s1[((size_t)b * g.slots + k) * 2 + 1]; }
                    const float* p = h1.data() + (size_t)b * HW * Cout;
                    for (size_t i = 0; i < (size_t)HW * Cout; ++i) { r1 += p[i]; r2 += (double)p[i] * p[i]; }
                    const double m1 = t1 / n, mr = r1 / n, v1 = t2 / n - m1 * m1, vr = r2 / n - mr * mr;
                    statdiff = std::max(statdiff, std::fabs(m1 - mr) / std::sqrt(std::max(vr, 1e-30)));
                    statdiff = std::max(statdiff, std::fabs(v1 - vr) / std::max(vr, 1e-30));
                }
            }
        }
    }
    ms_out[1] = maxdiff;
    ms_out[2] = statdiff;
    if (d_stamps && getenv("SPDM_STAMP_DUMP")) {      // raw per-workgroup timeline of conv_wide (analysed offline)
        std::vector<unsigned long long> hs((size_t)65536 * 8);
        if (hipMemcpy(hs.data(), d_stamps, hs.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE* f = fopen(getenv("SPDM_STAMP_DUMP"), "wb")) { fwrite(hs.data(), 8, hs.size(), f); fclose(f); }
        }
    } else if (d_stamps) {      // print the stamp deltas of the traced workgroup (cycles between consecutive stamps)
        unsigned long long hs[256];
        if (hipMemcpy(hs, d_stamps, sizeof(hs), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int g = 0; g < 2; ++g) {
                const int n = (int)hs[g * 128 + 127];
                printf("stamps half %d (%d):", g, n);
                for (int i = 1; i < n && i < 126; ++i) printf(" %llu", hs[g * 128 + i] - hs[g * 128 + i - 1]);
                printf("  total %llu\n", n > 1 ? hs[g * 128 + n - 1] - hs[g * 128] : 0ull);
            }
            fflush(stdout);
        }
    }
    if (e != hipSuccess) return fail(SPDM_ERR_HIP, "bench_gemm: %s", hipGetErrorString(e));
    *ms_out = ms / iters;
    return SPDM_OK;
}

// Micro-benchmark of one fused conv_chain.hip launch on synthetic data (tools/bench_chain.py); not on the product path.
// debug: DBG_NO_MFMA, honoured by SPDM_DIAG builds only.  *ms_out: average device time per launch (HIP events).
extern "C" int spdm_bench_chain(int32_t device, int32_t B, int32_t HW, int32_t n_layers, const int32_t* chan, int32_t iters,
                                int32_t debug, double* ms_out) {
    if (!ms_out || !chan || iters < 1 || B < 1 || HW < 1 || n_layers < 1 || n_layers > CHAIN_MAX_LAYERS) return fail(SPDM_ERR_INVALID, "bad argument");
    if ((long long)B * HW > INT32_MAX || !conv_chain_geometry(B * HW, HW, 1, 3, 1, n_layers, chan))
        return fail(SPDM_ERR_INVALID, "bench_chain: the kernel does not take this chain");
    HIP_TRY(hipSetDevice(device));
    const int M = B * HW, n = n_layers;
    size_t off[CHAIN_MAX_LAYERS], blob = 0, ngb = 0;
    for (int i = 0; i < n; ++i) { off[i] = blob; blob += (size_t)3 * chan[i + 1] * chan[i]; ngb += 2 * (size_t)chan[i]; }
    OwnWeights ow(blob);
    OpDev dev;
    struct Events {
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    float *src = nullptr, *dst = nullptr, *gb = nullptr;
    double* st = nullptr;
    const int slots = stats_slots(HW, CHAIN_M_TILE, 1);
    SPDM_TRY(dev.alloc(&src, (size_t)M * chan[0] * 4));
    SPDM_TRY(dev.alloc(&dst, (size_t)M * chan[n] * 4));
    SPDM_TRY(dev.alloc(&gb, ngb * 4));
    SPDM_TRY(dev.alloc(&st, (size_t)B * slots * 2 * 8));
    float* wf[CHAIN_MAX_LAYERS] = {};
    {   // deterministic pseudo-random fill, as spdm_bench_gemm: inputs ~U(-1, 1), weights at 1 / sqrt(fan-in), gains near 1
        std::vector<float> hsrc((size_t)M * chan[0]), hw(blob), hgb(ngb);
        unsigned x = 12345u;
        auto rnd = [&]() { x = x * 1664525u + 1013904223u; return ((x >> 8) * (1.0f / 8388608.0f)) - 1.0f; };
        for (auto& v : hsrc) v = rnd();
        for (int i = 0; i < n; ++i) {
            const float sc = 1.0f / std::sqrt(9.0f * chan[i]);
            for (size_t k = off[i]; k < off[i] + (size_t)3 * chan[i + 1] * chan[i]; ++k) hw[k] = rnd() * sc;
        }
        for (size_t k = 0; k < ngb; ++k) hgb[k] = (k & 1) ? 0.1f * rnd() : 1.0f + 0.1f * rnd();
        Recorder& R = ow.R;
        auto walk = [&]() {
            for (int i = 0; i < n; ++i) {
                const WeightCopy v = Recorder::dense((long long)off[i], 3, chan[i + 1], chan[i]);
                char name[32];
                snprintf(name, sizeof(name), "weight%d", i);
                wf[i] = R.split(v, chan[i], name) ? R.frag(v, 3, chan[i + 1], chan[i]) : nullptr;
            }
            return R.err;
        };
        SPDM_TRY(ow.lay_out(hw.data(), walk));
        HIP_TRY(hipMemcpy(src, hsrc.data(), hsrc.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(gb, hgb.data(), ngb * 4, hipMemcpyHostToDevice));
    }
    ChainArgs a{};
    a.src = src; a.src_ld = chan[0]; a.dst = dst; a.dst_ld = chan[n]; a.stats = st; a.slots = slots; a.M = M; a.HW = HW; a.n_layers = n;
    a.debug = debug;
    const float* g = gb;
    for (int i = 0; i < n; ++i, g += 2 * chan[i - 1]) {
        if (!wf[i]) return OwnWeights::outside("bench_chain", "weights", "unreachable for these weights");
        a.layer[i] = ChainLayer{wf[i], i ? g : nullptr, i ? g + chan[i] : nullptr, chan[i], chan[i + 1], i & 1};      // the plan's GELU pattern
    }
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));
    hipError_t e = launch_conv_chain(a, nullptr);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch_conv_chain(a, nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev.a, nullptr);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_conv_chain(a, nullptr);
    if (e == hipSuccess) e = hipEventRecord(ev.b, nullptr);
    if (e == hipSuccess) e = hipEventSynchronize(ev.b);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev.a, ev.b);
    if (e != hipSuccess) return fail(SPDM_ERR_HIP, "bench_chain: %s; device: %s", hipGetErrorString(e), hipGetErrorString(hipDeviceSynchronize()));
    *ms_out = ms / iters;
    return SPDM_OK;
}

// -------------------------------------------------------------------------------------------------
// The frame autoencoder (models/encoder/autoencoder.py): 96 x 96 frames <-> 128 latents through a [64][12][12] map.  FrameNet is
// what its two handles share: the state, the allocations, create / update / destroy, the chunk walk, the pending-pass protocol
// and the frame of the lazily built training state.  spdm_encoder and spdm_decoder below add their tensors, buffers and launches.
static constexpr int FRAME_FEAT = 64 * 12 * 12, FRAME_LATENT = 128, FRAME_PIX = 3 * 96 * 96;
static constexpr int FRAME_CHUNK = 2048;           // frames per walk over the layers: what every per-chunk buffer is sized for
static constexpr size_t FRAME_WG_FLOATS = (size_t)8 * FRAME_LATENT * FRAME_FEAT;     // launch_wgrad's partial slabs (the Linear: <= 7)
struct FrameItem { const char* name; std::vector<int> shape; };      // one of a handle's eight tensors: nn.Sequential key, torch shape
struct FrameBuf { float** p; size_t per_frame; };                     // one of a group of per-frame buffers that grow together

static int frame_chunk(int n) { return std::min<int>(n, FRAME_CHUNK); }
// body(i0, m) for each chunk of n frames, in order
template <class Body>
static int frame_chunks(int n, Body body) {
    const int chunk = frame_chunk(n);
    for (int i0 = 0; i0 < n; i0 += chunk) SPDM_TRY(body(i0, std::min(chunk, n - i0)));
    return SPDM_OK;
}
// y [m][out] = x [m][in] W^T + b on the exact fp32 MFMA path: the encoder's Linear(9216, 128), the decoder's Linear(128, 9216)
static hipError_t frame_linear(const float* x, int m, float* w, float* b, int in, int out, float* y, hipStream_t s) {
    return launch_gemm(linear_args(AffineSrc{x, in}, m, 0, LinW{w, nullptr, b, in, out}, /*split=*/false, /*sw=*/0, EPI_BIAS, y), s);
}
// dx [M][N] = dy [M][K] W: a plain data gradient, the forward GEMM on wT ([N][K], k contiguous) with no prologue or epilogue
static hipError_t frame_dgrad(const float* dy, long long M, int K, int N, const float* wT, float* dx, hipStream_t s) {
    return launch_gemm(gemm_args((int)M, 0, 1, 1, K, N, 1, 0, 0, nullptr, PRO_NONE, AffineSrc{dy, K}, 0, AffineSrc{}, wT, nullptr, dx,
                                 N, EPI_PLAIN, nullptr), s);
}

struct FrameNet {
    const char* const what;           // "encoder" / "decoder": the messages and the spdm_<what>_* names are spelt with it
    const char* const pass;           // the training forward whose saved maps ONE backward consumes: "train_forward" / "train_loss"
    int device = 0;
    WeightTable wt;                   // the eight tensors' kernel-layout copies and, once the handle trains, the data gradients'
    long long off[8] = {};            // blob offsets of the eight tensors (the index given to create)
    size_t numel[8] = {};             // ... and their sizes
    size_t blob_floats = 0;
    std::vector<void*> owned;
    int sv_n = 0;                     // frames of the training forward awaiting its backward
    float* g_tmp = nullptr;           // [blob_floats] a later chunk's gradient (training only)
    bool trains = false;              // the training state below is complete
    std::string broken;               // why it is not and never will be: every entry but destroy refuses such a handle
    FrameNet(const char* w, const char* p) : what(w), pass(p) {}
    virtual ~FrameNet() = default;

    int alloc(float** p, size_t floats) {
        void* q = nullptr;
        if (hipMalloc(&q, floats * sizeof(float)) != hipSuccess) return fail(SPDM_ERR_NOMEM, "%s workspace (%zu floats)", what, floats);
        owned.push_back(q);
        *p = (float*)q;
        return SPDM_OK;
    }
    void release(float** p) {
        if (!*p) return;
        for (auto it = owned.begin(); it != owned.end(); ++it)
            if (*it == (void*)*p) { owned.erase(it); break; }
        (void)hipFree(*p);
        *p = nullptr;
    }
    // room for `frames` frames in a group of buffers that holds `*cap`; the steady state returns at once
    int grow(int* cap, int frames, std::initializer_list<FrameBuf> bufs) {
        if (*cap >= frames) return SPDM_OK;
        HIP_TRY(hipDeviceSynchronize());      // (an earlier call's kernels may still read the buffers being replaced)
        for (const FrameBuf& b : bufs) release(b.p);
        *cap = 0;
        for (const FrameBuf& b : bufs) SPDM_TRY(alloc(b.p, (size_t)frames * b.per_frame));
        *cap = frames;
        return SPDM_OK;
    }
    // every entry but destroy, after its argument checks: a usable handle, its device current
    int enter() {
        if (!broken.empty())
            return fail(SPDM_ERR_STATE, "%s: the handle is unusable, its training state was not completed: %s", what, broken.c_str());
        HIP_TRY(hipSetDevice(device));
        return SPDM_OK;
    }
    // a backward pass of n frames consumes the pending training forward of the same n; a wrong n leaves it pending
    int pending(int n) const {
        if (sv_n == 0) return fail(SPDM_ERR_STATE, "%s_backward: no spdm_%s_%s is pending", what, what, pass);
        if (sv_n != n) return fail(SPDM_ERR_STATE, "%s_backward: %d frames, the pending %s had %d", what, n, pass, sv_n);
        return SPDM_OK;
    }
    // The training state, built by the first training forward.  record(R) allocates the handle's scratch and records the data
    // gradients' copies; the handle keeps no blob, so to_blob(T) writes the current weights back to their blob offsets in T
    // (g_tmp: scratch until a backward pass), and laying that out again fills the new copies.  All or nothing: a step that
    // fails leaves a table with copies its device mirror may not hold, so the handle is marked broken and never records again.
    template <class Record, class ToBlob>
    int train_state(hipStream_t s, Record record, ToBlob to_blob) {
        if (trains) return SPDM_OK;
        const int rc = [&]() -> int {
            Recorder R(wt, blob_floats);
            R.plan = false;
            SPDM_TRY(record(R));
            SPDM_TRY(R.err);
            SPDM_TRY(alloc(&g_tmp, blob_floats));
            SPDM_TRY(wt.upload(false));
            SPDM_TRY(to_blob(g_tmp));
            return wt.relayout(g_tmp, s);
        }();
        if (rc != SPDM_OK) broken = g_err;
        trains = rc == SPDM_OK;
        return rc;
    }
    // A backward pass over the chunks: body(i0, m, G) writes chunk (i0, m)'s gradient to G in blob order -- d_grad for the first
    // chunk, g_tmp for a later one, which is then added tensor by tensor: the sum runs in chunk order.
    template <class Body>
    int grad_chunks(int n, float* d_grad, hipStream_t s, Body body) {
        HIP_TRY(hipMemsetAsync(d_grad, 0, blob_floats * sizeof(float), s));
        return frame_chunks(n, [&](int i0, int m) -> int {
            SPDM_TRY(body(i0, m, i0 == 0 ? d_grad : g_tmp));
            if (i0 != 0) {
                for (int k = 0; k < 8; ++k) HIP_TRY(launch_add(g_tmp + off[k], numel[k], d_grad + off[k], s));
            }
            return SPDM_OK;
        });
    }
};

static void frame_destroy(FrameNet* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    for (void* p : f->owned) (void)hipFree(p);
    delete f;
}

// record(f, R) records the kernel-layout copies of the eight tensors, whose names and shapes have been checked against the index
template <class Net, class Record>
static int frame_create(const FrameItem (&items)[8], int32_t device, const float* blob, size_t n, const spdm_tensor_index* index,
                        int32_t n_index, Net** out, Record record) {
    if (!blob || !index || n_index <= 0 || !out) return fail(SPDM_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(device));
    Net* f = new Net();
    f->device = device;
    f->blob_floats = n;
    Recorder R(f->wt, n, index, n_index);
    R.plan = false;                        // fp32 copies only: nothing to ask the device first
    int k = 0;
    for (; k < 8; ++k) {
        const long long off = R.at(items[k].name, items[k].shape);
        if (off < 0) break;
        f->off[k] = off;
        f->numel[k] = 1;
        for (int d : items[k].shape) f->numel[k] *= (size_t)d;
    }
    if (k == 8) record(f, R);
    DevBlob db;
    int rc = R.err;
    if (rc == SPDM_OK) rc = db.upload(blob, n);
    if (rc == SPDM_OK) rc = R.finish(db.p);
    if (rc != SPDM_OK) { frame_destroy(f); return rc; }
    *out = f;
    return SPDM_OK;
}

// the new values go into the handle's tensors in place, and into the data gradients' copies of a handle that trains
static int frame_update_weights(FrameNet* f, const float* d_blob, size_t n, void* stream) {
    if (!f || !d_blob) return fail(SPDM_ERR_INVALID, "null argument");
    if (n != f->blob_floats)
        return fail(SPDM_ERR_INVALID, "blob has %zu floats; the one given to spdm_%s_create had %zu", n, f->what, f->blob_floats);
    SPDM_TRY(f->enter());
    hipStream_t s = (hipStream_t)stream;
    f->sv_n = 0;                               // saved maps belong to the old weights
    SPDM_TRY(f->wt.relayout(d_blob, s));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

// -------------------------------------------------------------------------------------------------
// Observation front end: the autoencoder's encoder, models/encoder/autoencoder.py:11-20, applied by
// prepare_obs_cond_vectors (models/diffusion_ddpm.py:317-321) to every observed frame once per sample() call.
struct spdm_encoder : FrameNet {
    spdm_encoder() : FrameNet("encoder", "train_forward") {}
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr, *wl = nullptr, *bl = nullptr;
    float* feat = nullptr;            // [fw_cap][9216] flattened conv-3 maps of the chunk in flight (spdm_encoder_forward)
    int fw_cap = 0;
    // ---- training (spdm_encoder_train_forward / _backward; nothing below is allocated by a handle that never trains) ----
    float *wlT = nullptr, *w3T = nullptr, *w2T = nullptr;     // transposed copies: the data gradients' launch_gemm weights
    float *sv_feat = nullptr, *sv_x3 = nullptr;      // saved conv-3 map [sv_cap][9216] and conv-2 map [sv_cap][144][128] of ALL frames
    int sv_cap = 0;
    float *bw_a = nullptr, *bw_dz2 = nullptr, *bw_x2 = nullptr;   // backward scratch of one chunk (encoder_backward)
    int bw_cap = 0;
    float *wg_part = nullptr, *c1_part = nullptr;    // wgrad slabs, conv 1's partial rows
};
static constexpr int ENC_X3 = 144 * 128, ENC_X2 = 576 * 64;      // floats per frame of the conv-2 / conv-1 map

// nn.Sequential indices of Autoencoder.encoder: 0, 2, 4 = Conv2d; 7 = Linear
static const FrameItem ENC_ITEMS[8] = {{"0.weight", {16, 3, 2, 2}}, {"0.bias", {16}}, {"2.weight", {32, 16, 2, 2}}, {"2.bias", {32}},
                                       {"4.weight", {64, 32, 2, 2}}, {"4.bias", {64}},
                                       {"7.weight", {FRAME_LATENT, FRAME_FEAT}}, {"7.bias", {FRAME_LATENT}}};
static float* spdm_encoder::* const ENC_TENSORS[8] = {&spdm_encoder::w1, &spdm_encoder::b1, &spdm_encoder::w2, &spdm_encoder::b2,
                                                      &spdm_encoder::w3, &spdm_encoder::b3, &spdm_encoder::wl, &spdm_encoder::bl};

extern "C" void spdm_encoder_destroy(spdm_encoder* e) { frame_destroy(e); }

extern "C" int spdm_encoder_create(int32_t device, const float* blob, size_t n, const spdm_tensor_index* index, int32_t n_index,
                                   spdm_encoder** out) {
    return frame_create(ENC_ITEMS, device, blob, n, index, n_index, out, [](spdm_encoder* e, Recorder& R) {
        for (int k = 0; k < 8; ++k) e->*ENC_TENSORS[k] = R.f32(Recorder::dense(e->off[k], 1, 1, (int)e->numel[k]));
    });
}

extern "C" int spdm_encoder_forward(spdm_encoder* e, int32_t n_images, const float* d_images, float* d_latent, void* stream) {
    if (!e || !d_images || !d_latent || n_images <= 0) return fail(SPDM_ERR_INVALID, "bad argument");
    SPDM_TRY(e->enter());
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(e->grow(&e->fw_cap, frame_chunk(n_images), {{&e->feat, FRAME_FEAT}}));
    SPDM_TRY(frame_chunks(n_images, [&](int i0, int m) -> int {
        HIP_TRY(launch_encoder_convs(d_images + (size_t)i0 * FRAME_PIX, e->w1, e->b1, e->w2, e->b2, e->w3, e->b3, e->feat, m, s));
        HIP_TRY(frame_linear(e->feat, m, e->wl, e->bl, FRAME_FEAT, FRAME_LATENT, d_latent + (size_t)i0 * FRAME_LATENT, s));
        return SPDM_OK;
    }));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

// Replaces: self.vision_encoder(img.flatten(end_dim=1)) of prepare_obs_cond_vectors (models/diffusion_ddpm.py:317-321) inside
// training_step (:128-173), where autograd records the encoder.  The same launches as spdm_encoder_forward per chunk (the GEMM
// reads the same values in the same geometry: the same bits), with the maps the backward pass needs kept for all frames.
extern "C" int spdm_encoder_train_forward(spdm_encoder* e, int32_t n_images, const float* d_images, float* d_latent, void* stream) {
    if (!e || !d_images || !d_latent || n_images <= 0) return fail(SPDM_ERR_INVALID, "bad argument");
    SPDM_TRY(e->enter());
    hipStream_t s = (hipStream_t)stream;
    e->sv_n = 0;
    SPDM_TRY(e->train_state(s,
        [&](Recorder& R) -> int {
            SPDM_TRY(e->alloc(&e->wg_part, FRAME_WG_FLOATS));
            SPDM_TRY(e->alloc(&e->c1_part, (size_t)encoder_conv1_wgrad_blocks(FRAME_CHUNK) * 208));
            // the transposed copies the data gradients read: dx = dy W is the forward GEMM on W^T ([N = in][K = out], k contiguous)
            e->w2T = R.transposed(e->off[2], 32, 64);                         // (32, 16*4)  -> [64][32]
            e->w3T = R.transposed(e->off[4], 64, 128);                        // (64, 32*4)  -> [128][64]
            e->wlT = R.transposed(e->off[6], FRAME_LATENT, FRAME_FEAT);       // (128, 9216) -> [9216][128]
            return SPDM_OK;
        },
        [&](float* T) -> int {
            for (int k = 0; k < 8; ++k)
                HIP_TRY(hipMemcpyAsync(T + e->off[k], e->*ENC_TENSORS[k], e->numel[k] * sizeof(float), hipMemcpyDeviceToDevice, s));
            return SPDM_OK;
        }));
    SPDM_TRY(e->grow(&e->sv_cap, n_images, {{&e->sv_feat, FRAME_FEAT}, {&e->sv_x3, ENC_X3}}));
    SPDM_TRY(frame_chunks(n_images, [&](int i0, int m) -> int {
        const float* img = d_images + (size_t)i0 * FRAME_PIX;
        float *feat = e->sv_feat + (size_t)i0 * FRAME_FEAT, *x3 = e->sv_x3 + (size_t)i0 * ENC_X3;
        HIP_TRY(launch_encoder_train_convs(img, e->w1, e->b1, e->w2, e->b2, e->w3, e->b3, feat, x3, m, s));
        HIP_TRY(frame_linear(feat, m, e->wl, e->bl, FRAME_FEAT, FRAME_LATENT, d_latent + (size_t)i0 * FRAME_LATENT, s));
        // the saved maps' ReLU masks from a float64 evaluation (after the GEMM has read feat: the latents are untouched)
        HIP_TRY(launch_encoder_kinks(img, e->w1, e->b1, e->w2, e->b2, e->w3, e->b3, feat, x3, m, s));
        return SPDM_OK;
    }));
    e->sv_n = n_images;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

// Replaces: loss.backward() through self.vision_encoder (models/encoder/autoencoder.py:11-20) -- the part of
// training_step's backward pass (models/diffusion_ddpm.py:128-173 under Lightning's automatic optimisation) that reaches the
// encoder's parameters, which configure_optimizers (:115-116) hands to Adam with the U-Net's.  Exact fp32, no atomics.
extern "C" int spdm_encoder_backward(spdm_encoder* e, int32_t n_images, const float* d_images, const float* d_grad_latent,
                                     float* d_grad, void* stream) {
    if (!e || !d_images || !d_grad_latent || !d_grad || n_images <= 0) return fail(SPDM_ERR_INVALID, "bad argument");
    SPDM_TRY(e->enter());
    SPDM_TRY(e->pending(n_images));
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(e->grow(&e->bw_cap, frame_chunk(n_images), {{&e->bw_a, ENC_X2}, {&e->bw_dz2, ENC_X3}, {&e->bw_x2, ENC_X2}}));
    e->sv_n = 0;                               // the saved maps serve ONE backward
    SPDM_TRY(e->grad_chunks(n_images, d_grad, s, [&](int i0, int m, float* G) -> int {
        const float* img = d_images + (size_t)i0 * FRAME_PIX;
        const float* g = d_grad_latent + (size_t)i0 * FRAME_LATENT;
        const float* feat = e->sv_feat + (size_t)i0 * FRAME_FEAT;
        const float* x3 = e->sv_x3 + (size_t)i0 * ENC_X3;
        // bw_a holds [dfeat | dz3 | dx3] (9216 + 9216 + 18432 floats per frame) and, once dz2 exists and those three are dead,
        // dx2 (36864 per frame) in the same place
        float *dfeat = e->bw_a, *dz3 = dfeat + (size_t)m * FRAME_FEAT, *dx3 = dz3 + (size_t)m * FRAME_FEAT, *dx2 = e->bw_a;
        const long long M3 = (long long)m * 144, M2 = (long long)m * 576;
        // ---- Linear(9216, 128) ----
        HIP_TRY(launch_wgrad(g, FRAME_LATENT, feat, FRAME_FEAT, m, 1, 1, 1, FRAME_LATENT, FRAME_FEAT, 0, e->wg_part, FRAME_WG_FLOATS,
                             G + e->off[6], s));
        HIP_TRY(launch_colsum(g, FRAME_LATENT, m, FRAME_LATENT, G + e->off[7], s));
        HIP_TRY(frame_dgrad(g, m, FRAME_LATENT, FRAME_FEAT, e->wlT, dfeat, s));
        // ---- conv 3: rows = windows, K = 32 * 4 ----
        HIP_TRY(launch_encoder_dz3(dfeat, feat, m, dz3, s));
        HIP_TRY(launch_wgrad(dz3, 64, x3, 128, M3, 1, 1, 1, 64, 128, 0, e->wg_part, FRAME_WG_FLOATS, G + e->off[4], s));
        HIP_TRY(launch_colsum(dz3, 64, M3, 64, G + e->off[5], s));
        HIP_TRY(frame_dgrad(dz3, M3, 64, 128, e->w3T, dx3, s));
        // ---- conv 2: K = 16 * 4, conv 1's map recomputed from the frames ----
        HIP_TRY(launch_encoder_dz2(dx3, x3, m, e->bw_dz2, s));
        HIP_TRY(launch_encoder_x2(img, e->w1, e->b1, m, e->bw_x2, s));
        HIP_TRY(launch_wgrad(e->bw_dz2, 32, e->bw_x2, 64, M2, 1, 1, 1, 32, 64, 0, e->wg_part, FRAME_WG_FLOATS, G + e->off[2], s));
        HIP_TRY(launch_colsum(e->bw_dz2, 32, M2, 32, G + e->off[3], s));
        HIP_TRY(frame_dgrad(e->bw_dz2, M2, 32, 64, e->w2T, dx2, s));
        // ---- conv 1: K = 3 * 4, no data gradient (nothing is differentiated with respect to the frames) ----
        HIP_TRY(launch_encoder_conv1_wgrad(img, dx2, e->bw_x2, m, e->c1_part, G + e->off[0], G + e->off[1], s));
        return SPDM_OK;
    }));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

// Replaces: optimizer.step() on self.vision_encoder's parameters (Adam(self.parameters()), models/diffusion_ddpm.py:115-116)
extern "C" int spdm_encoder_update_weights(spdm_encoder* e, const float* d_blob, size_t n, void* stream) {
    return frame_update_weights(e, d_blob, n, stream);
}

// -------------------------------------------------------------------------------------------------
// The autoencoder's decoder and its reconstruction training: Autoencoder.decoder of
// models/encoder/autoencoder.py:23-32 under MSELoss(recon, batch) (:48,55-58).  Kernels and row layouts: decoder.hip.
struct spdm_decoder : FrameNet {
    spdm_decoder() : FrameNet("decoder", "train_loss") {}
    // kernel-layout copies (WeightTable): the Linear with its rows in channels-last order q*64 + c, the transposed
    // convolutions as [ci][kk][co] -- which is also what their data gradients read -- and the biases
    float *w0 = nullptr, *b0 = nullptr, *w2 = nullptr, *b2 = nullptr, *w4 = nullptr, *b4 = nullptr, *w6 = nullptr, *b6 = nullptr;
    float* h0 = nullptr;              // [fw_cap][9216] the Linear's output of the chunk in flight (spdm_decoder_forward)
    int fw_cap = 0;
    // ---- training (nothing below is allocated by a handle that never trains) ----
    float* w0g = nullptr;             // [128][9216 as q*64 + c]: the weights of d loss / d latent
    float *sv_h0 = nullptr, *sv_a1 = nullptr, *sv_a2 = nullptr, *sv_recon = nullptr;   // saved maps of ALL frames
    double* sv_sq = nullptr;          // per-frame sums of squared errors
    int sv_cap = 0;
    float *bw_dz4 = nullptr, *bw_dz2 = nullptr, *bw_dh0 = nullptr;     // backward scratch of one chunk
    int bw_cap = 0;
    float *wg_part = nullptr, *wg_tmp = nullptr, *cs_part = nullptr, *w6_part = nullptr;
};
static constexpr int DEC_A1 = 576 * 32, DEC_A2 = 2304 * 16;       // floats per frame of the two post-ReLU maps
// launch_wgrad cuts the rows of a thin layer into as many slabs as its budget holds, down to 64 rows each, and one thread per
// weight then adds them; 256 slabs (one per compute unit) keep that sum short
static constexpr size_t DEC_WG_SLABS = 256;

// nn.Sequential indices of Autoencoder.decoder: 0 = Linear; 2, 4, 6 = ConvTranspose2d (in, out, kH, kW)
static const FrameItem DEC_ITEMS[8] = {{"0.weight", {FRAME_FEAT, FRAME_LATENT}}, {"0.bias", {FRAME_FEAT}}, {"2.weight", {64, 32, 2, 2}},
                                       {"2.bias", {32}}, {"4.weight", {32, 16, 2, 2}}, {"4.bias", {16}}, {"6.weight", {16, 3, 2, 2}},
                                       {"6.bias", {3}}};

// (cin, cout, 2, 2) at src as [ci][kk][co]
static WeightCopy convt_copy(long long src, int cin, int cout) {
    WeightCopy c = Recorder::dense(src, cin, 4, cout);
    c.stride[0] = (long long)cout * 4; c.stride[1] = 1; c.stride[2] = 4;
    return c;
}

extern "C" void spdm_decoder_destroy(spdm_decoder* d) { frame_destroy(d); }

extern "C" int spdm_decoder_create(int32_t device, const float* blob, size_t n, const spdm_tensor_index* index, int32_t n_index,
                                   spdm_decoder** out) {
    const int rc = frame_create(DEC_ITEMS, device, blob, n, index, n_index, out, [](spdm_decoder* d, Recorder& R) {
        // Linear (9216, 128): row c*144 + q -> row q*64 + c, the bias likewise
        WeightCopy w0 = Recorder::dense(d->off[0], 144, 64, FRAME_LATENT);
        w0.stride[0] = FRAME_LATENT; w0.stride[1] = (long long)144 * FRAME_LATENT; w0.stride[2] = 1;
        WeightCopy b0 = Recorder::dense(d->off[1], 1, 144, 64);
        b0.stride[1] = 1; b0.stride[2] = 144;
        d->w0 = R.f32(w0);
        d->b0 = R.f32(b0);
        d->w2 = R.f32(convt_copy(d->off[2], 64, 32));
        d->b2 = R.f32(Recorder::dense(d->off[3], 1, 1, 32));
        d->w4 = R.f32(convt_copy(d->off[4], 32, 16));
        d->b4 = R.f32(Recorder::dense(d->off[5], 1, 1, 16));
        d->w6 = R.f32(convt_copy(d->off[6], 16, 3));
        d->b6 = R.f32(Recorder::dense(d->off[7], 1, 1, 3));
    });
    return rc == SPDM_ERR_MISSING ? SPDM_ERR_INVALID : rc;      // (a decoder's eight names are its shape: one answer for both)
}

extern "C" int spdm_decoder_forward(spdm_decoder* d, int32_t n, const float* d_latent, float* d_recon, void* stream) {
    if (!d || !d_latent || !d_recon || n <= 0) return fail(SPDM_ERR_INVALID, "bad argument");
    SPDM_TRY(d->enter());
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(d->grow(&d->fw_cap, frame_chunk(n), {{&d->h0, FRAME_FEAT}}));
    SPDM_TRY(frame_chunks(n, [&](int i0, int m) -> int {
        // h0 [m][9216] = latent W0^T + b0, columns in channels-last order
        HIP_TRY(frame_linear(d_latent + (size_t)i0 * FRAME_LATENT, m, d->w0, d->b0, FRAME_LATENT, FRAME_FEAT, d->h0, s));
        HIP_TRY(launch_decoder_convs(d->h0, d->w2, d->b2, d->w4, d->b4, d->w6, d->b6, d_recon + (size_t)i0 * FRAME_PIX, m, s));
        return SPDM_OK;
    }));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int spdm_decoder_train_loss(spdm_decoder* d, int32_t n, const float* d_latent, const float* d_target, float* d_recon,
                                       float* d_loss, void* stream) {
    if (!d || !d_latent || !d_target || !d_loss || n <= 0) return fail(SPDM_ERR_INVALID, "bad argument");
    SPDM_TRY(d->enter());
    hipStream_t s = (hipStream_t)stream;
    d->sv_n = 0;
    SPDM_TRY(d->train_state(s,
        [&](Recorder& R) -> int {
            SPDM_TRY(d->alloc(&d->wg_part, FRAME_WG_FLOATS));
            SPDM_TRY(d->alloc(&d->wg_tmp, (size_t)FRAME_FEAT * FRAME_LATENT));
            SPDM_TRY(d->alloc(&d->cs_part, (size_t)decoder_colsum_slabs(FRAME_CHUNK) * FRAME_FEAT));      // (the widest: 0.bias)
            SPDM_TRY(d->alloc(&d->w6_part, (size_t)FRAME_CHUNK * 208));
            // d loss / d latent = dh0 W0 is the forward GEMM on [N = 128][K = 9216], k in h0's column order q*64 + c
            WeightCopy g = Recorder::dense(d->off[0], FRAME_LATENT, 144, 64);
            g.stride[0] = 1; g.stride[1] = FRAME_LATENT; g.stride[2] = (long long)144 * FRAME_LATENT;
            d->w0g = R.f32(g);
            return SPDM_OK;
        },
        [&](float* T) -> int {            // through the inverse permutations
            HIP_TRY(launch_decoder_unperm_linear(d->w0, T + d->off[0], s));
            HIP_TRY(launch_decoder_colsum(d->b0, FRAME_FEAT, 1, FRAME_FEAT, 1, d->cs_part, T + d->off[1], s));      // (one row: a permutation)
            HIP_TRY(launch_decoder_unperm_conv(d->w2, 64, 32, T + d->off[2], s));
            HIP_TRY(launch_decoder_unperm_conv(d->w4, 32, 16, T + d->off[4], s));
            HIP_TRY(launch_decoder_unperm_conv(d->w6, 16, 3, T + d->off[6], s));
            const float* const bias[3] = {d->b2, d->b4, d->b6};
            for (int k = 0; k < 3; ++k)
                HIP_TRY(hipMemcpyAsync(T + d->off[3 + 2 * k], bias[k], d->numel[3 + 2 * k] * sizeof(float), hipMemcpyDeviceToDevice, s));
            return SPDM_OK;
        }));
    SPDM_TRY(d->grow(&d->sv_cap, n, {{&d->sv_h0, FRAME_FEAT}, {&d->sv_a1, DEC_A1}, {&d->sv_a2, DEC_A2}, {&d->sv_recon, FRAME_PIX},
                                     {(float**)&d->sv_sq, 2}}));
    SPDM_TRY(frame_chunks(n, [&](int i0, int m) -> int {
        const float* lat = d_latent + (size_t)i0 * FRAME_LATENT;
        float *h0 = d->sv_h0 + (size_t)i0 * FRAME_FEAT, *a1 = d->sv_a1 + (size_t)i0 * DEC_A1, *a2 = d->sv_a2 + (size_t)i0 * DEC_A2;
        HIP_TRY(frame_linear(lat, m, d->w0, d->b0, FRAME_LATENT, FRAME_FEAT, h0, s));
        HIP_TRY(launch_decoder_train_convs(h0, d->w2, d->b2, d->w4, d->b4, d->w6, d->b6, d->sv_recon + (size_t)i0 * FRAME_PIX,
                                           d_target + (size_t)i0 * FRAME_PIX, a1, a2, d->sv_sq + i0, m, s));
        // the saved maps' ReLU masks from a float64 evaluation (the reconstruction and the loss stay the fp32 forward's)
        HIP_TRY(launch_decoder_kinks(lat, d->w0, d->b0, d->w2, d->b2, d->w4, d->b4, a1, a2, m, s));
        return SPDM_OK;
    }));
    HIP_TRY(launch_decoder_loss(d->sv_sq, n, d_loss, s));
    if (d_recon) HIP_TRY(hipMemcpyAsync(d_recon, d->sv_recon, (size_t)n * FRAME_PIX * sizeof(float), hipMemcpyDeviceToDevice, s));
    d->sv_n = n;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int spdm_decoder_backward(spdm_decoder* d, int32_t n, const float* d_latent, const float* d_target, float* d_grad,
                                     float* d_grad_latent, void* stream) {
    if (!d || !d_latent || !d_target || !d_grad || !d_grad_latent || n <= 0) return fail(SPDM_ERR_INVALID, "bad argument");
    SPDM_TRY(d->enter());
    SPDM_TRY(d->pending(n));
    hipStream_t s = (hipStream_t)stream;
    SPDM_TRY(d->grow(&d->bw_cap, frame_chunk(n), {{&d->bw_dz4, DEC_A2}, {&d->bw_dz2, DEC_A1}, {&d->bw_dh0, FRAME_FEAT}}));
    d->sv_n = 0;                               // the saved maps serve ONE backward
    const float scale = (float)(2.0 / ((double)n * FRAME_PIX));        // d mean((recon - target)^2) / d recon = scale (recon - target)
    SPDM_TRY(d->grad_chunks(n, d_grad, s, [&](int i0, int m, float* G) -> int {
        const float* lat = d_latent + (size_t)i0 * FRAME_LATENT;
        const float* h0 = d->sv_h0 + (size_t)i0 * FRAME_FEAT;
        const float* a1 = d->sv_a1 + (size_t)i0 * DEC_A1;
        const float* a2 = d->sv_a2 + (size_t)i0 * DEC_A2;
        const long long M1 = (long long)m * 144, M2 = (long long)m * 576;
        // ---- ConvTranspose2d(16, 3) + Sigmoid + MSE: dz6 from recon and target, 6.weight / 6.bias, dz4 ----
        HIP_TRY(launch_decoder_bwd6(d->sv_recon + (size_t)i0 * FRAME_PIX, d_target + (size_t)i0 * FRAME_PIX, a2, d->w6, scale, m,
                                    d->bw_dz4, d->w6_part, G + d->off[6], G + d->off[7], s));
        // ---- ConvTranspose2d(32, 16): rows r2, dz4 [M2][64], x = a1 [M2][32] ----
        HIP_TRY(launch_wgrad(a1, 32, d->bw_dz4, 64, M2, 1, 1, 1, 32, 64, 0, d->wg_part, DEC_WG_SLABS * 32 * 64, d->wg_tmp, s));
        HIP_TRY(launch_decoder_unperm_conv(d->wg_tmp, 32, 16, G + d->off[4], s));
        HIP_TRY(launch_decoder_colsum(d->bw_dz4, 64, M2, 16, 4, d->cs_part, G + d->off[5], s));
        HIP_TRY(launch_decoder_dgrad4(d->bw_dz4, a1, d->w4, m, d->bw_dz2, s));
        // ---- ConvTranspose2d(64, 32): rows r1, dz2 [M1][128], x = h0 [M1][64] ----
        HIP_TRY(launch_wgrad(h0, 64, d->bw_dz2, 128, M1, 1, 1, 1, 64, 128, 0, d->wg_part, DEC_WG_SLABS * 64 * 128, d->wg_tmp, s));
        HIP_TRY(launch_decoder_unperm_conv(d->wg_tmp, 64, 32, G + d->off[2], s));
        HIP_TRY(launch_decoder_colsum(d->bw_dz2, 128, M1, 32, 4, d->cs_part, G + d->off[3], s));
        HIP_TRY(frame_dgrad(d->bw_dz2, M1, 128, 64, d->w2, d->bw_dh0, s));      // (no activation follows the Linear)
        // ---- Linear(128, 9216): dh0 [m][9216] in channels-last columns ----
        HIP_TRY(launch_wgrad(d->bw_dh0, FRAME_FEAT, lat, FRAME_LATENT, m, 1, 1, 1, FRAME_FEAT, FRAME_LATENT, 0, d->wg_part,
                             FRAME_WG_FLOATS, d->wg_tmp, s));
        HIP_TRY(launch_decoder_unperm_linear(d->wg_tmp, G + d->off[0], s));
        HIP_TRY(launch_decoder_colsum(d->bw_dh0, FRAME_FEAT, m, FRAME_FEAT, 1, d->cs_part, G + d->off[1], s));
        HIP_TRY(frame_dgrad(d->bw_dh0, m, FRAME_FEAT, FRAME_LATENT, d->w0g, d_grad_latent + (size_t)i0 * FRAME_LATENT, s));
        return SPDM_OK;
    }));
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return SPDM_OK;
}

extern "C" int spdm_decoder_update_weights(spdm_decoder* d, const float* d_blob, size_t n, void* stream) {
    return frame_update_weights(d, d_blob, n, stream);
}

// -------------------------------------------------------------------------------------------------
// Gradient clipping + Adam (include/spdm.h, optim.hip).  Stateless: the moments are the caller's arrays.
extern "C" size_t spdm_adam_workspace_doubles(void) { return (size_t)ADAM_GRID + 1; }
extern "C" size_t spdm_adam_norm_index(void) { return (size_t)ADAM_GRID; }

// A beta arrives as a float, and 1 - (double)0.999f is 1.3e-5 away from 1 - 0.999 in relative terms: two hundred fp32 roundings
// on every second moment.  So a beta is read as the shortest decimal that rounds to the given float (0.999f is 0.999), which
// is what its caller wrote; a float with no short decimal comes back as itself to nine digits.
static double beta_as_written(float b) {
    char buf[40];
    for (int prec = 1; prec <= 9; ++prec) {
        snprintf(buf, sizeof(buf), "%.*g", prec, (double)b);
        const double d = strtod(buf, nullptr);
        if ((float)d == b) return d;
    }
    return (double)b;
}

extern "C" int spdm_adam_step(int32_t device, const spdm_optim_segment* h_segments, int32_t n_segments, int64_t step, float lr,
                              float beta1, float beta2, float eps, float max_norm, double* d_workspace, void* stream) {
    if (!h_segments || !d_workspace) return fail(SPDM_ERR_INVALID, "adam_step: null argument");
    if (n_segments < 1 || n_segments > SPDM_OPTIM_MAX_SEGMENTS)
        return fail(SPDM_ERR_INVALID, "adam_step: %d segments (1 .. %d)", n_segments, SPDM_OPTIM_MAX_SEGMENTS);
    if (step < 1) return fail(SPDM_ERR_INVALID, "adam_step: step %lld (the count including this step, >= 1)", (long long)step);
    if (!std::isfinite(lr) || !std::isfinite(eps) || !std::isfinite(beta1) || !std::isfinite(beta2))
        return fail(SPDM_ERR_INVALID, "adam_step: lr, eps and the betas must be finite");
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
        return fail(SPDM_ERR_INVALID, "adam_step: betas (%g, %g) outside [0, 1)", (double)beta1, (double)beta2);
    if (std::isnan(max_norm)) return fail(SPDM_ERR_INVALID, "adam_step: max_norm is NaN");
    if ((uintptr_t)d_workspace % 16) return fail(SPDM_ERR_INVALID, "adam_step: d_workspace is not 16-byte aligned");
    OptimArgs a = {};
    for (int i = 0; i < n_segments; ++i) {
        const spdm_optim_segment& g = h_segments[i];
        if (!g.d_param || !g.d_grad || !g.d_exp_avg || !g.d_exp_avg_sq) return fail(SPDM_ERR_INVALID, "adam_step: segment %d: null pointer", i);
        if (g.numel == 0) return fail(SPDM_ERR_INVALID, "adam_step: segment %d is empty", i);
        if (((uintptr_t)g.d_param | (uintptr_t)g.d_grad | (uintptr_t)g.d_exp_avg | (uintptr_t)g.d_exp_avg_sq) % 16)
            return fail(SPDM_ERR_INVALID, "adam_step: segment %d: a pointer is not 16-byte aligned", i);
        a.seg[i] = {g.d_param, g.d_grad, g.d_exp_avg, g.d_exp_avg_sq, (unsigned long long)g.numel};
    }
    const double b1 = beta_as_written(beta1), b2 = beta_as_written(beta2);
    const double bc1 = 1.0 - std::pow(b1, (double)step), bc2 = 1.0 - std::pow(b2, (double)step);
    a.nseg = n_segments;
    a.clip = max_norm > 0.f;
    a.max_norm = max_norm;
    a.beta1 = (float)b1;  a.beta1_lo = (float)(b1 - (double)a.beta1);  a.one_minus_beta1 = (float)(1.0 - b1);
    a.beta2 = (float)b2;  a.beta2_lo = (float)(b2 - (double)a.beta2);  a.one_minus_beta2 = (float)(1.0 - b2);
    a.eps = eps;
    a.step_size = (float)((double)lr / bc1);
    a.bc2_sqrt = (float)std::sqrt(bc2);
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_adam_step(a, d_workspace, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// EMA of the weights (include/spdm.h, optim.hip).  Stateless, like spdm_adam_step: the shadow is the caller's arrays.
extern "C" int spdm_ema_step(int32_t device, const spdm_ema_segment* h_segments, int32_t n_segments, float one_minus_decay,
                             void* stream) {
    if (!h_segments) return fail(SPDM_ERR_INVALID, "ema_step: null argument");
    if (n_segments < 1 || n_segments > SPDM_OPTIM_MAX_SEGMENTS)
        return fail(SPDM_ERR_INVALID, "ema_step: %d segments (1 .. %d)", n_segments, SPDM_OPTIM_MAX_SEGMENTS);
    if (!(one_minus_decay >= 0.f && one_minus_decay <= 1.f))        // (a NaN fails both comparisons)
        return fail(SPDM_ERR_INVALID, "ema_step: one_minus_decay %g outside [0, 1]", (double)one_minus_decay);
    EmaArgs a = {};
    for (int i = 0; i < n_segments; ++i) {
        const spdm_ema_segment& g = h_segments[i];
        if (!g.d_ema || !g.d_param) return fail(SPDM_ERR_INVALID, "ema_step: segment %d: null pointer", i);
        if (g.numel == 0) return fail(SPDM_ERR_INVALID, "ema_step: segment %d is empty", i);
        const uintptr_t e = (uintptr_t)g.d_ema, p = (uintptr_t)g.d_param;
        if ((e | p) % 16) return fail(SPDM_ERR_INVALID, "ema_step: segment %d: a pointer is not 16-byte aligned", i);
        const uintptr_t gap = e > p ? e - p : p - e;      // the ranges [e, e + 4 numel) and [p, p + 4 numel) must be disjoint
        if (gap / sizeof(float) < g.numel)
            return fail(SPDM_ERR_INVALID, "ema_step: segment %d: d_ema and d_param overlap", i);
        a.seg[i] = {g.d_ema, g.d_param, (unsigned long long)g.numel};
    }
    a.nseg = n_segments;
    a.omd = one_minus_decay;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(launch_ema_step(a, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// Host-only introspection (no GPU): the launch geometry gemm_geometry picks for a statistics-epilogue convolution, plus the
// statistics-slot reservation the plan makes for it (stats_slots_reserved, as Ctx::salloc).  tests/test_geometry.py checks the invariants between the
// two on a grid of shapes (a mismatch is a silent wrong-statistics bug on the GPU).
extern "C" int spdm_debug_geometry(int32_t M, int32_t N, int32_t K, int32_t HW, int32_t W, int32_t taps, uint32_t switches,
                                   int32_t out[10]) {
    if (!out || M <= 0 || N <= 0 || K <= 0 || HW <= 0 || W <= 0 || M % HW != 0) return fail(SPDM_ERR_INVALID, "bad argument");
    const GemmGeom g = gemm_geometry(M, N, K, HW, W, taps, /*split=*/1, switches, /*stats_epi=*/true);
    out[0] = g.m_tile; out[1] = g.n_tile; out[2] = g.n_tiles; out[3] = g.slots; out[4] = g.ksplit; out[5] = g.skinny | (g.reg << 1);
    out[6] = g.st_m_tile; out[7] = g.st_n_tiles;
    out[8] = stats_slots_reserved(HW, N, g.slots);
    out[9] = combine_rows(HW, N);
    return SPDM_OK;
}

// op-level test hook: y = GELU(x) with the device's own erf (the one every conv prologue uses)
extern "C" int spdm_op_gelu(const float* d_x, float* d_y, size_t n, void* stream) {
    if (!d_x || !d_y || n == 0) return fail(SPDM_ERR_INVALID, "bad argument");
    HIP_TRY(launch_gelu(d_x, d_y, n, (hipStream_t)stream));
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return SPDM_OK;
}

// Host-only introspection: how the launch of the most recent spdm_op_gemm call staged its input slab (GemmRoute::whole)
static int g_op_gemm_whole = -1;
extern "C" int spdm_debug_whole_tiles(void) { return g_op_gemm_whole; }
// ... how many launches of this process (plan or spdm_op_gemm; a captured step counts once) read the upsample through conv_wide's loader
extern "C" int spdm_debug_fused_upsample_launches(void) { return gemm_wide_upcat_launches(); }
extern "C" int spdm_debug_pooled_epilogue_launches(void) { return g_pooled_epilogue_launches; }
extern "C" int spdm_debug_conv_chain_launches(void) { return g_conv_chain_launches; }
extern "C" int spdm_debug_plan_routes(const spdm_handle* h, int32_t B, int32_t* out, int32_t cap) {
    static_assert(sizeof(PlanRoutes) == SPDM_PLAN_ROUTES_INTS * sizeof(int32_t), "PlanRoutes is the query's layout");
    spdm_handle* hm = const_cast<spdm_handle*>(h);       // (Ctx holds a mutable handle; choose_routes is const)
    SPDM_TRY(check_ready(hm, B));
    if (!out || cap < SPDM_PLAN_ROUTES_INTS) return fail(SPDM_ERR_INVALID, "out must hold %d values", SPDM_PLAN_ROUTES_INTS);
    const Ctx c{hm, B, nullptr, false};
    const PlanRoutes r = h->simple ? PlanRoutes{} : c.choose_routes();
    memcpy(out, &r, sizeof(r));
    return SPDM_OK;
}

// op-level test hooks, the frame they share.  Each hook is: validate on the host (OpCheck), upload what the launch dereferences
// (OpDev), ONE launch_* on the caller's tensors, op_finish.  A hook's per-op switch fills need[] / optional[] / absent[] and
// states the op's own shape rules; the rules every op shares are the checker's, in one wording each.
namespace {
struct OpCheck {
    static constexpr int MAX_BUFS = 11;                   // the largest hook's (spdm_op_frame)
    static constexpr int64_t ANY_INDEX = (int64_t)INT32_MAX + 1;     // indices(): a limit no int32 reaches
    const char* hook;
    int op;
    const int64_t* d = nullptr;                           // the hook's dim[] (dims)
    bool ok = true;                                       // every extent so far fits 31 bits
    uint64_t need[MAX_BUFS] = {};                         // floats of d_buf[i]
    bool optional[MAX_BUFS] = {}, absent[MAX_BUFS] = {};  // may be null / must be null in this call
    int nbuf = 0;                                         // buffers the op takes: those from nbuf on are absent
    OpCheck(const char* hook_name, int op_id) : hook(hook_name), op(op_id) {}
    __attribute__((format(printf, 2, 3))) int bad(const char* fmt, ...) const {
        char msg[sizeof(g_err)];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        return fail(SPDM_ERR_INVALID, "%s: %s", hook, msg);
    }
    // element counts that must stay within 31 bits; no intermediate can overflow
    uint64_t mul(std::initializer_list<int64_t> f) {
        uint64_t v = 1;
        for (int64_t x : f) {
            v *= (uint64_t)x;              // both factors are below 2^31
            if (v > (uint64_t)INT32_MAX) { ok = false; v = 1; }
        }
        return v;
    }
    uint64_t strided(uint64_t rows, int64_t ld, int64_t width) {      // rows of ld floats, the last one width long
        if (rows == 0) { ok = false; return 0; }
        const uint64_t v = mul({(int64_t)rows - 1, ld}) + (uint64_t)width;
        if (v > (uint64_t)INT32_MAX) ok = false;
        return v;
    }
    int fits() const { return ok ? SPDM_OK : bad("op %d: a tensor extent is beyond 31 bits", op); }
    // the op is one of the hook's n_ops; every dim in [0, 2^31) -- dim[lo_index] from lo on --, and those beyond the
    // taken_of[op] the op reads are 0
    int dims(const int64_t* dim, int total, const int* taken_of, int n_ops, int lo = 0, int lo_index = -1) {
        if (op < 0 || op >= n_ops) return bad("unknown op %d", op);
        const int taken = taken_of[op];
        d = dim;
        for (int i = 0; i < total; ++i) {
            const int from = i == lo_index ? lo : 0;
            if (d[i] < from || d[i] > INT32_MAX) return bad("dim[%d] = %lld outside [%d, 2^31)", i, (long long)d[i], from);
            if (i >= taken && d[i] != 0) return bad("op %d takes %d dims; dim[%d] must be 0", op, taken, i);
        }
        return SPDM_OK;
    }
    bool positive(std::initializer_list<int> which) const {
        for (int i : which) if (d[i] < 1) return false;
        return true;
    }
    // the extents fit; a buffer the call does not take is null, one it takes is there (unless optional) and holds need[i] floats
    int buffers(float* const* d_buf, const uint64_t* cap, int total) const {
        SPDM_TRY(fits());
        for (int i = 0; i < total; ++i) {
            if (i >= nbuf || absent[i]) {
                if (d_buf[i]) return bad("op %d does not take d_buf[%d] here; it must be null", op, i);
            } else if (!d_buf[i]) {
                if (!optional[i]) return bad("op %d: d_buf[%d] is null", op, i);
            } else if (cap[i] < need[i]) {
                return bad("op %d: d_buf[%d] holds %llu floats, the launch needs %llu", op, i, (unsigned long long)cap[i], (unsigned long long)need[i]);
            }
        }
        return SPDM_OK;
    }
    // a host index array (`name`: h_idx[k], h_t): `want` entries (0: not taken here), each in [0, lim); ANY_INDEX: no upper bound
    int indices(const char* name, const int32_t* h_idx, int64_t n_idx, int64_t want, int64_t lim) const {
        if (want == 0) return h_idx || n_idx ? bad("op %d takes no index arrays at %s here; it must be null", op, name) : SPDM_OK;
        if (!h_idx || n_idx != want) return bad("op %d: %s must hold %lld entries", op, name, (long long)want);
        for (int64_t i = 0; i < want; ++i)
            if (h_idx[i] < 0 || h_idx[i] >= lim) return bad("op %d: %s[%lld] = %d outside [0, %lld)", op, name, (long long)i, h_idx[i], (long long)lim);
        return SPDM_OK;
    }
    // a side buffer of doubles (d_stats_out, d_sq): `want` of them (0: not taken here)
    int doubles(const char* name, const double* ptr, uint64_t cap, uint64_t want, bool may_be_null) const {
        if (want == 0) return ptr || cap ? bad("op %d does not take %s here; it must be null", op, name) : SPDM_OK;
        if (!ptr) return may_be_null ? SPDM_OK : bad("op %d: %s is null", op, name);
        if (cap < want) return bad("op %d: %s holds %llu doubles, the launch needs %llu", op, name, (unsigned long long)cap, (unsigned long long)want);
        return SPDM_OK;
    }
};

// launch_wgrad's partial slabs under a budget of floats: chunks of M, floats of all slabs (0: they exceed the budget), rows per chunk
struct WgradSlabs { int nch; uint64_t slab; int wrows; };
WgradSlabs wgrad_slabs(long long M, int taps, int Co, int Ci, size_t budget) {
    const int nch = wgrad_chunks(M, taps, Co, Ci, budget);
    const uint64_t slab = (uint64_t)nch * taps * Co * Ci;
    if (nch < 1 || slab > budget) return {nch, 0, 0};
    return {nch, slab, (int)(((M + nch - 1) / nch + 3) / 4 * 4)};
}

// the hooks' tail: drain the device, then the launch's error with the device's state, or the device's own
int op_finish(const char* hook, int op, hipError_t el) {
    const hipError_t es = hipDeviceSynchronize();
    if (el != hipSuccess) return fail(SPDM_ERR_HIP, "%s: op %d: launch failed: %s; device: %s", hook, op, hipGetErrorString(el), hipGetErrorString(es));
    if (es != hipSuccess) return fail(SPDM_ERR_HIP, "%s: op %d: %s", hook, op, hipGetErrorString(es));
    return SPDM_OK;
}
}  // namespace

// op-level test hook: one launch_gemm exactly as the plan builds it, on the caller's tensors (include/spdm.h)
extern "C" int spdm_op_gemm(spdm_op_gemm_args* p) {
    g_op_gemm_whole = -1;
    if (!p) return fail(SPDM_ERR_INVALID, "op_gemm: null argument");
    spdm_op_gemm_args& q = *p;
    for (int i = 0; i < 10; ++i) q.out[i] = -1;
    const int HW = q.H * q.W;
    if (q.B <= 0 || q.H <= 0 || q.W <= 0 || q.K <= 0 || q.N <= 0) return fail(SPDM_ERR_INVALID, "op_gemm: empty shape");
    if (!(q.taps == 9 || q.taps == 3 || q.taps == 1)) return fail(SPDM_ERR_INVALID, "op_gemm: taps must be 9, 3 or 1");
    if (q.taps == 3 && q.W != 1) return fail(SPDM_ERR_INVALID, "op_gemm: 3-tap convolutions need W == 1");
    if (q.taps == 1 && HW != 1) return fail(SPDM_ERR_INVALID, "op_gemm: a Linear layer has H == W == 1 (B = rows)");
    if (q.taps != 1 && q.W > 8) return fail(SPDM_ERR_INVALID, "op_gemm: maps wider than 8");
    if (q.K % 32 != 0 || q.N % 64 != 0) return fail(SPDM_ERR_INVALID, "op_gemm: K %% 32 == 0 and N %% 64 == 0 required (K %d, N %d)", q.K, q.N);
    if (q.pro < PRO_NONE || q.pro > PRO_UPCAT || q.epi < EPI_STATS || q.epi > EPI_PLAIN) return fail(SPDM_ERR_INVALID, "op_gemm: unknown pro / epi");
    if (!q.d_src || !q.d_dst || !q.h_weight) return fail(SPDM_ERR_INVALID, "op_gemm: src, dst and weight are required");
    if (q.dst_ld < q.N || q.dst_ld % 4 || q.src_ld % 4) return fail(SPDM_ERR_INVALID, "op_gemm: bad leading dimension");
    const bool fused = q.pro == PRO_POOL || q.pro == PRO_UPCAT, two = !fused && q.d_skip != nullptr;
    if (q.src_ld < ((fused && q.pro == PRO_UPCAT) || two ? q.up_C : q.K)) return fail(SPDM_ERR_INVALID, "op_gemm: src_ld too small");
    if ((q.d_skip != nullptr) != (q.pro == PRO_UPCAT || two)) return fail(SPDM_ERR_INVALID, "op_gemm: skip is the second source of pro 4 / a two-source input only");
    if (q.d_skip && (q.up_C <= 0 || q.up_C >= q.K || q.skip_ld % 4 || q.skip_ld < q.K - q.up_C)) return fail(SPDM_ERR_INVALID, "op_gemm: bad up_C / skip_ld");
    if (two && (q.pro != PRO_NONE || q.d_src_stats)) return fail(SPDM_ERR_INVALID, "op_gemm: a two-source input takes its prologue from the skip statistics only");
    if (q.d_skip_stats && !q.d_skip) return fail(SPDM_ERR_INVALID, "op_gemm: skip statistics without skip");
    if ((q.pro == PRO_GN || q.pro == PRO_GN_GELU) && !q.d_src_stats) return fail(SPDM_ERR_INVALID, "op_gemm: GroupNorm prologue without statistics");
    if ((q.d_src_stats && (!q.d_gamma || !q.d_beta || q.src_slots <= 0 || q.src_m_tile <= 0 || q.src_n_tiles <= 0)) ||
        (q.d_skip_stats && (!q.d_skip_gamma || !q.d_skip_beta || q.skip_slots <= 0 || q.skip_m_tile <= 0 || q.skip_n_tiles <= 0)))
        return fail(SPDM_ERR_INVALID, "op_gemm: pending GroupNorm needs gamma, beta and the partials' geometry");
    if (q.d_src_stats && q.pro == PRO_NONE) return fail(SPDM_ERR_INVALID, "op_gemm: src statistics given with pro 0");
    if (q.epi != EPI_STATS && q.epi != EPI_PLAIN && !q.d_bias) return fail(SPDM_ERR_INVALID, "op_gemm: bias epilogue without bias");
    if (q.epi == EPI_BIAS_RESID && (!q.d_resid || q.resid_ld < q.N || q.resid_ld % 4)) return fail(SPDM_ERR_INVALID, "op_gemm: bad residual");
    if (q.d_row_stats && q.taps != 1) return fail(SPDM_ERR_INVALID, "op_gemm: row statistics are a Linear layer's output");
    const int M = q.B * HW;
    const int src_rows = q.pro == PRO_POOL ? 4 * HW : q.pro == PRO_UPCAT ? HW / 4 : HW;      // rows per sample of src
    if (q.pro == PRO_UPCAT && ((q.H & 1) || (q.W & 1))) return fail(SPDM_ERR_INVALID, "op_gemm: upsample read-through needs an even map");
    const int split = q.split ? 1 : 0;
    OwnWeights ow((size_t)q.N * q.K * (q.taps == 1 ? 1 : 9));
    Recorder& R = ow.R;
    float *dw = nullptr, *dwf = nullptr;
    auto walk = [&]() {                    // Loader::linear / Loader::conv (Cout % 64 == 0 here: a fragment-order copy)
        const WeightCopy v = q.taps == 1 ? Recorder::dense(0, 1, q.N, q.K) : Recorder::conv_taps(0, q.N, q.K, q.taps);
        dw = split ? R.split(v, q.K, "weight") : R.f32(v);
        dwf = (split && dw && q.taps != 1) ? R.frag(v, q.taps, q.N, q.K) : nullptr;
        return R.err;
    };
    SPDM_TRY(ow.lay_out(q.h_weight, walk));
    if (!dw) return OwnWeights::outside("op_gemm", "weights", "the loader keeps such a layer on the exact path");
    const unsigned sw = switches_from_env();
    // as the plan: a split-precision convolution may split K unless switched off (the handle then holds no partial buffer)
    const bool may_partial = split && q.taps != 1 && q.epi == EPI_STATS && !(sw & SW_NO_SPLITK);
    const GemmGeom g = gemm_geometry(M, q.N, q.K, HW, q.W, q.taps, split, sw, may_partial);
    if (q.epi == EPI_STATS && (!q.d_stats || q.stats_cap < (size_t)q.B * g.slots * 2))
        return fail(SPDM_ERR_INVALID, "op_gemm: statistics buffer needs %zu doubles", (size_t)q.B * g.slots * 2);
    if (q.d_row_stats && q.row_stats_cap < (size_t)M * g.n_tiles * 2)
        return fail(SPDM_ERR_INVALID, "op_gemm: row statistics buffer needs %zu doubles", (size_t)M * g.n_tiles * 2);
    if (g.ksplit > 1 && (size_t)g.ksplit * M * q.N * sizeof(float) > SPLITK_WORKSPACE_BYTES)
        return fail(SPDM_ERR_INVALID, "op_gemm: split-K slabs exceed the workspace");
    float* dp = nullptr;                   // (freed with the table)
    if (may_partial) SPDM_TRY(ow.wt.alloc((void**)&dp, g.ksplit > 1 ? (size_t)g.ksplit * M * q.N * sizeof(float) : 0));
    // the caller's tensors as the plan's sources, pending GroupNorms from the raw partials; then the plan's own builder
    auto ref = [](const double* st, int slots, int m_tile, int n_tiles, int rows, int cnorm) {
        return StatsRef{st, slots, m_tile, n_tiles, rows, 1.0 / ((double)cnorm * rows)};
    };
    const int src_c = (q.pro == PRO_UPCAT || two) ? q.up_C : q.K;
    AffineSrc src{q.d_src, q.src_ld}, skip{q.d_skip, q.skip_ld};
    if (q.d_src_stats)
        src = AffineSrc{q.d_src, q.src_ld, ref(q.d_src_stats, q.src_slots, q.src_m_tile, q.src_n_tiles, src_rows,
                                               q.src_cnorm > 0 ? q.src_cnorm : src_c), q.d_gamma, q.d_beta};
    if (q.d_skip_stats)
        skip = AffineSrc{q.d_skip, q.skip_ld, ref(q.d_skip_stats, q.skip_slots, q.skip_m_tile, q.skip_n_tiles, HW,
                                                  q.skip_cnorm > 0 ? q.skip_cnorm : q.K - q.up_C), q.d_skip_gamma, q.d_skip_beta};
    const int pro = (two && q.d_skip_stats) ? PRO_GN : q.pro;         // (Ctx::two_args)
    GemmArgs a = gemm_args(M, M, q.H, q.W, q.K, q.N, q.taps, split, sw, dp, pro, src, q.up_C, skip, dw,
                           dwf, q.d_dst, q.dst_ld, q.epi, q.epi == EPI_STATS ? q.d_stats : nullptr, q.d_bias,
                           q.d_resid, q.resid_ld, q.d_row_stats);
    if (fused && !gemm_takes_fused_source(a))
        return fail(SPDM_ERR_INVALID, "op_gemm: this launch does not take a fused source (the plan materialises it)");
    if (two && !gemm_takes_two_sources(a))
        return fail(SPDM_ERR_INVALID, "op_gemm: this launch does not take a two-source input (the plan concatenates)");
    GemmRoute r{-1, -1, -1, -1, 0};
    a.route = &r;                 // the launch records what it dispatched
    // unwritten partials read as NaN
    if (q.epi == EPI_STATS) HIP_TRY(hipMemset(q.d_stats, 0xff, (size_t)q.B * g.slots * 2 * sizeof(double)));
    if (q.d_row_stats) HIP_TRY(hipMemset(q.d_row_stats, 0xff, (size_t)M * g.n_tiles * 2 * sizeof(double)));
    const hipError_t el = launch_gemm(a, nullptr);
    if (el == hipErrorInvalidValue && r.kernel < 0)
        return fail(SPDM_ERR_INVALID, "op_gemm: launch_gemm failed (%s) before any kernel was dispatched (a host-side shape contract); device: %s",
                    hipGetErrorString(el), hipGetErrorString(hipDeviceSynchronize()));
    // (the split-K main kernel may have been launched before the combine reported an error: the tail drains the device first)
    SPDM_TRY(op_finish("op_gemm", 0, el));                // (its one op)
    g_op_gemm_whole = (r.kernel == ROUTE_WIDE) ? r.whole : 0;
    q.out[0] = r.kernel; q.out[1] = r.variant; q.out[2] = r.m_tile; q.out[3] = r.n_tile; q.out[4] = g.ksplit;
    q.out[5] = two ? 1 : 0; q.out[6] = fused ? 1 : 0; q.out[7] = g.slots; q.out[8] = g.st_m_tile; q.out[9] = g.st_n_tiles;
    return SPDM_OK;
}

// op-level test hook: one launch_conv_chain as the plan builds it, on the caller's tensors (include/spdm.h)
extern "C" int spdm_op_chain(spdm_op_chain_args* p) {
    if (!p) return fail(SPDM_ERR_INVALID, "op_chain: null argument");
    spdm_op_chain_args& q = *p;
    for (int i = 0; i < 4; ++i) q.out[i] = -1;
    static_assert(SPDM_OP_CHAIN_MAX_LAYERS == CHAIN_MAX_LAYERS, "the hook's table is the launch's");
    OpCheck E("op_chain", 0);                             // (its one op)
    if (q.B < 1 || q.HW < 1 || q.n_layers < 1 || q.n_layers > CHAIN_MAX_LAYERS) return E.bad("B, HW positive and 1 <= n_layers <= %d required", CHAIN_MAX_LAYERS);
    const int n = q.n_layers;
    const uint64_t M = E.mul({q.B, q.HW});
    SPDM_TRY(E.fits());
    if (!conv_chain_geometry((int)M, q.HW, 1, 3, 1, n, q.chan))
        return E.bad("the kernel does not take this chain (HW a power of two in [4, 64], widths multiples of 64 up to 512)");
    const int C0 = q.chan[0], CN = q.chan[n];
    if (!q.d_src || !q.d_dst) return E.bad("src and dst are required");
    if (q.src_ld < C0 || q.src_ld % 4 || q.dst_ld < CN || q.dst_ld % 4) return E.bad("bad leading dimension");
    (void)E.strided(M, q.src_ld, C0);
    (void)E.strided(M, q.dst_ld, CN);
    SPDM_TRY(E.fits());
    size_t blob = 0, off[CHAIN_MAX_LAYERS];
    for (int i = 0; i < n; ++i) {
        if (!q.h_weight[i]) return E.bad("h_weight[%d] is null", i);
        if (i > 0 && (!q.d_gamma[i] || !q.d_beta[i])) return E.bad("layer %d: the GroupNorm on its input needs gamma and beta", i);
        off[i] = blob;
        blob += (size_t)3 * q.chan[i + 1] * q.chan[i];
    }
    const int slots = stats_slots(q.HW, CHAIN_M_TILE, 1);
    SPDM_TRY(E.doubles("d_stats", q.d_stats, q.stats_cap, (uint64_t)q.B * slots * 2, false));
    // the layers' weights as one blob, laid out as Loader::conv lays a 3-tap layer out (split copy: the range verdict; its
    // fragment-order copy: what the kernel reads)
    std::vector<float> hblob(blob);
    for (int i = 0; i < n; ++i) memcpy(hblob.data() + off[i], q.h_weight[i], (size_t)3 * q.chan[i + 1] * q.chan[i] * sizeof(float));
    OwnWeights ow(blob);
    Recorder& R = ow.R;
    float* wf[CHAIN_MAX_LAYERS] = {};
    auto walk = [&]() {
        for (int i = 0; i < n; ++i) {
            const WeightCopy v = Recorder::dense((long long)off[i], 3, q.chan[i + 1], q.chan[i]);
            char name[32];
            snprintf(name, sizeof(name), "weight%d", i);
            wf[i] = R.split(v, q.chan[i], name) ? R.frag(v, 3, q.chan[i + 1], q.chan[i]) : nullptr;
        }
        return R.err;
    };
    SPDM_TRY(ow.lay_out(hblob.data(), walk));
    ChainArgs a{};
    a.src = q.d_src; a.src_ld = q.src_ld; a.dst = q.d_dst; a.dst_ld = q.dst_ld; a.stats = q.d_stats; a.slots = slots;
    a.M = (int)M; a.HW = q.HW; a.n_layers = n;
    for (int i = 0; i < n; ++i) {
        if (!wf[i]) return OwnWeights::outside("op_chain", "weights", "the plan keeps such a site on its per-layer launches");
        a.layer[i] = ChainLayer{wf[i], i ? q.d_gamma[i] : nullptr, i ? q.d_beta[i] : nullptr, q.chan[i], q.chan[i + 1], i ? (q.gelu[i] != 0) : 0};
    }
    HIP_TRY(hipMemset(q.d_stats, 0xff, (size_t)q.B * slots * 2 * sizeof(double)));       // unwritten partials read as NaN
    SPDM_TRY(op_finish("op_chain", 0, launch_conv_chain(a, nullptr)));
    q.out[0] = conv_chain_blocks(a.M); q.out[1] = slots; q.out[2] = CHAIN_M_TILE; q.out[3] = 1;
    return SPDM_OK;
}

// op-level test hook: one launch_* of the training pass on the caller's tensors (include/spdm.h).  Validate, upload the integer
// arrays, launch, synchronise.
extern "C" int spdm_op_train(spdm_op_train_args* p) {
    if (!p) return fail(SPDM_ERR_INVALID, "op_train: null argument");
    spdm_op_train_args& q = *p;
    for (int i = 0; i < 4; ++i) q.info[i] = -1;
    OpCheck E("op_train", q.op);
    static const int n_dims[SPDM_OPT_COUNT] = {9, 8, 3, 3, 4, 5, 7, 4, 5, 4, 2, 2, 1, 4, 4, 5, 6, 3};
    const int64_t* d = q.dim;
    SPDM_TRY(E.dims(d, SPDM_OP_TRAIN_DIMS, n_dims, SPDM_OPT_COUNT));
    auto pow2_le512 = [](int64_t C) { return C >= 1 && C <= 512 && (C & (C - 1)) == 0; };
    auto& need = E.need;
    auto& optional = E.optional;
    int& nbuf = E.nbuf;
    int64_t idx_n[SPDM_OP_TRAIN_IDX] = {0, 0}, idx_lim[SPDM_OP_TRAIN_IDX] = {0, 0};    // entries of h_idx[k] (0: not taken), each below idx_lim[k]
    uint64_t M = 0;
    WgradSlabs ws{0, 0, 0};
    switch (q.op) {
        case SPDM_OPT_WGRAD:
        case SPDM_OPT_WGRAD_MAPPED: {
            const bool mapped = q.op == SPDM_OPT_WGRAD_MAPPED;
            if (!E.positive({0, 1, 2, 3, 4, 5})) return E.bad("wgrad: B, H, W, taps, Co, Ci must be positive");
            const int64_t taps = d[3], Co = d[4], Ci = d[5];
            if (!(taps == 9 || taps == 3 || (taps == 1 && !mapped))) return E.bad("wgrad: taps %lld", (long long)taps);
            if (taps == 3 && d[2] != 1) return E.bad("wgrad: 3-tap layers need W == 1");
            if (taps == 1 && (d[1] != 1 || d[2] != 1)) return E.bad("wgrad: a Linear layer has H == W == 1 (B = rows)");
            M = E.mul({d[0], d[1], d[2]});
            int64_t ldy = Co, ldx = Ci;
            uint64_t ndst;
            if (mapped) {
                if (!E.positive({6, 7}) || d[6] > Co || d[7] > Ci) return E.bad("wgrad_mapped: need 1 <= no <= Co and 1 <= ni <= Ci");
                ndst = E.mul({d[6], d[7], 9});
                idx_n[0] = d[6]; idx_lim[0] = Co; idx_n[1] = d[7]; idx_lim[1] = Ci;
            } else {
                if (d[6] != (taps == 1 ? 0 : 1)) return E.bad("wgrad: conv9 is 1 for taps 9 / 3 and 0 for taps 1");
                ldy = d[7]; ldx = d[8];
                if (ldy < Co || ldx < Ci) return E.bad("wgrad: ldy >= Co and ldx >= Ci required");
                ndst = E.mul({Co, Ci, d[6] ? 9 : 1});
            }
            need[0] = E.strided(M, ldy, Co); need[1] = E.strided(M, ldx, Ci); need[2] = ndst; nbuf = 3;
            (void)E.mul({taps, Co, Ci});
            if (!E.ok) break;
            ws = wgrad_slabs((long long)M, (int)taps, (int)Co, (int)Ci, TrainPass::WGRAD_BUDGET);
            if (!ws.slab) return E.bad("wgrad: the partial slabs exceed the budget");
            break;
        }
        case SPDM_OPT_COLSUM:
            if (!E.positive({0, 1, 2}) || d[2] < d[1]) return E.bad("colsum: M, C positive and ld >= C required");
            need[0] = E.strided((uint64_t)d[0], d[2], d[1]); need[1] = (uint64_t)d[1]; nbuf = 2;
            break;
        case SPDM_OPT_GN_STATS:
            if (!E.positive({0, 1}) || d[2] > d[1]) return E.bad("gn_stats: B, n positive and 0 <= cnt <= n required");
            need[0] = E.mul({d[0], d[1]}); need[1] = need[2] = (uint64_t)d[0]; nbuf = 3;
            break;
        case SPDM_OPT_GN_BWD:
        case SPDM_OPT_GN_BWD_MAPPED: {
            if (!E.positive({0, 1, 2}) || d[3] > 1) return E.bad("gn_bwd: B, HW, C positive and gelu 0 / 1 required");
            const int64_t C = d[2];
            if (q.op == SPDM_OPT_GN_BWD) {
                if (!pow2_le512(C)) return E.bad("gn_bwd: C must be a power of two <= 512 (got %lld)", (long long)C);
            } else {
                if (C % 64 != 0 || C > 512) return E.bad("gn_bwd_mapped: C must be a multiple of 64 <= 512 (got %lld)", (long long)C);
                if (d[4] < 1 || d[4] > C) return E.bad("gn_bwd_mapped: need 1 <= nreal <= C");
                idx_n[0] = d[4]; idx_lim[0] = C;
            }
            const uint64_t n = E.mul({d[0], d[1], C});
            need[0] = n; need[1] = need[2] = (uint64_t)d[0]; need[3] = need[4] = (uint64_t)C; need[5] = need[6] = n;
            need[7] = E.mul({d[0], C, 2}); nbuf = 8;
            break;
        }
        case SPDM_OPT_FILM_BWD: {
            if (!E.positive({0, 1, 2, 3, 4})) return E.bad("film_bwd: B, HW, C, t_count, T must be positive");
            const int64_t B = d[0], C = d[2];
            if (!pow2_le512(C)) return E.bad("film_bwd: C must be a power of two <= 512 (got %lld)", (long long)C);
            if (d[3] != 1 && d[3] != B) return E.bad("film_bwd: t_count must be 1 or B");
            if ((q.d_buf[2] == nullptr) != (q.d_buf[6] == nullptr)) return E.bad("film_bwd: film and dfilm go together");
            const uint64_t n = E.mul({B, d[1], C});
            need[0] = n; need[1] = E.mul({d[4], C}); need[2] = E.mul({B, 2, C}); optional[2] = true; need[3] = need[4] = n;
            need[5] = E.mul({B, C}); need[6] = need[2]; optional[6] = true; nbuf = 7;
            idx_n[0] = d[3]; idx_lim[0] = d[4];
            break;
        }
        case SPDM_OPT_MSE:
            if (!E.positive({0, 1, 2, 3, 4}) || d[5] + d[1] > d[3] || d[6] + d[2] > d[4])
                return E.bad("mse: B, H0, D, Hp, Wp positive, lh + H0 <= Hp and lw + D <= Wp required");
            need[0] = need[3] = E.mul({d[0], d[3], d[4]}); need[1] = need[4] = E.mul({d[0], d[1], d[2]}); need[2] = 1;
            optional[4] = true; nbuf = 5;
            break;
        case SPDM_OPT_POOL_BWD:
            if (!E.positive({0, 1, 2, 3}) || (d[1] & 1) || (d[2] & 1)) return E.bad("pool_bwd: B, H, W, C positive and H, W even required");
            need[0] = need[2] = E.mul({d[0], d[1], d[2], d[3]}); need[1] = E.mul({d[0], d[1] / 2, d[2] / 2, d[3]}); nbuf = 3;
            break;
        case SPDM_OPT_UP_BWD:
            if (!E.positive({0, 1, 2, 3, 4}) || d[4] < d[3]) return E.bad("up_bwd: B, h, w, C positive and ld >= C required");
            need[0] = E.strided(E.mul({4, d[0], d[1], d[2]}), d[4], d[3]); need[1] = E.mul({d[0], d[1], d[2], d[3]}); nbuf = 2;
            break;
        case SPDM_OPT_MISH_BWD:
            if (!E.positive({0, 1, 2, 3}) || d[2] < d[3]) return E.bad("mish_bwd: nblk, B, cond_dim positive and ld >= cond_dim required");
            need[0] = E.strided(E.mul({d[0], d[1]}), d[2], d[3]); need[1] = need[2] = E.mul({d[1], d[3]}); nbuf = 3;
            break;
        case SPDM_OPT_LN_FWD:
        case SPDM_OPT_LN_BWD: {
            if (!E.positive({0, 1})) return E.bad("layernorm: rows and C must be positive");
            const int64_t rows = d[0], C = d[1];
            if (C != 64 && C != 128 && C != 256) return E.bad("layernorm: C must be 64, 128 or 256 (got %lld)", (long long)C);
            const uint64_t n = E.mul({rows, C});
            if (q.op == SPDM_OPT_LN_FWD) {
                need[0] = n; need[1] = need[2] = (uint64_t)C; need[3] = n; need[4] = need[5] = (uint64_t)rows; nbuf = 6;
            } else {
                need[0] = n; need[1] = need[2] = (uint64_t)rows; need[3] = (uint64_t)C; need[4] = need[5] = need[6] = n;
                optional[5] = true;
                need[7] = E.mul({(int64_t)ln_bwd_blocks(rows), 2, C}); nbuf = 8;
            }
            break;
        }
        case SPDM_OPT_GELU_BWD:
            if (!E.positive({0})) return E.bad("gelu_bwd: n must be positive");
            need[0] = need[1] = need[2] = (uint64_t)d[0]; nbuf = 3;
            break;
        case SPDM_OPT_ATTN_FWD_LSE:
        case SPDM_OPT_ATTN_BWD: {
            if (!E.positive({0, 1, 2, 3})) return E.bad("attention: B, L, C, heads must be positive");
            if (!attn_train_supported((int)d[1], (int)d[2], (int)d[3]))
                return E.bad("attention: L %lld, C %lld, heads %lld not supported (L <= 512, C / heads in {16, 32, 64}, LDS)",
                        (long long)d[1], (long long)d[2], (long long)d[3]);
            const uint64_t nq = E.mul({d[0], d[1], 3, d[2]}), no = E.mul({d[0], d[1], d[2]}), nl = E.mul({d[0], d[3], d[1]});
            if (q.op == SPDM_OPT_ATTN_FWD_LSE) { need[0] = nq; need[1] = no; need[2] = nl; nbuf = 3; }
            else { need[0] = nq; need[1] = need[2] = no; need[3] = nl; need[4] = nq; nbuf = 5; }
            break;
        }
        case SPDM_OPT_SIMPLE_TAIL_BWD: {
            if (!E.positive({0, 1, 2, 3, 4, 5})) return E.bad("simple_tail_bwd: B, HW, Co, Cr, Cz, cemb_ld must be positive");
            const int64_t Co = d[2], Cr = d[3], Cz = d[4];
            if (Co % 64 != 0 || Co > 512 || Cr > Cz || Cz > Co || Cr + 32 > Co || d[5] < 32)
                return E.bad("simple_tail_bwd: Co a multiple of 64 <= 512, Cr <= Cz <= Co, Cr + 32 <= Co and cemb_ld >= 32 required");
            need[0] = E.mul({d[0], d[1], Co}); need[1] = E.mul({d[0], d[1], Cz}); need[2] = E.mul({d[0], Cr});
            need[3] = E.strided((uint64_t)d[0], d[5], 32); nbuf = 4;
            break;
        }
        case SPDM_OPT_SILU_BWD:
            if (!E.positive({0, 1, 2}) || d[2] < d[1]) return E.bad("silu_bwd: B, cond_dim positive and ld >= cond_dim required");
            need[0] = E.strided((uint64_t)d[0], d[2], d[1]); need[1] = need[2] = E.mul({d[0], d[1]}); nbuf = 3;
            break;
    }
    SPDM_TRY(E.buffers(q.d_buf, q.cap, SPDM_OP_TRAIN_BUFS));
    static const char* const idx_name[SPDM_OP_TRAIN_IDX] = {"h_idx[0]", "h_idx[1]"};
    for (int k = 0; k < SPDM_OP_TRAIN_IDX; ++k) SPDM_TRY(E.indices(idx_name[k], q.h_idx[k], q.n_idx[k], idx_n[k], idx_lim[k]));
    if (q.op == SPDM_OPT_GN_BWD_MAPPED) {                                   // a channel map names each storage lane once
        bool seen[512] = {};
        for (int64_t i = 0; i < idx_n[0]; ++i) {
            if (seen[q.h_idx[0][i]]) return E.bad("gn_bwd_mapped: pos names lane %d twice", q.h_idx[0][i]);
            seen[q.h_idx[0][i]] = true;
        }
    }
    // ---- the device from here on ----
    OpDev dev;
    const int* di[SPDM_OP_TRAIN_IDX] = {nullptr, nullptr};
    for (int k = 0; k < SPDM_OP_TRAIN_IDX; ++k) SPDM_TRY(dev.upload_ints(q.h_idx[k], idx_n[k], &di[k]));
    float* partial = nullptr;
    SPDM_TRY(dev.nan_scratch(ws.slab, &partial));
    float* const* b = q.d_buf;
    const int i0 = (int)d[0], i1 = (int)d[1], i2 = (int)d[2], i3 = (int)d[3], i4 = (int)d[4], i5 = (int)d[5], i6 = (int)d[6];
    hipStream_t s = nullptr;
    hipError_t el = hipSuccess;
    switch (q.op) {
        case SPDM_OPT_WGRAD:
            el = launch_wgrad(b[0], (int)d[7], b[1], (int)d[8], (long long)M, i1, i2, i3, i4, i5, i6, partial, TrainPass::WGRAD_BUDGET, b[2], s);
            q.info[0] = ws.nch; q.info[1] = ws.wrows;
            break;
        case SPDM_OPT_WGRAD_MAPPED:
            el = launch_wgrad_mapped(b[0], b[1], (long long)M, i1, i2, i3, i4, i5, di[0], i6, di[1], (int)d[7], partial,
                                     TrainPass::WGRAD_BUDGET, b[2], s);
            q.info[0] = ws.nch; q.info[1] = ws.wrows;
            break;
        case SPDM_OPT_COLSUM: el = launch_colsum(b[0], i2, (long long)d[0], i1, b[1], s); break;
        case SPDM_OPT_GN_STATS:
            el = i2 == 0 ? launch_gn_stats(b[0], i0, i1, b[1], b[2], s) : launch_gn_stats_real(b[0], i0, i1, i2, b[1], b[2], s);
            break;
        case SPDM_OPT_GN_BWD: el = launch_gn_bwd(b[0], b[1], b[2], b[3], b[4], b[5], i3, i0, i1, i2, b[6], b[7], s); break;
        case SPDM_OPT_FILM_BWD: el = launch_film_bwd(b[0], b[1], di[0], i3, b[2], b[3], i0, i1, i2, b[4], b[5], b[6], s); break;
        case SPDM_OPT_MSE: el = launch_mse(b[0], b[1], i0, i1, i2, i3, i4, i5, i6, b[2], b[3], b[4], s); break;
        case SPDM_OPT_POOL_BWD: el = launch_pool_bwd(b[0], b[1], i0, i1, i2, i3, b[2], s); break;
        case SPDM_OPT_UP_BWD: el = launch_up_bwd(b[0], i4, i0, i1, i2, i3, b[1], s); break;
        case SPDM_OPT_MISH_BWD: el = launch_mish_bwd(b[0], i0, i1, i2, b[1], i3, b[2], s); break;
        case SPDM_OPT_LN_FWD: el = launch_ln_fwd(b[0], b[1], b[2], (long long)d[0], i1, b[3], b[4], b[5], s); break;
        case SPDM_OPT_LN_BWD:
            el = launch_ln_bwd(b[0], b[1], b[2], b[3], b[4], b[5], (long long)d[0], i1, b[6], b[7], s);
            q.info[0] = ln_bwd_blocks((long long)d[0]);
            break;
        case SPDM_OPT_GELU_BWD: el = launch_gelu_bwd(b[0], b[1], (size_t)d[0], b[2], s); break;
        case SPDM_OPT_ATTN_FWD_LSE: el = launch_attn_fwd_lse(b[0], b[1], b[2], i0, i1, i2, i3, s); break;
        case SPDM_OPT_ATTN_BWD: el = launch_attn_bwd(b[0], b[1], b[2], b[3], b[4], i0, i1, i2, i3, s); break;
        case SPDM_OPT_GN_BWD_MAPPED:
            el = launch_gn_bwd_mapped(b[0], b[1], b[2], b[3], b[4], b[5], i3, i0, i1, i2, di[0], i4, b[6], b[7], s);
            break;
        case SPDM_OPT_SIMPLE_TAIL_BWD: el = launch_simple_tail_bwd(b[0], i0, i1, i2, i3, i4, b[1], b[2], b[3], i5, s); break;
        case SPDM_OPT_SILU_BWD: el = launch_silu_bwd(b[0], i2, b[1], i0, i1, b[2], s); break;
    }
    return op_finish(E.hook, q.op, el);
}

// A pending GroupNorm as the op-level hooks take it (spdm_op_stream_gn, include/spdm.h) -> the StatsRef its consumer reads, checked
// host-side: source k of the checker's op, B samples of HW rows, C channels (0: the op takes none there), `aff` floats of
// gamma / beta.  Without statistics *st is the empty reference.
static int op_pending_gn(const OpCheck& E, int k, const spdm_op_stream_gn& g, int64_t B, int64_t C, int64_t HW, int64_t aff, StatsRef* st) {
    const int op = E.op;
    *st = StatsRef{nullptr, 0, 1, 1, (int)HW, 0.0};
    if (C == 0 || !g.d_stats) {
        if (g.d_stats) return E.bad("op %d takes no pending GroupNorm on source %d; gn[%d] must be empty", op, k, k);
        if (g.stats_cap || g.slots || g.m_tile || g.n_tiles || g.cnorm || g.d_gamma || g.d_beta || g.affine_cap)
            return E.bad("op %d: gn[%d] has no statistics; its other fields must be empty", op, k);
        return SPDM_OK;
    }
    if (g.slots < 1 || g.m_tile < 1 || g.n_tiles < 1) return E.bad("op %d: gn[%d] needs slots, m_tile and n_tiles >= 1", op, k);
    if (g.cnorm < 1 || g.cnorm > C) return E.bad("op %d: gn[%d].cnorm %d outside [1, %lld]", op, k, g.cnorm, (long long)C);
    if (!g.d_gamma || !g.d_beta) return E.bad("op %d: gn[%d] needs gamma and beta", op, k);
    if (g.affine_cap < (uint64_t)aff)
        return E.bad("op %d: gn[%d] gamma / beta hold %llu floats, the launch needs %lld", op, k, (unsigned long long)g.affine_cap, (long long)aff);
    // the slots sample b's consumer adds: tiles first .. last of its rows, n_tiles each (sample_mean_rstd_wave)
    const int64_t mt = g.m_tile;
    int64_t reads = ((HW + mt - 2) / mt + 1) * g.n_tiles;                  // the bound over every alignment
    if (std::min<int64_t>(B, mt) <= (1 << 20)) {                            // the alignments repeat with period <= m_tile
        reads = 0;
        for (int64_t b = 0; b < std::min<int64_t>(B, mt); ++b)
            reads = std::max<int64_t>(reads, ((b * HW + HW - 1) / mt - (b * HW) / mt + 1) * g.n_tiles);
    }
    if (g.slots < reads) return E.bad("op %d: gn[%d] has %d slots per sample, the consumer reads %lld", op, k, g.slots, (long long)reads);
    OpCheck own(E.hook, op);                                               // (this extent alone: the caller reports its own)
    const uint64_t cap = own.mul({B, g.slots, 2});
    SPDM_TRY(own.fits());
    if (g.stats_cap < cap) return E.bad("op %d: gn[%d] statistics hold %llu doubles, the launch needs %llu", op, k, (unsigned long long)g.stats_cap, (unsigned long long)cap);
    *st = StatsRef{g.d_stats, g.slots, g.m_tile, g.n_tiles, (int)HW, 1.0 / ((double)g.cnorm * (double)HW)};
    return SPDM_OK;
}

// op-level test hook: one launch_* of elementwise.hip (the streaming kernels of the forward / sampling path) on the caller's tensors
// (include/spdm.h).  Validate, upload the host integers, build AffineSrc / StatsRef / StepArgs, launch, synchronise.
extern "C" int spdm_op_stream(spdm_op_stream_args* p) {
    if (!p) return fail(SPDM_ERR_INVALID, "op_stream: null argument");
    spdm_op_stream_args& q = *p;
    for (int i = 0; i < 4; ++i) q.info[i] = -1;
    OpCheck E("op_stream", q.op);
    static const int n_dims[SPDM_OPS_COUNT] = {11, 4, 5, 5, 5, 2, 3, 3, 1, 3, 9, 4, 14};
    const int64_t* d = q.dim;
    SPDM_TRY(E.dims(d, SPDM_OP_STREAM_DIMS, n_dims, SPDM_OPS_COUNT, -2, q.op == SPDM_OPS_CONV_IN ? 8 : -1));      // conv_in's adv
    auto& need = E.need;
    auto& optional = E.optional;
    auto& absent = E.absent;
    int& nbuf = E.nbuf;
    int64_t idx_n = 0, idx_lim = 0;                 // entries of h_idx[0] (0: the op takes none), each below idx_lim
    int64_t gn_C[SPDM_OP_STREAM_GN] = {0, 0}, gn_HW[SPDM_OP_STREAM_GN] = {0, 0}, gn_aff[SPDM_OP_STREAM_GN] = {0, 0};   // gn_C == 0: not taken
    int64_t B = d[0];
    uint64_t stats_need = 0;                        // doubles of d_stats_out (0: the op writes none)
    bool stats_optional = false, words = false;
    int parts = 0, slots_out = 0, rows = 0;
    switch (q.op) {
        case SPDM_OPS_CONV_IN: {
            if (!E.positive({0, 1, 2, 3, 4})) return E.bad("conv_in: B, H0, D, Hp, Wp must be positive");
            if (d[5] + d[1] > d[3] || d[6] + d[2] > d[4]) return E.bad("conv_in: lh + H0 <= Hp and lw + D <= Wp required");
            const uint64_t HW = E.mul({d[3], d[4]});
            if (!E.ok || (HW + 8) * sizeof(float) > 64 * 1024) return E.bad("conv_in: the padded image exceeds the LDS (Hp Wp + 8 floats in 64 KiB)");
            if (d[8] == -2) {
                if (d[9] != 0 || d[10] != 0) return E.bad("conv_in: adv -2 takes n_steps = step0 = 0");
            } else {
                if (d[9] < 1 || d[10] >= d[9] || d[8] > d[9]) return E.bad("conv_in: n_steps >= 1, 0 <= step0 < n_steps and adv <= n_steps required");
                idx_n = d[9]; idx_lim = OpCheck::ANY_INDEX;
                words = true;
            }
            need[0] = E.mul({B, d[1], d[2]}); need[1] = 9 * 64; need[2] = E.mul({B, (int64_t)HW, 64}); nbuf = 3;
            parts = conv_in_parts((int)d[3], (int)d[4], (int)(d[7] > 0 ? d[7] : B));
            slots_out = stats_slots((int)HW, (int)HW / parts, 1);
            stats_need = E.mul({B, slots_out, 2});
            break;
        }
        case SPDM_OPS_POOL:
            if (!E.positive({0, 1, 2, 3}) || (d[1] & 1) || (d[2] & 1)) return E.bad("pool: B, H, W, C positive and H, W even required");
            if (d[3] % 4 != 0 || d[3] > 1024) return E.bad("pool: C must be a multiple of 4 <= 1024 (got %lld)", (long long)d[3]);
            need[0] = E.mul({B, d[1], d[2], d[3]}); need[1] = E.mul({B, d[1] / 2, d[2] / 2, d[3]}); nbuf = 2;
            gn_C[0] = gn_aff[0] = d[3]; gn_HW[0] = (int64_t)E.mul({d[1], d[2]});
            break;
        case SPDM_OPS_UPCAT: {
            if (!E.positive({0, 1, 2, 3})) return E.bad("upcat: B, Hin, Win, Cu must be positive");
            const int64_t Cu = d[3], Cs = d[4];
            if (Cu % 4 != 0 || Cs % 4 != 0 || Cu + Cs > 1024) return E.bad("upcat: Cu and Cs must be multiples of 4 with Cu + Cs <= 1024");
            const int64_t HWi = (int64_t)E.mul({d[1], d[2]}), HWo = (int64_t)E.mul({4, d[1], d[2]});
            need[0] = E.mul({B, HWi, Cu}); need[1] = Cs ? E.mul({B, HWo, Cs}) : 0; absent[1] = Cs == 0;
            need[2] = E.mul({B, HWo, Cu + Cs}); nbuf = 3;
            gn_C[0] = gn_aff[0] = Cu; gn_HW[0] = HWi;
            gn_C[1] = gn_aff[1] = Cs; gn_HW[1] = HWo;
            break;
        }
        case SPDM_OPS_FILM_APPLY:
        case SPDM_OPS_FILM_COEF: {
            if (!E.positive({0, 1, 2, 3, 4})) return E.bad("film: B, HW, C, t_count, T must be positive");
            const int64_t C = d[2];
            const bool apply = q.op == SPDM_OPS_FILM_APPLY;
            if (apply && (C % 4 != 0 || C > 1024 || 256 % (C / 4) != 0)) return E.bad("film_apply: C / 4 must divide 256 (got C = %lld)", (long long)C);
            if (d[3] != 1 && d[3] != B) return E.bad("film: t_count must be 1 or B");
            const int it = apply ? 1 : 0;                                       // buffer index of temb
            if (apply) need[0] = E.mul({B, d[1], C});
            need[it] = E.mul({d[4], C}); optional[it] = true;
            need[it + 1] = E.mul({B, 2, C}); optional[it + 1] = true;
            need[it + 2] = apply ? need[0] : need[it + 1]; nbuf = it + 3;
            if (q.d_buf[it]) { idx_n = d[3]; idx_lim = d[4]; }
            else if (d[3] != 1 || d[4] != 1) return E.bad("film: without temb, t_count = T = 1");
            gn_C[0] = gn_aff[0] = C; gn_HW[0] = d[1];
            if (apply) {
                stats_need = E.mul({B, d[1], 2}); stats_optional = true;
                if (q.d_stats_out && !(C == 64 || C == 128 || C == 256)) return E.bad("film_apply: row statistics need C 64, 128 or 256 (got %lld)", (long long)C);
            }
            break;
        }
        case SPDM_OPS_LAYERNORM:
            if (!E.positive({0, 1})) return E.bad("layernorm: rows and C must be positive");
            if (d[1] != 64 && d[1] != 128 && d[1] != 256 && d[1] != 512) return E.bad("layernorm: C must be 64, 128, 256 or 512 (got %lld)", (long long)d[1]);
            need[0] = need[3] = E.mul({d[0], d[1]}); need[1] = need[2] = (uint64_t)d[1]; nbuf = 4;
            break;
        case SPDM_OPS_MISH_PAD:
        case SPDM_OPS_SILU_PAD:
            if (!E.positive({0, 1, 2}) || d[2] < d[1]) return E.bad("mish_pad / silu_pad: B, cond_dim positive and Kp >= cond_dim required");
            need[0] = E.mul({B, d[1]}); need[1] = E.mul({B, d[2]}); nbuf = 2;
            break;
        case SPDM_OPS_SILU:
            if (!E.positive({0})) return E.bad("silu: n must be positive");
            need[0] = need[1] = (uint64_t)d[0]; nbuf = 2;
            break;
        case SPDM_OPS_DC_FINISH:
            if (!E.positive({0, 1, 2})) return E.bad("dc_finish: B, HW, C must be positive");
            if (d[2] % 4 != 0 || d[2] > 1024) return E.bad("dc_finish: C must be a multiple of 4 <= 1024 (got %lld)", (long long)d[2]);
            need[0] = need[1] = need[2] = E.mul({B, d[1], d[2]}); optional[1] = true; nbuf = 3;
            gn_C[0] = gn_aff[0] = d[2]; gn_HW[0] = d[1];
            break;
        case SPDM_OPS_SIMPLE_TAIL: {
            if (!E.positive({0, 1, 2, 3, 4, 5, 6, 7, 8})) return E.bad("simple_tail: every dimension must be positive");
            const int64_t Co = d[2], Cr = d[3], Cs = d[4], tld = d[5], cld = d[6];
            if (Co % 4 || Cr % 4 || Cs % 4 || tld % 4 || cld % 4) return E.bad("simple_tail: Co, Cr, src_C, temb_ld, cemb_ld must be multiples of 4");
            if (Co > 1024 || Cr > Cs || Cr + 32 > Co || tld < Cr || cld < 32)
                return E.bad("simple_tail: Co <= 1024, Cr <= src_C, Cr + 32 <= Co, temb_ld >= Cr and cemb_ld >= 32 required");
            if (d[7] != 1 && d[7] != B) return E.bad("simple_tail: t_count must be 1 or B");
            need[0] = E.mul({B, d[1], Cs}); need[1] = E.strided((uint64_t)d[8], tld, Cr); need[2] = E.strided((uint64_t)B, cld, 32);
            need[3] = E.mul({B, d[1], Co}); nbuf = 4;
            idx_n = d[7]; idx_lim = d[8];
            gn_C[0] = Cs; gn_aff[0] = Cr; gn_HW[0] = d[1];
            break;
        }
        case SPDM_OPS_SPLITK_COMBINE: {
            if (!E.positive({0, 1, 2}) || d[3] < 2) return E.bad("splitk_combine: B, HW, N positive and ksplit >= 2 required");
            if (d[2] % 4 != 0) return E.bad("splitk_combine: N must be a multiple of 4 (got %lld)", (long long)d[2]);
            need[1] = E.mul({B, d[1], d[2]}); need[0] = E.mul({d[3], B, d[1], d[2]}); nbuf = 2;
            rows = combine_rows((int)d[1], (int)d[2]);
            if (d[1] % rows != 0) return E.bad("splitk_combine: rows per workgroup do not divide HW");
            slots_out = stats_slots((int)d[1], rows, 1);
            stats_need = E.mul({B, slots_out, 2});
            break;
        }
        case SPDM_OPS_OUT_STEP: {
            if (!E.positive({0, 1, 2, 3, 4, 10})) return E.bad("out_step: B, H0, D, Hp, Wp, n_steps must be positive");
            if (d[5] + d[1] > d[3] || d[6] + d[2] > d[4]) return E.bad("out_step: lh + H0 <= Hp and lw + D <= Wp required");
            const int64_t mode = d[8], inp_h = d[11];
            if (d[7] > 1 || mode > 2 || d[12] > 1 || d[13] > 1) return E.bad("out_step: kind, inpaint_per_sample, indirect are 0 / 1 and mode 0, 1 or 2");
            if (d[9] >= d[10]) return E.bad("out_step: step %lld outside [0, %lld)", (long long)d[9], (long long)d[10]);
            if (inp_h > d[1]) return E.bad("out_step: inp_h must not exceed H0");
            const uint64_t El = E.mul({B, d[1], d[2]});
            need[0] = E.mul({B, d[3], d[4], 64}); need[1] = 64; need[2] = need[3] = El; need[4] = E.mul({d[10], 6});
            need[5] = E.mul({d[10], (int64_t)El}); need[6] = E.mul({d[12] ? B : 1, inp_h ? inp_h : 1, d[2]}); need[7] = E.mul({d[10] + 1, (int64_t)El});
            nbuf = 8;
            absent[0] = absent[1] = mode == 2;
            absent[2] = mode == 1;
            for (int i = 3; i < 8; ++i) absent[i] = mode == 0;
            optional[5] = optional[7] = true;
            if (mode != 0 && inp_h == 0) absent[6] = true;
            words = true;
            break;
        }
    }
    SPDM_TRY(E.buffers(q.d_buf, q.cap, SPDM_OP_STREAM_BUFS));
    SPDM_TRY(E.indices("h_idx[0]", q.h_idx[0], q.n_idx[0], idx_n, idx_lim));
    StatsRef st[SPDM_OP_STREAM_GN];
    for (int k = 0; k < SPDM_OP_STREAM_GN; ++k) SPDM_TRY(op_pending_gn(E, k, q.gn[k], B, gn_C[k], gn_HW[k], gn_aff[k], &st[k]));
    SPDM_TRY(E.doubles("d_stats_out", q.d_stats_out, q.stats_out_cap, stats_need, stats_optional));
    if (words != (q.d_words != nullptr)) return E.bad("op %d with these arguments %s d_words", q.op, words ? "needs" : "does not take");
    // ---- the device from here on ----
    OpDev dev;
    const int* di = nullptr;
    SPDM_TRY(dev.upload_ints(q.h_idx[0], idx_n, &di));
    if (words) {
        const int w3[3] = {(int)(q.op == SPDM_OPS_CONV_IN ? d[10] : d[9]), -1, 0};
        HIP_TRY(hipMemcpy(q.d_words, w3, sizeof(w3), hipMemcpyHostToDevice));
    }
    float* const* b = q.d_buf;
    const int i0 = (int)d[0], i1 = (int)d[1], i2 = (int)d[2], i3 = (int)d[3], i4 = (int)d[4], i5 = (int)d[5], i6 = (int)d[6];
    auto asrc = [&](int k, const float* x, int C) { return AffineSrc{x, C, st[k], q.gn[k].d_gamma, q.gn[k].d_beta}; };
    hipStream_t s = nullptr;
    hipError_t el = hipSuccess;
    switch (q.op) {
        case SPDM_OPS_CONV_IN:
            el = launch_conv_in(b[0], b[1], b[2], q.d_stats_out, i0, i1, i2, i3, i4, i5, i6, q.d_words, q.d_words ? q.d_words + 1 : nullptr, di,
                                (int)d[9], (int)d[8], s, (int)d[7]);
            q.info[0] = parts; q.info[1] = slots_out;
            break;
        case SPDM_OPS_POOL: el = launch_pool(asrc(0, b[0], i3), b[1], i0, i1, i2, s); break;
        case SPDM_OPS_UPCAT: el = launch_upcat(asrc(0, b[0], i3), asrc(1, b[1], i4), b[2], i0, i1, i2, s); break;
        case SPDM_OPS_FILM_APPLY:
            if (!b[1] && !b[2] && !q.gn[0].d_stats && !q.d_stats_out) el = launch_gn_apply(asrc(0, b[0], i2), b[3], i0, i1, s);
            else el = launch_film_apply(asrc(0, b[0], i2), b[1], di, i3, b[2], b[3], q.d_stats_out, i0, i1, s);
            break;
        case SPDM_OPS_FILM_COEF: el = launch_film_coef(asrc(0, nullptr, i2), b[0], di, i3, b[1], b[2], i0, s); break;
        case SPDM_OPS_LAYERNORM: el = launch_layernorm(b[0], b[1], b[2], b[3], i0, i1, s); break;
        case SPDM_OPS_MISH_PAD: el = launch_mish_pad(b[0], b[1], i0, i1, i2, s); break;
        case SPDM_OPS_SILU_PAD: el = launch_silu_pad(b[0], b[1], i0, i1, i2, s); break;
        case SPDM_OPS_SILU: el = launch_silu(b[0], b[1], (size_t)d[0], s); break;
        case SPDM_OPS_DC_FINISH: el = launch_dc_finish(asrc(0, b[0], i2), b[1], b[2], i0, i1, s); break;
        case SPDM_OPS_SIMPLE_TAIL:
            el = launch_simple_tail(asrc(0, b[0], i4), i3, b[1], i5, di, (int)d[7], b[2], i6, b[3], i2, i0, i1, s);
            break;
        case SPDM_OPS_SPLITK_COMBINE:
            el = launch_splitk_combine(b[0], i3, b[1], i0 * i1, i2, i1, q.d_stats_out, s);
            q.info[0] = rows; q.info[1] = slots_out;
            break;
        case SPDM_OPS_OUT_STEP: {
            const unsigned long long rng[2] = {q.seed, q.first_index};
            StepArgs a{};
            SPDM_TRY(dev.upload(rng, sizeof(rng), &a.rng_dev));
            a.feat = b[0]; a.w = b[1]; a.bias = q.bias; a.x = b[3];
            a.eps_out = d[8] == 0 ? b[2] : nullptr;
            a.eps_in = d[8] == 2 ? b[2] : nullptr;
            a.coef = b[4]; a.step_dev = q.d_words; a.kind = (int)d[7];
            a.flag_dev = q.d_words + 2;
            a.inp_h = (int)d[11]; a.inpaint_per_sample = (int)d[12];
            if (d[13]) {
                const void* ptrs[3] = {b[6], b[5], b[7]};
                SPDM_TRY(dev.upload(ptrs, sizeof(ptrs), &a.ptrs_dev));
            } else {
                a.inpaint = b[6]; a.noise = b[5]; a.history = b[7];
            }
            a.B = i0; a.H0 = i1; a.D = i2; a.Hp = i3; a.Wp = i4; a.lh = i5; a.lw = i6;
            el = launch_out_step(a, s);
            break;
        }
    }
    return op_finish(E.hook, q.op, el);
}

// op-level test hook: one launch_* of the autoencoder's decoder stage (decoder.hip), launch_add, or launch_wgrad under the slab
// budgets of the encoder / decoder passes, on the caller's tensors (include/spdm.h).  Validate, allocate the product's scratch
// (NaN-filled), launch, synchronise.
extern "C" int spdm_op_frame(spdm_op_frame_args* p) {
    if (!p) return fail(SPDM_ERR_INVALID, "op_frame: null argument");
    spdm_op_frame_args& q = *p;
    for (int i = 0; i < 4; ++i) q.info[i] = -1;
    OpCheck E("op_frame", q.op);
    static const int n_dims[SPDM_OPF_COUNT] = {2, 1, 1, 1, 1, 1, 1, 2, 1, 1, 1, 1, 3, 2, 0, 2};
    const int64_t* d = q.dim;
    SPDM_TRY(E.dims(d, SPDM_OP_FRAME_DIMS, n_dims, SPDM_OPF_COUNT));
    auto& need = E.need;
    auto& absent = E.absent;                       // a buffer that must be NULL in this call (DEC_CONVS without train)
    int& nbuf = E.nbuf;
    uint64_t need_sq = 0;                          // extent of d_sq; 0: the op does not take it
    uint64_t scratch = 0;                          // floats of the hook's own scratch
    // (the loss is formed once over ALL frames of a call, not per chunk)
    const bool frames = q.op <= SPDM_OPF_ENC_CONV1_WGRAD || (q.op >= SPDM_OPF_DEC_CONVS && q.op <= SPDM_OPF_DEC_DGRAD4 && q.op != SPDM_OPF_DEC_LOSS);
    if (frames && (d[0] < 1 || d[0] > FRAME_CHUNK)) return E.bad("op %d: n = %lld outside [1, %d] frames", q.op, (long long)d[0], FRAME_CHUNK);
    const int64_t n = d[0];
    int wCo = 0, wCi = 0;
    WgradSlabs ws{0, 0, 0};
    size_t budget = 0;
    switch (q.op) {
        case SPDM_OPF_ENC_CONVS:
        case SPDM_OPF_ENC_KINKS: {
            if (q.op == SPDM_OPF_ENC_CONVS && d[1] > 1) return E.bad("enc_convs: train must be 0 or 1");
            const uint64_t w[9] = {E.mul({n, FRAME_PIX}), 16 * 3 * 4, 16, 32 * 16 * 4, 32, 64 * 32 * 4, 64, E.mul({n, FRAME_FEAT}), E.mul({n, ENC_X3})};
            for (int i = 0; i < 9; ++i) need[i] = w[i];
            nbuf = 9;
            if (q.op == SPDM_OPF_ENC_CONVS && d[1] == 0) absent[8] = true;
            break;
        }
        case SPDM_OPF_ENC_X2: need[0] = E.mul({n, FRAME_PIX}); need[1] = 192; need[2] = 16; need[3] = E.mul({n, ENC_X2}); nbuf = 4; break;
        case SPDM_OPF_ENC_DZ3: need[0] = need[1] = need[2] = E.mul({n, FRAME_FEAT}); nbuf = 3; break;
        case SPDM_OPF_ENC_DZ2: need[0] = need[1] = need[2] = E.mul({n, ENC_X3}); nbuf = 3; break;
        case SPDM_OPF_ENC_CONV1_WGRAD:
            need[0] = E.mul({n, FRAME_PIX}); need[1] = need[2] = E.mul({n, ENC_X2}); need[3] = 192; need[4] = 16; nbuf = 5;
            scratch = (uint64_t)encoder_conv1_wgrad_blocks((int)n) * 208;           // c1_part: [blocks(FRAME_CHUNK)][208] in the product
            break;
        case SPDM_OPF_DEC_CONVS: {
            if (d[1] > 1) return E.bad("dec_convs: train must be 0 or 1");
            const uint64_t w[7] = {E.mul({n, FRAME_FEAT}), 64 * 4 * 32, 32, 32 * 4 * 16, 16, 16 * 4 * 3, 3};
            for (int i = 0; i < 7; ++i) need[i] = w[i];
            need[7] = need[8] = E.mul({n, FRAME_PIX}); need[9] = E.mul({n, DEC_A1}); need[10] = E.mul({n, DEC_A2}); nbuf = 11;
            if (d[1] == 0) absent[8] = absent[9] = absent[10] = true;
            else need_sq = (uint64_t)n;
            if (d[1] == 0 && q.d_sq) return E.bad("dec_convs: d_sq must be null without train");
            break;
        }
        case SPDM_OPF_DEC_KINKS: {
            const uint64_t w[9] = {E.mul({n, FRAME_LATENT}), (uint64_t)FRAME_FEAT * FRAME_LATENT, FRAME_FEAT, 64 * 4 * 32, 32, 32 * 4 * 16, 16,
                                   E.mul({n, DEC_A1}), E.mul({n, DEC_A2})};
            for (int i = 0; i < 9; ++i) need[i] = w[i];
            nbuf = 9;
            break;
        }
        case SPDM_OPF_DEC_LOSS:
            if (n < 1) return E.bad("dec_loss: n must be positive");
            need[0] = 1; nbuf = 1; need_sq = (uint64_t)n;
            break;
        case SPDM_OPF_DEC_BWD6:
            if (!std::isfinite(q.scale)) return E.bad("dec_bwd6: scale is not finite");
            need[0] = need[1] = E.mul({n, FRAME_PIX}); need[2] = need[4] = E.mul({n, DEC_A2}); need[3] = need[5] = 192; need[6] = 3; nbuf = 7;
            scratch = (uint64_t)n * 208;                                          // w6_part: [FRAME_CHUNK][208] in the product
            break;
        case SPDM_OPF_DEC_DGRAD4:
            need[0] = E.mul({n, 576, 64}); need[1] = need[3] = E.mul({n, DEC_A1}); need[2] = 32 * 64; nbuf = 4;
            break;
        case SPDM_OPF_DEC_COLSUM: {
            const int64_t M = d[0], C = d[1], fold = d[2];
            if (M < 1) return E.bad("dec_colsum: M must be positive");
            if (!((fold == 4 && (C == 64 || C == 128)) || (fold == 1 && C == FRAME_FEAT)))
                return E.bad("dec_colsum: (C, fold) must be (64, 4), (128, 4) or (9216, 1)");
            const int64_t max_m = (int64_t)FRAME_CHUNK * (fold == 1 ? 1 : C == 64 ? 576 : 144);
            if (M > max_m) return E.bad("dec_colsum: M = %lld beyond the %lld rows of one chunk", (long long)M, (long long)max_m);
            need[0] = E.mul({M, C}); need[1] = (uint64_t)(C / fold); nbuf = 2;
            scratch = (uint64_t)decoder_colsum_slabs(M) * (uint64_t)C;
            if (scratch > (uint64_t)decoder_colsum_slabs(FRAME_CHUNK) * FRAME_FEAT) return E.bad("dec_colsum: the slabs exceed cs_part");
            break;
        }
        case SPDM_OPF_DEC_UNPERM_CONV:
            if (!((d[0] == 64 && d[1] == 32) || (d[0] == 32 && d[1] == 16) || (d[0] == 16 && d[1] == 3)))
                return E.bad("dec_unperm_conv: (cin, cout) must be (64, 32), (32, 16) or (16, 3)");
            need[0] = need[1] = (uint64_t)(d[0] * d[1] * 4); nbuf = 2;
            break;
        case SPDM_OPF_DEC_UNPERM_LINEAR: need[0] = need[1] = (uint64_t)FRAME_FEAT * FRAME_LATENT; nbuf = 2; break;
        case SPDM_OPF_ADD:
            if (d[0] < 1) return E.bad("add: n must be positive");
            need[0] = need[1] = (uint64_t)d[0]; nbuf = 2;
            break;
        case SPDM_OPF_FRAME_WGRAD: {
            static const struct { int Co, Ci, rows_per_frame; } W[6] = {{FRAME_LATENT, FRAME_FEAT, 1}, {64, 128, 144}, {32, 64, 576},
                                                                        {32, 64, 576}, {64, 128, 144}, {FRAME_FEAT, FRAME_LATENT, 1}};
            if (d[0] < 1) return E.bad("frame_wgrad: M must be positive");
            if (d[1] > 5) return E.bad("frame_wgrad: which = %lld outside [0, 5]", (long long)d[1]);
            const int k = (int)d[1];
            wCo = W[k].Co; wCi = W[k].Ci;
            const size_t budgets[6] = {FRAME_WG_FLOATS, FRAME_WG_FLOATS, FRAME_WG_FLOATS, DEC_WG_SLABS * 32 * 64, DEC_WG_SLABS * 64 * 128, FRAME_WG_FLOATS};
            budget = budgets[k];
            if (d[0] > (int64_t)FRAME_CHUNK * W[k].rows_per_frame)
                return E.bad("frame_wgrad: M = %lld beyond the %lld rows of one chunk", (long long)d[0], (long long)FRAME_CHUNK * W[k].rows_per_frame);
            need[0] = E.mul({d[0], wCo}); need[1] = E.mul({d[0], wCi}); need[2] = (uint64_t)wCo * wCi; nbuf = 3;
            if (!E.ok) break;
            ws = wgrad_slabs((long long)d[0], 1, wCo, wCi, budget);
            scratch = ws.slab;
            if (!scratch) return E.bad("frame_wgrad: the partial slabs exceed the budget");
            break;
        }
    }
    SPDM_TRY(E.buffers(q.d_buf, q.cap, SPDM_OP_FRAME_BUFS));
    SPDM_TRY(E.doubles("d_sq", q.d_sq, q.d_sq ? q.sq_cap : 0, need_sq, false));       // (sq_cap without d_sq is not looked at)
    if (q.op != SPDM_OPF_DEC_BWD6 && q.scale != 0.f) return E.bad("op %d does not take a scale; it must be 0", q.op);
    // ---- the device from here on ----
    OpDev dev;
    float* part = nullptr;
    SPDM_TRY(dev.nan_scratch(scratch, &part));
    float* const* b = q.d_buf;
    const int ni = (int)n;
    hipStream_t s = nullptr;
    hipError_t el = hipSuccess;
    switch (q.op) {
        case SPDM_OPF_ENC_CONVS:
            el = d[1] ? launch_encoder_train_convs(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], ni, s)
                      : launch_encoder_convs(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], ni, s);
            break;
        case SPDM_OPF_ENC_KINKS: el = launch_encoder_kinks(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], ni, s); break;
        case SPDM_OPF_ENC_X2: el = launch_encoder_x2(b[0], b[1], b[2], ni, b[3], s); break;
        case SPDM_OPF_ENC_DZ3: el = launch_encoder_dz3(b[0], b[1], ni, b[2], s); break;
        case SPDM_OPF_ENC_DZ2: el = launch_encoder_dz2(b[0], b[1], ni, b[2], s); break;
        case SPDM_OPF_ENC_CONV1_WGRAD:
            el = launch_encoder_conv1_wgrad(b[0], b[1], b[2], ni, part, b[3], b[4], s);
            q.info[0] = encoder_conv1_wgrad_blocks(ni);
            break;
        case SPDM_OPF_DEC_CONVS:
            el = d[1] ? launch_decoder_train_convs(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], b[9], b[10], q.d_sq, ni, s)
                      : launch_decoder_convs(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], ni, s);
            break;
        case SPDM_OPF_DEC_KINKS: el = launch_decoder_kinks(b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7], b[8], ni, s); break;
        case SPDM_OPF_DEC_LOSS: el = launch_decoder_loss(q.d_sq, ni, b[0], s); break;
        case SPDM_OPF_DEC_BWD6: el = launch_decoder_bwd6(b[0], b[1], b[2], b[3], q.scale, ni, b[4], part, b[5], b[6], s); break;
        case SPDM_OPF_DEC_DGRAD4: el = launch_decoder_dgrad4(b[0], b[1], b[2], ni, b[3], s); break;
        case SPDM_OPF_DEC_COLSUM:
            el = launch_decoder_colsum(b[0], (int)d[1], (long long)d[0], (int)(d[1] / d[2]), (int)d[2], part, b[1], s);
            q.info[0] = decoder_colsum_slab_rows((long long)d[0]); q.info[1] = decoder_colsum_slabs((long long)d[0]);
            break;
        case SPDM_OPF_DEC_UNPERM_CONV: el = launch_decoder_unperm_conv(b[0], (int)d[0], (int)d[1], b[1], s); break;
        case SPDM_OPF_DEC_UNPERM_LINEAR: el = launch_decoder_unperm_linear(b[0], b[1], s); break;
        case SPDM_OPF_ADD: el = launch_add(b[0], (size_t)d[0], b[1], s); break;
        case SPDM_OPF_FRAME_WGRAD:
            el = launch_wgrad(b[0], wCo, b[1], wCi, (long long)d[0], 1, 1, 1, wCo, wCi, 0, part, budget, b[2], s);
            q.info[0] = ws.nch; q.info[1] = ws.wrows; q.info[2] = wCo; q.info[3] = wCi;
            break;
    }
    return op_finish(E.hook, q.op, el);
}

// op-level test hook: one forward SelfAttention launch (sa_fused.hip, sa_tail.hip, attention.hip) exactly as Ctx::attention makes
// it, on the caller's tensors (include/spdm.h).  Validate -- the launcher's own refusals by asking the launcher (SaRoute::dry) --,
// lay out the weights with the loader's code, upload the timesteps, build FilmSpec / SaCrop, launch, synchronise.
extern "C" int spdm_op_sa(spdm_op_sa_args* p) {
    if (!p) return fail(SPDM_ERR_INVALID, "op_sa: null argument");
    spdm_op_sa_args& q = *p;
    for (int i = 0; i < 5; ++i) q.info[i] = -1;
    OpCheck E("op_sa", q.op);
    static const int n_dims[SPDM_OPA_COUNT] = {10, 3, 3, 3, 4};
    const int64_t* d = q.dim;
    SPDM_TRY(E.dims(d, SPDM_OP_SA_DIMS, n_dims, SPDM_OPA_COUNT));
    const bool fused = q.op == SPDM_OPA_FUSED64, core = q.op == SPDM_OPA_CORE;
    const int64_t B = fused || core ? d[0] : d[1], L = fused || core ? d[1] : d[2], C = fused ? 64 : core ? d[2] : d[0];
    if (B < 1 || L < 1) return E.bad("op %d: B and L must be positive", q.op);
    if (core ? !(C == 64 || C == 128 || C == 256) : !fused && !(C == 128 || C == 256))
        return E.bad("op %d: C = %lld (CORE: 64, 128 or 256; QKV, HEAD, TAIL: 128 or 256)", q.op, (long long)C);
    const bool crop = fused && d[3] == 1, outc = fused && d[9] == 1;
    if (fused) {
        if (d[2] > 1 || d[3] > 1 || d[9] > 1) return E.bad("fused64: no_wlds, crop and outc are 0 / 1");
        if (!crop && (d[4] || d[5] || d[6] || d[7] || d[8] || d[9])) return E.bad("fused64: without crop, H0 = D = Wp = lh = lw = outc = 0");
    }
    // a hole of launch_sa_fused64 closed here as well as there: its crop checks ran in int, so two large factors could wrap into
    // the accepted range ((lh + H0) Wp with Wp = 2^31 - 1) and the kernel would read tokens far outside the sample.  Every crop
    // dimension of an accepted crop is at most L ((lh + H0) Wp <= L, lw + D <= Wp); beyond that nothing is asked of the launcher
    if (crop)
        for (int i = 4; i <= 8; ++i)
            if (d[i] > L) return E.bad("fused64: crop dimension dim[%d] = %lld exceeds L = %lld", i, (long long)d[i], (long long)L);
    if (core && d[3] > 1) return E.bad("core: valu is 0 / 1");
    auto& need = E.need;
    auto& absent = E.absent;
    E.nbuf = SPDM_OP_SA_BUFS;                      // every op here says which of the three it does not take
    bool takes_w[SPDM_OP_SA_WEIGHTS] = {}, takes_v[SPDM_OP_SA_VECS] = {};
    const uint64_t rowsC = E.mul({B, L, C}), rows3C = E.mul({B, L, 3, C});
    switch (q.op) {
        case SPDM_OPA_FUSED64:
            need[0] = need[1] = rowsC; need[2] = crop ? E.mul({B, d[4], d[5]}) : 0;
            absent[1] = outc; absent[2] = !outc;
            for (bool& t : takes_w) t = true;
            for (bool& t : takes_v) t = true;
            break;
        case SPDM_OPA_QKV: need[0] = rowsC; need[1] = rows3C; absent[2] = true; takes_w[0] = takes_v[0] = takes_v[1] = takes_v[2] = true; break;
        case SPDM_OPA_HEAD: need[0] = need[1] = rowsC; absent[2] = true; takes_w[0] = takes_v[0] = takes_v[1] = takes_v[2] = true; break;
        case SPDM_OPA_TAIL:
            need[0] = need[1] = need[2] = rowsC;
            takes_w[1] = takes_w[2] = takes_w[3] = true;
            for (int i = 3; i < 8; ++i) takes_v[i] = true;
            break;
        case SPDM_OPA_CORE: need[0] = rows3C; need[1] = rowsC; absent[2] = true; break;
    }
    SPDM_TRY(E.buffers(q.d_buf, q.cap, SPDM_OP_SA_BUFS));
    for (int i = 0; i < SPDM_OP_SA_WEIGHTS; ++i)
        if ((q.h_w[i] != nullptr) != takes_w[i]) return E.bad("op %d %s h_w[%d]", q.op, takes_w[i] ? "needs" : "does not take", i);
    for (int i = 0; i < SPDM_OP_SA_VECS; ++i) {
        if ((q.d_vec[i] != nullptr) != takes_v[i]) return E.bad("op %d %s d_vec[%d]", q.op, takes_v[i] ? "needs" : "does not take", i);
        const uint64_t nv = (uint64_t)(i == 2 ? 3 * C : C);
        if (takes_v[i] ? q.vec_cap[i] < nv : q.vec_cap[i] != 0)
            return E.bad("op %d: d_vec[%d] holds %llu floats, the launch needs %llu", q.op, i, (unsigned long long)q.vec_cap[i], (unsigned long long)(takes_v[i] ? nv : 0));
    }
    if (outc ? (!q.d_outc_w || q.outc_w_cap < 64 || !std::isfinite(q.outc_b)) : (q.d_outc_w || q.outc_w_cap || q.outc_b != 0.f))
        return E.bad("op %d: outc's weight [64] and a finite bias go with outc = 1 only", q.op);
    // the block input's affine: coefficients from memory (ab) or a recipe the kernel evaluates (FilmSpec); a hole of the launchers
    // closed here: they take any t_count, and the kernels read t_dev[b] for every t_count but 1
    if (q.film_on != 0 && q.film_on != 1) return E.bad("film_on is 0 / 1");
    if (core && (q.d_ab || q.film_on)) return E.bad("core takes neither ab nor a FilmSpec");
    if (q.d_ab && q.film_on) return E.bad("op %d: ab and a FilmSpec are mutually exclusive", q.op);
    if (q.d_ab ? q.ab_cap < E.mul({B, 2, C}) : q.ab_cap != 0) return E.bad("op %d: ab holds %llu floats, [B 2C] are needed", q.op, (unsigned long long)q.ab_cap);
    StatsRef st{nullptr, 0, 1, 1, (int)L, 0.0};
    if (!q.film_on) {
        if (q.t_count || q.T || q.d_temb || q.temb_cap || q.h_t || q.d_film || q.film_cap) return E.bad("op %d: film_on 0, its FilmSpec fields must be empty", q.op);
        SPDM_TRY(op_pending_gn(E, 0, q.gn, B, 0, L, 0, &st));
    } else {
        if (q.t_count != 1 && q.t_count != B) return E.bad("film: t_count must be 1 or B");
        if (q.T < 1 || q.T > INT32_MAX) return E.bad("film: T must be positive");
        if (q.d_temb) {
            if (q.temb_cap < E.mul({q.T, C})) return E.bad("film: temb holds %llu floats, [T C] are needed", (unsigned long long)q.temb_cap);
            SPDM_TRY(E.indices("h_t", q.h_t, q.t_count, q.t_count, q.T));      // (temb needs the timesteps)
        } else if (q.h_t || q.temb_cap || q.t_count != 1 || q.T != 1) {
            return E.bad("film: without temb, h_t is null and t_count = T = 1");
        }
        if (q.d_film ? q.film_cap < E.mul({B, 2, C}) : q.film_cap != 0) return E.bad("film: film holds %llu floats, [B 2C] are needed", (unsigned long long)q.film_cap);
        SPDM_TRY(op_pending_gn(E, 0, q.gn, B, C, L, C, &st));
    }
    SPDM_TRY(E.fits());
    // ---- the launch, asked of the launcher twice: dry (its own refusals, before the device is touched), then for real ----
    FilmSpec fs{};
    fs.st = st; fs.gamma = q.gn.d_gamma; fs.beta = q.gn.d_beta; fs.temb = q.d_temb; fs.t_count = q.t_count; fs.film = q.d_film; fs.C = (int)C;
    const FilmSpec* fsp = q.film_on ? &fs : nullptr;
    SaCrop cr{(int)d[4], (int)d[5], (int)d[6], (int)d[7], (int)d[8], q.d_outc_w, q.outc_b, outc ? q.d_buf[2] : nullptr};
    const SaCrop* crp = crop ? &cr : nullptr;
    unsigned sw = 0;
    if (fused && d[2]) sw |= SW_SA_NO_WLDS;
    if (core && d[3]) sw |= SW_ATTN_VALU;
    const void* fw[8] = {};
    const float* wf[4] = {};
    float* const* b = q.d_buf;
    const float* const* v = q.d_vec;
    const int iB = (int)B, iL = (int)L, iC = (int)C, rows = (int)(B * L);
    hipStream_t s = nullptr;
    SaRoute r{1, -1, -1, -1, -1, -1};
    auto launch = [&]() -> hipError_t {
        switch (q.op) {
            case SPDM_OPA_FUSED64:
                return launch_sa_fused64(b[0], b[1], iB, iL, v[0], v[1], v[4], v[5], fw, v[2], v[3], v[6], v[7], q.d_ab, sw, s, fsp, crp, &r);
            case SPDM_OPA_QKV: return launch_sa_qkv(iC, b[0], b[1], rows, wf[0], v[2], v[0], v[1], q.d_ab, iL, s, fsp, &r);
            case SPDM_OPA_HEAD: return launch_sa_head(iC, b[0], b[1], rows, wf[0], v[2], v[0], v[1], q.d_ab, iL, s, fsp, &r);
            case SPDM_OPA_TAIL:
                return launch_sa_tail(iC, b[0], b[1], b[2], rows, wf[1], wf[2], wf[3], v[3], v[6], v[7], v[4], v[5], q.d_ab, iL, s, fsp, &r);
            default: return launch_attention_auto(b[0], b[1], iB, iL, iC, 4, sw, s, &r);
        }
    };
    for (int i = 0; i < 4; ++i) wf[i] = takes_w[i] ? q.h_w[i] : nullptr;      // (dry: any non-null pointer; not dereferenced)
    if (launch() != hipSuccess) return E.bad("op %d: the launcher refuses this launch (shape, route or LDS limits; kernels.h)", q.op);
    // ---- the device from here on ----
    std::vector<float> blob;                // the caller's torch-layout weights, one after the other
    spdm_tensor_index index[SPDM_OP_SA_WEIGHTS] = {};
    int n_index = 0;
    for (int i = 0; i < SPDM_OP_SA_WEIGHTS; ++i) {
        if (!takes_w[i]) continue;
        spdm_tensor_index& e = index[n_index++];
        snprintf(e.name, SPDM_NAME_MAX, "w%d", i);
        e.offset = blob.size(); e.numel = (uint64_t)(i == 0 ? 3 : 1) * C * C; e.ndim = 2; e.shape[0] = (int)((i == 0 ? 3 : 1) * C); e.shape[1] = (int)C;
        blob.insert(blob.end(), q.h_w[i], q.h_w[i] + e.numel);
    }
    OwnWeights ow(blob.size(), index, n_index);
    Recorder& R = ow.R;
    void* dfw[8] = {};
    float* dwf[4] = {};
    auto walk = [&]() {                    // Loader::attn, which starts each pass from an empty AttnW: a demoted weight leaves its
        for (void*& f : dfw) f = nullptr;  // pointers untouched in the load pass, and the plan pass had set them to its stand-in
        for (int i = 0; i < SPDM_OP_SA_WEIGHTS; ++i) {
            if (!takes_w[i]) continue;
            const std::string name = "w" + std::to_string(i);
            const int out = (int)((i == 0 ? 3 : 1) * C);
            if (C == 64) R.perm_split(name, out, &dfw[2 * i], &dfw[2 * i + 1]);
            else dwf[i] = R.linear_frag(name, out, (int)C);
        }
        return R.err;
    };
    if (n_index) {
        SPDM_TRY(ow.lay_out(blob.data(), walk));
        for (int i = 0; i < SPDM_OP_SA_WEIGHTS; ++i)
            if (takes_w[i] && !(C == 64 ? dfw[2 * i] && dfw[2 * i + 1] : dwf[i] != nullptr))
                return OwnWeights::outside("op_sa", ("h_w[" + std::to_string(i) + "]").c_str(), "the plan keeps such a block on the GEMM chain");
    }
    for (int i = 0; i < 8; ++i) fw[i] = dfw[i];
    for (int i = 0; i < 4; ++i) wf[i] = dwf[i];
    OpDev dev;
    if (q.film_on && q.d_temb) SPDM_TRY(dev.upload_ints(q.h_t, q.t_count, &fs.t_dev));
    r = SaRoute{0, -1, -1, -1, -1, -1};
    SPDM_TRY(op_finish(E.hook, q.op, launch()));
    q.info[0] = r.kernel; q.info[1] = r.waves; q.info[2] = r.grid; q.info[3] = r.wlds; q.info[4] = r.qw;
    return SPDM_OK;
}
