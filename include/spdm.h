/*
 * spdm.h -- C ABI of libspdm_hip.so: the MI355X (gfx950) denoising hot path of
 * rafaelsoStanford/State_Policy_DiffusionModel.
 *
 * The reference has no FFI/plugin registry: its boundary for this path is the
 * Python object protocol.  Each entry point below names the
 * reference call it stands behind; the Python host mirror lives in
 * state_policy_diffusionmodel_amd/{engine,diffusion,schedulers}.py and binds
 * these symbols with ctypes (INTEGRATION.md shows the stub a reference
 * maintainer would add).
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch / HIP types in signatures
 *    (`stream` is a hipStream_t passed as void*; NULL = the null stream and the
 *    call synchronises before returning, matching the reference's blocking
 *    semantics).
 *  - `d_` pointers are DEVICE pointers owned by the caller (e.g. PyTorch-ROCm
 *    tensors' data_ptr()), `h_` pointers are HOST pointers.
 *  - Tensors at the boundary use the reference's own layouts: trajectories
 *    (B,1,H,D) contiguous fp32 == (B,H,D); cond (B,1,obs_h,obs_dim) == (B,cond_dim).
 *  - Every function returns 0 on success or a negative spdm_status; the text of
 *    the last error is available from spdm_last_error().  Nothing throws across
 *    the ABI and nothing calls exit().
 *  - One handle = one device = one in-flight call (not re-entrant per handle;
 *    distinct handles are independent).
 */
#ifndef SPDM_H
#define SPDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPDM_NAME_MAX 64
#define SPDM_ABI_VERSION 2

typedef enum {
    SPDM_OK = 0,
    SPDM_ERR_INVALID = -1,      /* bad argument / shape */
    SPDM_ERR_HIP = -2,          /* a HIP runtime call failed */
    SPDM_ERR_STATE = -3,        /* call order (weights/schedule not set, ...) */
    SPDM_ERR_MISSING = -4,      /* tensor name not found in the index */
    SPDM_ERR_NOMEM = -5
} spdm_status;

typedef enum { SPDM_DDPM = 0, SPDM_DDIM = 1, SPDM_DPMPP_2M = 2 } spdm_scheduler_kind;

typedef struct spdm_handle spdm_handle;

/* Shape of one noise predictor instance.  Mirrors the constructor arguments at
 * models/diffusion_ddpm.py:76-82 (UNet_Film(in=1, out=1, noise_steps,
 * global_cond_dim=observation_dim*obs_horizon, time_dim=256)) plus the trajectory
 * geometry sample() uses (pred_horizon + inpaint_horizon rows of prediction_dim,
 * models/diffusion_ddpm.py:252). */
typedef struct {
    int32_t horizon;              /* H: rows of x_t (unpadded)                      */
    int32_t state_dim;            /* D: columns of x_t (unpadded), 1..8             */
    int32_t cond_dim;             /* obs_horizon * observation_dim (flattened y)    */
    int32_t time_dim;             /* sinusoidal embedding width (256)               */
    int32_t attention;            /* 1: UNet_Film, 0: UNet_Film_noAttention         */
    int32_t max_batch;            /* workspace is sized for this many trajectories  */
    int32_t device;               /* HIP device ordinal                             */
    int32_t num_train_timesteps;  /* rows of the time-embedding table (t < this)    */
    int32_t flags;                /* SPDM_FLAG_*                                    */
} spdm_config;

#define SPDM_FLAG_DEBUG_KEEP 1    /* keep every intermediate alive for spdm_debug_tensor */
#define SPDM_FLAG_EXACT_FP32 2    /* contractions on the exact fp32 MFMA path instead of the default split-fp16
                                    path (hi + 2^-11 lo, 3 fp16 MFMAs, fp32 accumulate); env SPDM_PREC=f32 does the same */
#define SPDM_FLAG_SIMPLE_UNET 4   /* the noise predictor is UNet of models/simple_Unet.py (Diffusion_DDPM's default
                                    model='UNet', models/diffusion_ddpm.py:53-62) instead of UNet_Film[_noAttention]:
                                     - attention must be 0 (spdm_create returns SPDM_ERR_INVALID otherwise);
                                     - conditioning is required: cond_dim >= 1 at create, and spdm_unet_forward /
                                       spdm_sample* with d_cond == NULL return SPDM_ERR_INVALID (the reference's
                                       channel counts only match with y given);
                                     - spdm_load_weights takes UNet.state_dict() names ("input_conv.first.weight",
                                       "down1.cond_emb_layer.1.weight", ...) including the buffer
                                       "pos_encoding.pos_encoding", which must be (num_train_timesteps, time_dim):
                                       it IS the time table (spdm_set_time_table may still overwrite it), so timesteps
                                       are valid below its row count (noise_steps + 1 in the reference);
                                     - evaluation semantics (model.eval()): the positional encoding's dropout is off;
                                     - spdm_debug_tensor names: x1 x2 x3 x4 u1 u2 u3 (block outputs, in the plan's
                                       channel-padded storage: real channels first, zeros after);
                                     - every other entry point (schedules, sampling, graphs, switches, profiler,
                                       pinned geometry, precision flags) behaves as for UNet_Film. */

#define SPDM_FLAG_TRAIN 8         /* the handle also serves spdm_train_loss_grad: it keeps flipped / transposed weight copies for
                                    the backward pass and a training workspace sized at max_batch.  UNet_Film_noAttention, or
                                    UNet_Film (attention = 1) together with SPDM_FLAG_TRAIN_ATTENTION, or simple_Unet.py's UNet
                                    (SPDM_FLAG_SIMPLE_UNET) together with SPDM_FLAG_TRAIN_SIMPLE: spdm_create returns
                                    SPDM_ERR_INVALID with attention = 1 and no SPDM_FLAG_TRAIN_ATTENTION, and with
                                    SPDM_FLAG_SIMPLE_UNET and no SPDM_FLAG_TRAIN_SIMPLE.  Every other entry point behaves as on a
                                    handle without the flag. */

#define SPDM_FLAG_TRAIN_ATTENTION 16   /* with SPDM_FLAG_TRAIN and attention = 1: spdm_train_loss_grad covers UNet_Film's six
                                    SelfAttention blocks too (their weights' gradients are part of the blob).  Opt-in because its
                                    workspace is larger.  SPDM_ERR_INVALID without SPDM_FLAG_TRAIN, with attention = 0, with
                                    SPDM_FLAG_SIMPLE_UNET, and where a block's token count H_l x W_l exceeds 512 (horizon above
                                    64).  Every other entry point behaves as on a plain attention handle. */

#define SPDM_FLAG_TRAIN_SIMPLE 32  /* with SPDM_FLAG_TRAIN and SPDM_FLAG_SIMPLE_UNET: spdm_train_loss_grad serves simple_Unet.py's
                                    UNet (its gradient covers every parameter; the blob slot of the buffer
                                    "pos_encoding.pos_encoding" receives zeros; d_cond is required).  Training mode of the
                                    positional encoding's dropout through spdm_train_set_time_scale.  SPDM_ERR_INVALID without
                                    SPDM_FLAG_TRAIN, without SPDM_FLAG_SIMPLE_UNET and with SPDM_FLAG_TRAIN_ATTENTION.  Every other
                                    entry point behaves as on a plain SPDM_FLAG_SIMPLE_UNET handle. */

/* One entry per tensor of the reference state_dict (names exactly as
 * UNet_Film.state_dict() gives them, e.g. "down1.cond_encoder.2.weight"),
 * torch-native layouts (conv: (Cout,Cin,3,3); linear: (out,in)). */
typedef struct {
    char     name[SPDM_NAME_MAX];
    uint64_t offset;              /* in floats, into the blob */
    uint64_t numel;
    int32_t  ndim;
    int32_t  shape[4];
} spdm_tensor_index;

int  spdm_abi_version(void);
const char* spdm_last_error(void);

/* Replaces: Diffusion_DDPM.__init__'s construction of self.noise_estimator
 * (models/diffusion_ddpm.py:76-82).  Allocates weights + workspace on `device`. */
int  spdm_create(const spdm_config* cfg, spdm_handle** out);
void spdm_destroy(spdm_handle* h);

/* Replaces: load_state_dict of the `noise_estimator.*` tensors
 * (generate.py:25-27 -> Lightning load_from_checkpoint).  `h_blob` is a HOST
 * array; the library uploads it once and re-lays the weights out for its kernels on the device. */
int  spdm_load_weights(spdm_handle* h, const float* h_blob, size_t n_floats,
                       const spdm_tensor_index* h_index, int32_t n_index);

/* Put updated weights (an optimiser step) into a loaded handle, in place: no allocation, the same workspace.
 * `d_blob` is a DEVICE blob of n_floats floats laid out as the blob last given to spdm_load_weights -- the layout
 * spdm_train_loss_grad writes its gradient in, so `param -= lr * grad` works on it directly.  Any handle kind.
 * Enqueues the split format's range check on `stream` and synchronises once to read its verdicts (and outc's bias,
 * a host scalar of the handle); then enqueues the re-layout of every weight copy on `stream` and returns:
 * `d_blob` must stay unchanged until `stream` has passed those kernels.  The time-embedding tables are recomputed
 * on the next evaluation; an open sampling session ends (spdm_sample_run answers SPDM_ERR_STATE until the next
 * spdm_sample_begin); a captured step graph whose outc bias changed is captured again on its next run.
 * The `pos_encoding.pos_encoding` slot of a simple_Unet.py blob is not read: the time table stays as loaded.
 * SPDM_ERR_INVALID: null pointer, or n_floats differs from the loaded blob's.  SPDM_ERR_STATE: no weights loaded;
 * or the set of tensors outside the split format's range (spdm_demoted_tensors) would change -- the workspace plan
 * depends on it: nothing is written, the handle keeps its weights bit for bit, and spdm_last_error names the first
 * such tensor; load the blob into a new handle instead. */
int  spdm_update_weights(spdm_handle* h, const float* d_blob, size_t n_floats, void* stream);

/* Test hook: a 64-bit hash of the bytes of every device weight copy (in the order spdm_load_weights made them),
 * of outc's bias and of the set of tensors outside the split format's range.  Synchronises the device. */
int  spdm_debug_weight_digest(const spdm_handle* h, uint64_t* out);

/* Optional: overwrite the sinusoidal table pos_encoding(t) for t = 0..T-1
 * (models/Unet_FiLmLayer.py:266-274), (T, time_dim) fp32 on the host.  By
 * default the library computes it itself in fp32; the Python host passes
 * torch's own values so that the table is bit-identical to the reference's. */
int  spdm_set_time_table(spdm_handle* h, const float* h_table, int32_t T);

/* Replaces: DDPMScheduler(...)/DDIMScheduler(...) construction +
 * set_timesteps(n) (models/diffusion_ddpm.py:65-70,268; generate.py:28-35).
 * Linear betas in [beta_start, beta_end], epsilon prediction, no clipping,
 * fixed_small variance / eta = 0. */
int  spdm_set_schedule(spdm_handle* h, int32_t kind, int32_t num_train_timesteps,
                       int32_t num_inference_steps, float beta_start, float beta_end);

/* Same, from caller-computed tables (a caller-assigned scheduler object):
 * h_timesteps[n_steps] in loop order, h_coef[n_steps][6] =
 *   { sqrt(1-abar_t), sqrt(abar_t), k_x0, k_x, k_eps, k_noise } with
 *   x0   = (x - c0*eps) / c1
 *   prev = k_x0*x0 + k_x*x [+ k_noise*z]   (DDPM)
 *   prev = k_x0*x0 + k_eps*eps              (DDIM, eta = 0)
 * SPDM_DPMPP_2M (DPM-Solver++, data prediction, multistep, midpoint) is accepted here only -- spdm_set_schedule
 * and spdm_schedule_tables refuse it, their signature has no room for the solver's options -- with the row
 *   { sigma_s, alpha_s, k_x, k0f, k0, k1 }: columns 0 and 1 as above (s: the timestep the iteration denoises from), and
 *   x0   = (x - c0*eps) / c1
 *   prev = k_x*x + k0f*x0                    first order: the first iteration a session runs, and every row with k1 == 0
 *   prev = k_x*x + k0*x0 + k1*x0_prev        second order; x0_prev: the x0 of the iteration before
 * (spdm_solver_step below is that update).  The first installation of such a schedule allocates two (max_batch,H,D) buffers
 * and a device word in the handle; a handle that never sees one allocates nothing for it.
 * A sampling session always starts first order: spdm_sample_begin discards the history.  Within a session
 * spdm_sample_run(b, e) continues it when the last iteration the session completed was b - 1 -- so run(0, k); run(k, n) equals
 * run(0, n) bit for bit -- and starts first order at b otherwise.  A loop suffix run from a caller's iterate (spdm_sample_begin,
 * spdm_sample_run(i0, n)) therefore begins with a first-order step and is NOT the tail of the whole loop from that iterate, as
 * it is for SPDM_DDPM / SPDM_DDIM. */
int  spdm_set_schedule_tables(spdm_handle* h, int32_t kind, int32_t n_steps,
                              const int32_t* h_timesteps, const float* h_coef);

/* Pure host helper (no GPU needed): the tables spdm_set_schedule would build. */
int  spdm_schedule_tables(int32_t kind, int32_t num_train_timesteps, int32_t num_inference_steps,
                          float beta_start, float beta_end,
                          int32_t* h_timesteps_out, float* h_coef_out /* [n][6] */);

/* Replaces: self.noise_estimator(x_t, torch.tensor([t]), obs_cond)
 * (models/diffusion_ddpm.py:272 -> UNet_Film.forward, models/Unet_FiLmLayer.py:277-312).
 * d_x (B,H,D), h_t[t_count] with t_count == 1 (broadcast) or B, d_cond (B,cond_dim),
 * d_eps (B,H,D).  cond may be NULL (no FiLM, `y=None`), except under SPDM_FLAG_SIMPLE_UNET. */
int  spdm_unet_forward(spdm_handle* h, int32_t B, const float* d_x, const int32_t* h_t,
                       int32_t t_count, const float* d_cond, float* d_eps, void* stream);

/* spdm_unet_forward with the timesteps where a device-side forward process leaves them: d_t[t_count] is a DEVICE array.
 * Checks and results are spdm_unet_forward's, except that there is no host copy of t and no host range check: a
 * stream-ordered kernel copies d_t into the handle, clamped into [0, num_train_timesteps), exactly as spdm_train_loss_grad_dt
 * does, so an out-of-range value can never index a table.  For in-range timesteps d_eps equals spdm_unet_forward's bit for
 * bit.  The time-embedding tables are still rebuilt with a wait after a weight update. */
int  spdm_unet_forward_dt(spdm_handle* h, int32_t B, const float* d_x, const int32_t* d_t,
                          int32_t t_count, const float* d_cond, float* d_eps, void* stream);

/* Replaces: the body of Diffusion_DDPM.sample / Diffusion_DDIM.sample after the
 * conditioning vectors are built (models/diffusion_ddpm.py:252-277,
 * models/diffusion_ddim.py:52-74): for t in timesteps: eps = unet(x,t,cond);
 * x = scheduler.step(eps,t,x).prev_sample; x[:, :, :inp_h, :] = inpaint.
 *
 *  d_cond     (B,cond_dim)
 *  d_inpaint  (B,inp_h,D) if inpaint_per_sample else (inp_h,D) broadcast; NULL/inp_h=0: none
 *  d_xT       (B,H,D) initial sample (the reference draws it uniform, ddpm.py:252)
 *  d_noise    (n_steps,B,H,D) pre-drawn N(0,1) (row i used by loop iteration i when t>0),
 *             or NULL: device Philox4x32-10 stream keyed by (seed, sample_offset+b, i)
 *  d_out      (B,H,D) final x_0
 *  d_history  NULL or (n_steps+1,B,H,D): x_T followed by every iterate (option='sample_history')
 */
int  spdm_sample(spdm_handle* h, int32_t B, const float* d_cond,
                 const float* d_inpaint, int32_t inp_h, int32_t inpaint_per_sample,
                 const float* d_xT, const float* d_noise, uint64_t seed, uint64_t sample_offset,
                 float* d_out, float* d_history, void* stream);

/* Replaces: one training_step of Diffusion_DDPM up to loss.backward() (models/diffusion_ddpm.py:128-173,
 * process_single_batch): eps = unet(x_noisy, t, cond); loss = mean((noise - eps)^2); the gradients of the loss with respect to
 * every weight of the network and to cond.  Handle created with SPDM_FLAG_TRAIN (SPDM_ERR_STATE otherwise); a UNet_Film handle
 * (attention = 1) also needs SPDM_FLAG_TRAIN_ATTENTION, and then its gradient covers the sa1 .. sa6 tensors; a
 * SPDM_FLAG_SIMPLE_UNET handle needs SPDM_FLAG_TRAIN_SIMPLE and a non-NULL d_cond (SPDM_ERR_INVALID otherwise).
 *  d_x_noisy, d_noise (B,H,D); h_t[t_count], t_count == 1 (broadcast) or B; d_cond (B,cond_dim) or NULL (no FiLM);
 *  d_loss     one float on the device;
 *  d_eps      NULL or (B,H,D): the predicted noise;
 *  d_grad     device blob laid out as the blob last given to spdm_load_weights: the gradient of every tensor at that tensor's
 *             offset, torch layout (tensors the call does not reach -- the FiLM encoders when d_cond is NULL -- get zeros);
 *  d_grad_cond NULL or (B,cond_dim): the gradient with respect to cond (spdm_encoder_backward takes its image-feature columns when the vision encoder trains jointly).
 * Every contraction of the call runs on the exact fp32 MFMA path, whatever the handle's precision.
 * Deterministic: no float atomics; two calls with the same inputs give bit-identical results. */
int  spdm_train_loss_grad(spdm_handle* h, int32_t B, const float* d_x_noisy, const int32_t* h_t, int32_t t_count,
                          const float* d_cond, const float* d_noise, float* d_loss, float* d_eps, float* d_grad,
                          float* d_grad_cond, void* stream);

/* spdm_train_loss_grad with the timesteps where a device-side forward process leaves them: d_t[t_count] is a DEVICE array.
 * Checks, results and the consumption of a pending spdm_train_set_time_scale are spdm_train_loss_grad's, except that there is
 * no host range check: a stream-ordered kernel copies d_t into the handle, clamped into [0, num_train_timesteps), so an
 * out-of-range value can never index a table.  For in-range timesteps every output equals spdm_train_loss_grad's bit for
 * bit.  What the entry removes is the host copy of t and the host range check; the waits inside the pass itself remain
 * (the training pass waits for the upload of its row index, and the time-embedding tables are rebuilt with a wait after a
 * weight update), so the call is NOT free of host synchronisation.  A NULL stream synchronises on return, as everywhere. */
int  spdm_train_loss_grad_dt(spdm_handle* h, int32_t B, const float* d_x_noisy, const int32_t* d_t, int32_t t_count,
                             const float* d_cond, const float* d_noise, float* d_loss, float* d_eps, float* d_grad,
                             float* d_grad_cond, void* stream);

/* The forward (noising) process of a training step in ONE launch.  Replaces: the head of training_step
 * (models/diffusion_ddpm.py:128-173) -- t = torch.randint(0, noise_steps, (B,)); noise = torch.randn_like(x);
 * x_noisy = noise_scheduler.add_noise(x, noise, t); add_constraints(x_noisy, x_0_inpaint) (:216-219) -- and, optionally, the
 * Dropout(p) mask of simple_Unet.py's PositionalEncoding (:226-257) in the form spdm_train_set_time_scale takes.
 * Stateless: there is no handle.  Enqueued on `stream` (NULL: the null stream, and the call synchronises).
 *
 * Randomness: Philox4x32-10, key = (seed low word, seed high word), counter = (q, sample, step, purpose) with
 * sample = (uint32)(sample_offset + b) the GLOBAL sample index -- a shard of a batch draws what the whole batch would -- and
 * `step` the caller's training-step counter.  purpose 0 is spdm_sample's stream and is never drawn here (4-7: spdm_obs_noise, 8:
 * spdm_policy_warm_start).
 *   purpose 2, q = 0:            t_b = (int32)(((uint64)w0 * T) >> 32), in [0, T);
 *   purpose 1, q = e / 4:        the four words give the normals of elements 4q .. 4q+3 of the sample's (H, D) window (in-painted
 *                                rows included) by Box-Muller, (w0, w1) -> r cos, r sin and (w2, w3) likewise,
 *                                u = ((w >> 8) + 0.5) 2^-24;
 *   purpose 3, q = j / 4:        column j of the mask row uses word j & 3: d_time_scale[b][j] = u(w) >= dropout_p ? s : 0 with
 *                                s = (float)(1 / (1 - (double)dropout_p)).
 * Arithmetic: x_noisy = fl(fl(sa x0) + fl(sb z)), sa = d_sqrt_abar[t_b], sb = d_sqrt_1m_abar[t_b], three separately rounded
 * fp32 operations: torch's `sa * x0 + sb * noise` bit for bit.  Rows h < inp_h of x_noisy are then d_inpaint's; their d_noise
 * rows keep the noise (the reference's loss covers them).
 *   d_x0 (B,H,D): the clean window, cat([x_0_inpaint, x_0], dim=2);  d_inpaint (B,inp_h,D), NULL exactly when inp_h == 0;
 *   d_sqrt_abar, d_sqrt_1m_abar: T floats each, the caller's tables;
 *   d_t_in (B) / d_noise_in (B,H,D): NULL = drawn; non-NULL = the caller's values enter the arithmetic instead.  A given t
 *     outside [0, T) is clamped into range before any table is read;
 *   d_t (B, int32) / d_noise (B,H,D): the values used (a given t after the clamp).  Required when the value is drawn; may be
 *     NULL, or the input array itself, when it was given (the input is then left as it is);
 *   d_x_noisy (B,H,D);  d_time_scale NULL or (B,time_dim) with time_dim >= 1;
 *   d_clamped NULL or one int32: the number of entries of d_t_in outside [0, T) (0 when t is drawn).
 * Deterministic: no atomics; two calls with the same arguments give the same bits.
 * SPDM_ERR_INVALID, before the GPU is touched: a null required pointer; B, H, D or T < 1; inp_h outside [0, H]; d_inpaint
 * NULL with inp_h > 0 (or set with inp_h == 0); time_dim < 1 with d_time_scale set; dropout_p outside [0, 1) or NaN. */
typedef struct {
    int32_t B;
    int32_t H;
    int32_t D;
    int32_t inp_h;
    int32_t T;
    int32_t time_dim;
    const float* d_x0;
    const float* d_inpaint;
    const float* d_sqrt_abar;
    const float* d_sqrt_1m_abar;
    uint64_t seed;
    uint64_t sample_offset;
    uint32_t step;
    float dropout_p;
    const int32_t* d_t_in;
    const float* d_noise_in;
    int32_t* d_t;
    float* d_noise;
    float* d_x_noisy;
    float* d_time_scale;
    int32_t* d_clamped;
} spdm_forward_process_args;
int  spdm_train_forward_process(int32_t device, const spdm_forward_process_args* a, void* stream);

/* A training batch gathered from a dataset that lives on the device, in ONE launch.  Replaces:
 * CarRacingDataset.__getitem__ (utils/load_data.py:91-99) -- sample_sequence_sparse (utils/data_utils.py:58-62) and
 * _normalize_position (utils/load_data.py:85-89; the inference flavour's translation, :127-143) -- the np.moveaxis of
 * _load_data (:47), the DataLoader's collate (:173-177) and the .float() casts of models/diffusion_ddpm.py:287-290.
 * Stateless: there is no handle.  Enqueued on `stream` (NULL: the null stream, and the call synchronises).
 *
 * Batch slot b holds window w = clamp(d_window_id[b], 0, n_windows - 1); its rows are s + r step_size, r < seq_len, with
 * s = clamp(start of w, 0, T - 1 - (seq_len - 1) step_size).  The kernel uses no row number but these, so it cannot read
 * outside the stores whatever d_window_id and d_window_start hold.
 *   T: rows in every store;  n_windows: entries of the window table;  B: batch slots;  seq_len, step_size: rows per window and
 *     their spacing;  n_frames in [0, seq_len]: frames emitted per slot, the window's FIRST n_frames rows;
 *   img_dtype: 0 = d_img holds uint8 pixels, emitted as (float)k / 255.0f, one correctly rounded fp32 division (which equals
 *     (float)((double)k / 255.0) for every byte k);  1 = d_img holds float32, copied;  reserved: ignored (keeps the pointers
 *     8-byte aligned without implicit padding);
 *   d_img (T,96,96,3): frames as they are stored, channels interleaved;  16-byte aligned;  may be NULL when n_frames == 0;
 *   d_position (T,2) float64, RAW;  d_velocity (T,2), d_action (T,3) float32, already normalised;  each may be NULL when no
 *     output reads it;
 *   d_window_start (n_windows) int32 and h_window_start, the same table in HOST memory: both or neither.  The host copy is
 *     checked on every call, before the GPU is touched: each start in [0, T - 1 - (seq_len - 1) step_size].  Neither:
 *     window i starts at row i, and n_windows <= T - (seq_len - 1) step_size is required;
 *   d_window_id (B) int32, device;
 *   pos_min, pos_max: the scalar position statistics.  In float64, every operation rounded on its own (no FMA):
 *     sn = (x - pos_min) / (pos_max - pos_min) * 2 - 1;  translation = sn of the window's first row;
 *     position = (float)((sn - translation) / 2): numpy's float64 result rounded once to fp32;
 *   outputs, each may be NULL to skip it:  d_image_out (B,n_frames,3,96,96) fp32, planar, 16-byte aligned (NULL exactly
 *     when n_frames == 0);  d_position_out (B,seq_len,2), d_velocity_out (B,seq_len,2), d_action_out (B,seq_len,3) fp32;
 *     d_translation_out (B,2) float64;  d_start_out (B) int32: s;
 *     d_bad, one int32: SET (not added) to the number of slots whose id or table start had to be clamped.
 * Duplicate ids are legal: outputs are indexed by slot.  Deterministic: no atomics.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; T, n_windows, B, seq_len or step_size < 1; n_frames outside
 * [0, seq_len]; an unknown img_dtype; (seq_len - 1) step_size >= T; a NULL d_window_id; d_image_out set without n_frames
 * (or the reverse); a NULL store that a requested output reads; a misaligned d_img or d_image_out; one table pointer
 * without the other; a table start outside its range. */
typedef struct {
    int32_t T;
    int32_t n_windows;
    int32_t B;
    int32_t seq_len;
    int32_t step_size;
    int32_t n_frames;
    int32_t img_dtype;
    int32_t reserved;
    const void* d_img;
    const double* d_position;
    const float* d_velocity;
    const float* d_action;
    const int32_t* d_window_start;
    const int32_t* h_window_start;
    const int32_t* d_window_id;
    double pos_min;
    double pos_max;
    float* d_image_out;
    float* d_position_out;
    float* d_velocity_out;
    float* d_action_out;
    double* d_translation_out;
    int32_t* d_start_out;
    int32_t* d_bad;
} spdm_dataset_gather_args;
int  spdm_dataset_gather(int32_t device, const spdm_dataset_gather_args* a, void* stream);

/* The inverse of the gather's frame path in ONE launch (dataset.hip): planar fp32 frames become interleaved
 * uint8 pixels, written as 96 x 96 tiles of a contact sheet.  Replaces the per-frame recon.permute(1, 2, 0).cpu().numpy()
 * and imshow's own conversion of the reference's models/encoder/eval_autoencoder.py:91-106.  Stateless.  Enqueued on `stream`,
 * no atomics, no host synchronisation (NULL stream: the null stream, and the call synchronises).
 *   n: frames;  d_frames (n,3,96,96) fp32, planar, 16-byte aligned;
 *   d_out: uint8 of shape (ceil(n_tiles / cols) 96, cols 96, 3), 16-byte aligned;  cols: tiles per sheet row.
 * Frame i goes to tile j = tile_offset + i, at tile row j / cols and tile column j % cols: pixel (y, x, c) of the frame lands
 * at out[(j / cols) 96 + y][(j % cols) 96 + x][c].  Tiles outside [tile_offset, tile_offset + n) are not touched.  With
 * cols = 1 and tile_offset = 0 the output is the image store's own (n,96,96,3) layout.
 * Quantisation, in fp32: v = x * 255.0f (one fp32 multiply);  q = rintf(v) (ties to even);  the byte is 0 if v is NaN, else
 * min(max(q, 0), 255).  For a byte k, (float)k / 255.0f -- what spdm_dataset_gather emits -- gives v == k exactly, so gather
 * followed by this call returns the stored bytes.  The float64 form of the same recipe rounds some values differently: the
 * fp32 form is the contract.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args or a NULL or misaligned d_frames or d_out; n, cols or n_tiles < 1;
 * tile_offset < 0; tile_offset + n > n_tiles. */
typedef struct {
    int32_t n;
    int32_t cols;
    int64_t tile_offset;
    int64_t n_tiles;
    const float* d_frames;
    uint8_t* d_out;
} spdm_frames_to_bytes_args;
int  spdm_frames_to_bytes(int32_t device, const spdm_frames_to_bytes_args* a, void* stream);

/* The error of sampled trajectories against the windows they were conditioned on, in ONE launch and without the
 * trajectories leaving the device.  Replaces the per-window body of the reference's
 * evaluation/eval_acurracy_diffusion_positions.py:118-140 and evaluation/eval_consistency_diffusion_positions.py:
 * unnormalize_position (utils/data_utils.py:35-40) of truth and prediction, and
 * np.linalg.norm(gt[0, obs_horizon:] - pred[inpaint_horizon:], axis=1).  Stateless.  Enqueued on `stream` (NULL: the null
 * stream, and the call synchronises); it does not synchronise otherwise and uses no atomics.
 *
 * Trajectory g = window k x runs + run r: the runs of a window are consecutive trajectories.  Prediction row b of this call is
 * trajectory first_traj + b and reads the truth of slot (first_traj + b) / runs - window_base, so a call may begin and end
 * inside a window's runs and the truth is never replicated.
 *   B: prediction rows;  H, D: the sampler's horizon and state dimension;  n_slots: truth windows passed;  seq: rows per
 *     truth window;  obs_h: truth rows before the first predicted step;  inp_h: prediction rows before it;  P: predicted
 *     steps compared;  runs >= 1;  window_base: the window number of slot 0;  first_traj >= 0;
 *   d_pred (B,H,D) fp32: x_0;  d_truth_pos (n_slots,seq,2), d_truth_act (n_slots,seq,3) fp32, normalised as
 *     spdm_dataset_gather emits them;  d_translation (n_slots,2) float64;
 *   pos_min, pos_max: the scalar position statistics;  act_min, act_max: the action statistics per channel.
 * d_pos_err (B,P) float64: for step j,  || U(truth[slot, obs_h + j]) - U(pred[b, inp_h + j, 0:2]) ||_2  with
 *     U(n) = (((double)n * 2 + translation) + 1) / 2 * (pos_max - pos_min) + pos_min  and the norm sqrt(dx dx + dy dy);
 *     every operation is a float64 operation rounded on its own (no FMA), which is numpy's result bit for bit.
 * d_act_err (B,P,3) float64, optional (NULL skips it; then d_truth_act may be NULL):  | A(truth) - A(pred[b, inp_h + j, 2:5]) |
 *     per channel with  A(n) = (double)((n + 1.0f) / 2.0f) * (act_max - act_min) + act_min:  the reference's unnormalize_data
 *     on a float32 array, whose first two operations stay float32.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args or a NULL d_pred, d_truth_pos, d_translation or d_pos_err; d_act_err
 * without d_truth_act; B, P, runs, n_slots or seq < 1; H != inp_h + P; D < 2, or D < 5 with d_act_err; seq < obs_h + P;
 * obs_h or inp_h < 0; inp_h > obs_h; first_traj < 0; a slot of row 0 or of row B - 1 outside [0, n_slots); B x P beyond 31
 * bits. */
typedef struct {
    int32_t B;
    int32_t H;
    int32_t D;
    int32_t n_slots;
    int32_t seq;
    int32_t obs_h;
    int32_t inp_h;
    int32_t P;
    int32_t runs;
    int32_t window_base;
    int64_t first_traj;
    const float* d_pred;
    const float* d_truth_pos;
    const float* d_truth_act;
    const double* d_translation;
    double pos_min;
    double pos_max;
    double act_min[3];
    double act_max[3];
    double* d_pos_err;
    double* d_act_err;
} spdm_eval_errors_args;
int  spdm_eval_errors(int32_t device, const spdm_eval_errors_args* a, void* stream);

/* Mean and population standard deviation of an error buffer d_err (N,C) float64, N = windows x runs rows in trajectory order
 * (np.mean / np.std of the reference's evaluation scripts).  Five launches on `stream`, no atomics, no host synchronisation
 * between them (NULL stream: the call synchronises at its end).  Every sum is two-pass: the mean first, then the squared
 * deviations from it.
 *   d_window_mean, d_window_std (N / runs, C): over the runs of each window, summed sequentially in run order -- bit for bit
 *     np.mean / np.std(axis=0) of the window's (runs, C) rows, which numpy reduces row by row;
 *   d_mean, d_std (C): over all N rows, in a fixed order that is a function of (N, C) alone (blocks of 1024 rows reduced
 *     in-thread, by wave shuffles and through LDS; the block partials added in block order), so two calls on the same
 *     input give the same bits;
 *   d_workspace: at least spdm_eval_reduce_workspace_doubles(N, C) doubles, its capacity in workspace_doubles.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args or any NULL pointer; N, C or runs < 1; N not a multiple of runs;
 * C > 65535; a workspace that is too small. */
typedef struct {
    int64_t N;
    int32_t C;
    int32_t runs;
    const double* d_err;
    double* d_window_mean;
    double* d_window_std;
    double* d_mean;
    double* d_std;
    double* d_workspace;
    uint64_t workspace_doubles;
} spdm_eval_reduce_args;
int  spdm_eval_reduce(int32_t device, const spdm_eval_reduce_args* a, void* stream);
/* doubles of workspace spdm_eval_reduce needs for (N, C); 0 for N or C < 1 */
size_t spdm_eval_reduce_workspace_doubles(int64_t N, int32_t C);

/* Uniform noise added to the observations of a batch of windows in ONE launch (obs_noise.hip).  Replaces the
 * four `batch[k] = batch[k] + torch.rand_like(batch[k]) * scaling_factor` of evaluation/eval_robustness.py:180-190.
 * Stateless: there is no handle.  Enqueued on `stream`, no atomics, no host synchronisation (NULL stream: the null stream,
 * and the call synchronises).
 *
 * For each tensor i < n_tensors, each row < n_rows and each element e < inner:
 *     d_dst[row dst_stride + e] = d_src[row src_stride + e] + alpha u(row_offset + row, e)
 * in float32 with two roundings, the product and then the sum (no FMA).  Elements at or beyond inner are neither read nor
 * written, so a tensor can be cut to its first rows on the fly (position: inner = obs_h 2, src_stride = seq 2,
 * dst_stride = obs_h 2).  d_dst == d_src is allowed; any other overlap of the two is not.
 *   u: Philox4x32-10, key (seed lo, seed hi), counter (e / 4, row_offset + row, draw, 4 + i); element e takes word w = e % 4
 *     of its quad and u = (float)(w >> 8) 2^-24, exact and in [0, 1): the values torch.rand produces.  Purposes 0 .. 3 belong
 *     to the sampler and to spdm_train_forward_process, 8 to spdm_policy_warm_start.  The value of an element depends on (seed, draw, i, row_offset + row,
 *     e) alone: not on alignment, strides, n_rows or the other tensors, so rows [r0, r1) with row_offset + r0 equal the rows
 *     of the whole.
 *   Where d_src, d_dst are 16-byte aligned and inner and both strides are multiples of 4 the tensor moves in 16-byte
 *     accesses; otherwise element by element.  The values are the same.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; n_rows < 1; n_tensors outside [1, 4]; an inner < 0; a stride below
 * its inner; inner / 4 + 1 beyond 32 bits; row_offset < 0 or row_offset + n_rows beyond 32 bits; a NULL d_src or d_dst where
 * inner > 0; alpha negative or not finite; a grid beyond 2^31 - 1 workgroups (1024 quads each). */
typedef struct {
    const float* d_src;
    float* d_dst;
    int64_t inner;
    int64_t src_stride;
    int64_t dst_stride;
} spdm_obs_noise_tensor;
typedef struct {
    int64_t n_rows;
    int64_t row_offset;
    uint64_t seed;
    uint32_t draw;
    float alpha;
    int32_t n_tensors;
    int32_t reserved;
    spdm_obs_noise_tensor tensors[4];
} spdm_obs_noise_args;
int  spdm_obs_noise(int32_t device, const spdm_obs_noise_args* a, void* stream);

/* The closed-loop caller's host side for E environments in lockstep (policy.hip): the observation history as
 * rings in device memory, the conditioning batch built from them, and the plan back in the dataset's units.  Replaces the four
 * deque(maxlen = obs_horizon step_size) of run_predictions.py:112-124 and :145-148, prepare_diffusion_batch (:30-60) and the
 * .cpu() + unnormalize_position of :158-164.  The three entry points are stateless: the rings are the caller's device memory
 * and the push count n is the caller's.  Each is ONE launch enqueued on `stream` (NULL: the null stream, and the call
 * synchronises), with no atomics and no host synchronisation otherwise.  L slots per environment; the reference has
 * L = obs_horizon step_size.
 *
 * spdm_policy_push writes push number n (0-based) of all E environments into slot n mod L.
 *   img_dtype: 0 = frames are uint8, 1 = float32, in d_img_in and in d_ring_img alike;  reserved: ignored;
 *   d_img_in (E,96,96,3), d_pos_in (E,2), d_vel_in (E,2), d_act_in (E,3) float32: one observation per environment, RAW;
 *   d_ring_img (E,L,96,96,3), d_ring_pos (E,L,2), d_ring_vel (E,L,2), d_ring_act (E,L,3): the rings, RAW copies;
 *   d_fill (E) int32, read only: where it is non-zero the observation goes into ALL L slots of that environment -- the initial
 *     fill of run_predictions.py:120-124, and what a reset means.  The caller clears it after the push.
 *   A frame moves in 16-byte pieces on both sides, 1728 (uint8) or 6912 (float32) of them; d_img_in and d_ring_img must be
 *   16-byte aligned (every frame then is: a frame is a whole number of pieces).
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; E or L < 1; E x L beyond 31 bits; n < 0; an unknown img_dtype; any
 * NULL pointer; a misaligned d_img_in or d_ring_img. */
typedef struct {
    int32_t E;
    int32_t L;
    int32_t img_dtype;
    int32_t reserved;
    int64_t n;
    const void* d_img_in;
    const float* d_pos_in;
    const float* d_vel_in;
    const float* d_act_in;
    const int32_t* d_fill;
    void* d_ring_img;
    float* d_ring_pos;
    float* d_ring_vel;
    float* d_ring_act;
} spdm_policy_push_args;
int  spdm_policy_push(int32_t device, const spdm_policy_push_args* a, void* stream);

/* spdm_policy_window builds the batch of list(deque)[::step_size] after n pushes (n >= 1): entry k < obs_h of environment e
 * is slot (n + k step_size) mod L.  Entry 0 is the oldest one, the slot the next push overwrites; with L = obs_h step_size
 * the entries are the deque's elements 0, step_size, 2 step_size, ...  L >= (obs_h - 1) step_size + 1 is required, so that the
 * entries are distinct slots.
 *   stats_f32: bit 0 set = the velocity statistics are float32 arrays, bit 1 set = the action statistics are;
 *   pos_min, pos_max: the scalar position statistics;  vel_min, vel_max, act_min, act_max: per channel (float32 statistics
 *     widened to double, which is exact).
 * Outputs, float32, each may be NULL to skip it:
 *   d_image_out (E,obs_h,3,96,96), planar, 16-byte aligned: (float)k / 255.0f, one correctly rounded division, for uint8; a
 *     copy for float32;
 *   d_position_out (E,obs_h,2), d_translation_out (E,2): in float32, every operation rounded on its own (no FMA), as
 *     normalize_position (utils/data_utils.py:28-33) computes on a CPU float32 tensor with scalar float64 statistics:
 *       sn = ((x - (float)pos_min) / (float)(pos_max - pos_min)) * 2.0f - 1.0f, the range formed in float64 and rounded once;
 *       translation = sn of entry 0;  position = (sn - translation) / 2.0f;
 *   d_velocity_out (E,obs_h,2), d_action_out (E,obs_h,3): normalize_data (utils/data_utils.py:18-21) per channel.  torch
 *     promotes by the dtype of the statistics ARRAYS:
 *       float64 statistics: (float)((((double)x - min) / (max - min)) * 2.0 - 1.0), float64 operations rounded on their own,
 *         the result rounded once to float32 (the model's .float());
 *       float32 statistics: ((x - min) / (max - min)) * 2.0f - 1.0f in float32, every operation rounded on its own.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; E, L, obs_h or step_size < 1; (obs_h - 1) step_size >= L; E x L or
 * E x obs_h x 3 beyond 31 bits; n < 1; an unknown img_dtype; stats_f32 outside [0, 3]; no output at all; a NULL ring that a
 * requested output reads; a misaligned d_ring_img or d_image_out. */
typedef struct {
    int32_t E;
    int32_t L;
    int32_t obs_h;
    int32_t step_size;
    int32_t img_dtype;
    int32_t stats_f32;
    int64_t n;
    const void* d_ring_img;
    const float* d_ring_pos;
    const float* d_ring_vel;
    const float* d_ring_act;
    double pos_min;
    double pos_max;
    double vel_min[2];
    double vel_max[2];
    double act_min[3];
    double act_max[3];
    float* d_image_out;
    float* d_position_out;
    float* d_velocity_out;
    float* d_action_out;
    float* d_translation_out;
} spdm_policy_window_args;
int  spdm_policy_window(int32_t device, const spdm_policy_window_args* a, void* stream);

/* spdm_policy_unnormalize turns the sampler's x_0 into way-points and actions in the dataset's units.
 *   d_x0 (E,H,D) float32;  d_translation (E,2) float32, as spdm_policy_window emits it;  inp_h: rows of x_0 before the first
 *     predicted step;  P = H - inp_h;
 *   d_waypoints (E,P,2) float64: U(x0[e, inp_h + j, 0:2]) with the U of spdm_eval_errors and (double)translation;
 *   d_actions (E,P,3) float64, optional (NULL skips it): A(x0[e, inp_h + j, 2:5]) with the A of spdm_eval_errors.
 * The two entry points share the device functions (csrc/unnormalize.h).
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args or a NULL d_x0, d_translation or d_waypoints; E < 1; inp_h < 0;
 * H <= inp_h; D < 2, or D < 5 with d_actions; E x P beyond 31 bits. */
typedef struct {
    int32_t E;
    int32_t H;
    int32_t D;
    int32_t inp_h;
    const float* d_x0;
    const float* d_translation;
    double pos_min;
    double pos_max;
    double act_min[3];
    double act_max[3];
    double* d_waypoints;
    double* d_actions;
} spdm_policy_unnormalize_args;
int  spdm_policy_unnormalize(int32_t device, const spdm_policy_unnormalize_args* a, void* stream);

/* spdm_policy_warm_start builds the starting iterate of a warm-started plan: the previous plan, shifted by the
 * time that has passed, re-centred on the new window and noised to an intermediate level of the schedule -- the forward process
 * of training (spdm_train_forward_process) applied to a guess instead of data.  spdm_sample_begin with this iterate as d_xT
 * and spdm_sample_run(h, i0, n_steps) then run only the last n_steps - i0 denoise steps.  Stateless, ONE launch on `stream`
 * (NULL: the null stream, and the call synchronises), no atomics, no host synchronisation otherwise.
 *   E, H, D, inp_h: environments, rows and columns of a plan, in-painted rows (0 <= inp_h <= H); D >= 2, columns 0 and 1 are
 *     the position;  step_size >= 1: pushes between two rows of a plan;
 *   delta >= 0: pushes (environment steps) between the previous plan and this one;
 *   sa, sb: sqrt(abar_t) and sqrt(1 - abar_t) of the timestep t the first executed loop iteration i0 denoises from: row i0,
 *     columns 1 and 0, of the [n][6] coefficient table of spdm_set_schedule_tables;
 *   seed, env_offset, draw: the noise stream (below); env_offset is the GLOBAL index of environment 0, so that a shard of the
 *     environments draws what the whole would; draw is the caller's plan counter;
 *   d_prev_x0 (E,H,D) float32: the previous plan as the sampler returned it;
 *   d_prev_translation, d_translation (E,2) float32: the translations of the previous and of the new window, as
 *     spdm_policy_window emits them;
 *   d_inpaint (E,inp_h,D) float32, NULL exactly when inp_h == 0;
 *   d_noise_in (E,H,D) float32: NULL = the noise is drawn; non-NULL = the caller's values enter the arithmetic instead
 *     (spdm_train_forward_process's convention);
 *   d_x (E,H,D) float32, required: the starting iterate;  d_guess (E,H,D), optional: the shifted, re-centred plan before
 *     noising;  d_noise (E,H,D), optional: the noise used (may be d_noise_in itself, which is then left as it is).  No output
 *     may overlap d_prev_x0.
 * Time alignment (run_predictions.plan_rows): a plan made after n pushes has its row r at push index n + (r - inp_h) step_size
 * -- row inp_h - 1 is the newest window entry, way-point j lies 1 + j step_size pushes after the latest observation -- so a plan
 * made delta pushes later wants, at its row r, the old plan at row r + delta / step_size.
 * Per element (e, r, c), every float32 operation rounded on its own (no FMA); q = delta / step_size, f = delta % step_size in
 * integers:
 *   1. r0 = min(r + q, H - 1), r1 = min(r + q + (f > 0), H - 1);  a = prev[e, r0, c], b = prev[e, r1, c]: past the end of the
 *      old plan its last row is held;
 *   2. f == 0: g = a, no arithmetic.  Otherwise w = (float)f / (float)step_size, one correctly rounded division, and
 *      g = a + w (b - a): subtract, multiply, add, three roundings (also where r0 == r1);
 *   3. c < 2 only: g <- (((2.0f g) + T0[e,c]) - T1[e,c]) / 2.0f with T0 = d_prev_translation, T1 = d_translation --
 *      normalize_position centres a window on its own first entry, so the two plans live in different frames.  The scalings by
 *      2 are exact, the sum and the difference round;
 *   4. z = d_noise_in[e,r,c] if given; otherwise Philox4x32-10 with key (seed low word, seed high word) and counter
 *      (k, (uint32)(env_offset + e), draw, 8), k = (r D + c) / 4: the four words give the normals of elements 4k .. 4k+3 of the
 *      environment's (H, D) window by Box-Muller exactly as purpose 1 of spdm_train_forward_process does.  Purposes: 0 the
 *      sampler, 1-3 spdm_train_forward_process, 4-7 spdm_obs_noise, 8 this entry;
 *   5. x = (sa g) + (sb z): three roundings, torch's add_noise;
 *   6. rows r < inp_h of d_x are d_inpaint's, exactly (add_constraints); d_guess and d_noise are not in-painted.
 * Deterministic: two calls with the same arguments give the same bits.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; a NULL d_prev_x0, d_prev_translation, d_translation or d_x; E, H or
 * step_size < 1; D < 2; inp_h outside [0, H]; d_inpaint NULL with inp_h > 0 (or set with inp_h == 0); delta < 0; E x H x D
 * beyond 31 bits; sa or sb not finite. */
typedef struct {
    int32_t E;
    int32_t H;
    int32_t D;
    int32_t inp_h;
    int32_t step_size;
    uint32_t draw;
    int64_t delta;
    uint64_t seed;
    uint64_t env_offset;
    float sa;
    float sb;
    const float* d_prev_x0;
    const float* d_prev_translation;
    const float* d_translation;
    const float* d_inpaint;
    const float* d_noise_in;
    float* d_x;
    float* d_guess;
    float* d_noise;
} spdm_policy_warm_start_args;
int  spdm_policy_warm_start(int32_t device, const spdm_policy_warm_start_args* a, void* stream);

/* spdm_policy_select keeps one of K candidate plans per environment: the one closest to the plan being executed
 * (COHERENT) or the medoid of the set (MEDOID), and reports the candidates' spread as an uncertainty signal.  Stateless, ONE
 * launch on `stream` (NULL: the null stream, and the call synchronises), one workgroup per environment, no atomics, no host
 * synchronisation otherwise, no randomness.
 *   E environments;  K candidates each, 1 <= K <= 64;  H, D: rows and columns of a plan, D >= 2, columns 0 and 1 are the
 *     position;  inp_h: in-painted rows, 0 <= inp_h < H;  P = H - inp_h;
 *   cols, 2 <= cols <= D: the columns of a row that enter a distance (2: positions only; D: positions and actions);
 *   mode: SPDM_SELECT_MEDOID or SPDM_SELECT_COHERENT;
 *   d_x0 (E K,H,D) float32: the candidates as the sampler returned them; candidate k of environment e is row e K + k;
 *   d_guess float32, COHERENT only (NULL otherwise): the previous plan shifted and re-centred into the new window's frame, the
 *     d_guess of spdm_policy_warm_start.  Row e guess_row_stride (of H D elements) belongs to environment e:
 *     guess_row_stride = 1 for an (E,H,D) guess, K for the (E K,H,D) guess of a warm start made over K-fold repeated inputs;
 *   rows, COHERENT only (0 otherwise), 1 <= rows <= P: the predicted rows, from row inp_h, that the previous plan still informs
 *     (P - delta / step_size - (delta % step_size > 0) for a plan made delta pushes ago);
 *   d_translation (E,2) float32, pos_min, pos_max: read for d_spread only;
 *   d_chosen (E) int32, required;  d_x0_out (E,H,D) float32, required: row e is candidate chosen[e], copied exactly; it must
 *     not overlap d_x0;  d_scores (E,K) float64, optional;  d_spread (E,P) float64, optional.
 * Arithmetic: float64, every operation rounded on its own (no FMA), every sum serial in the order stated, so the result does not
 * depend on how the work is spread over threads.  x_k is candidate k of the environment, g its guess row.
 *   MEDOID distance: d(j,k) = sum over r = inp_h .. H-1 (outer, ascending) and c = 0 .. cols-1 (inner, ascending) of
 *     ((double)x_j[r,c] - (double)x_k[r,c])^2, from 0.0: per term one subtraction, one multiplication, one addition into the
 *     running sum.  d(j,k) and d(k,j) are the same bits;
 *   MEDOID score: s_j = sum over k = 0 .. K-1, ascending, of d(j,k), from 0.0; d(j,j) is included;
 *   COHERENT score: s_j = sum over r = inp_h .. inp_h+rows-1 and c < cols of ((double)x_j[r,c] - (double)g[r,c])^2, same order;
 *   choice: chosen[e] = the smallest j whose s_j is minimal.  A NaN score never wins against a non-NaN one; if every score is
 *     NaN the choice is 0;
 *   spread[e,p], r = inp_h + p: u_k = U(x_k[r,0]), v_k = U(x_k[r,1]) with the U of spdm_eval_errors and (double)translation[e];
 *     mu = (sum_k u_k) / (double)K, mv = (sum_k v_k) / (double)K, k ascending from 0.0;
 *     spread = sqrt((sum_k ((u_k - mu)^2 + (v_k - mv)^2)) / (double)K), k ascending from 0.0; inside a term: square u, square
 *     v, add.  sqrt is the correctly rounded one.  In words: the RMS distance, in the dataset's units, of the K candidates'
 *     way-point p from their mean.
 * Deterministic: two calls with the same arguments give the same bits.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; a NULL d_x0, d_chosen or d_x0_out; E < 1; K outside [1, 64];
 * inp_h < 0 or H <= inp_h; D < 2; cols outside [2, D]; an unknown mode; COHERENT with a NULL d_guess, rows outside [1, P] or
 * guess_row_stride < 1; MEDOID with a d_guess or rows != 0; d_spread without d_translation; E x K x H x D beyond 31 bits;
 * d_x0_out overlapping d_x0. */
enum { SPDM_SELECT_MEDOID = 0, SPDM_SELECT_COHERENT = 1 };
typedef struct {
    int32_t E;
    int32_t K;
    int32_t H;
    int32_t D;
    int32_t inp_h;
    int32_t cols;
    int32_t mode;
    int32_t rows;
    int64_t guess_row_stride;
    const float* d_x0;
    const float* d_guess;
    const float* d_translation;
    double pos_min;
    double pos_max;
    int32_t* d_chosen;
    float* d_x0_out;
    double* d_scores;
    double* d_spread;
} spdm_policy_select_args;
int  spdm_policy_select(int32_t device, const spdm_policy_select_args* a, void* stream);

/* spdm_solver_step is one DPM-Solver++ (2M) update (Lu et al. 2022, Algorithm 2: data prediction, multistep, midpoint) on the
 * caller's buffers: the launch the SPDM_DPMPP_2M sampling loop makes after each noise prediction.  Stateless,
 * ONE kernel launch on `stream` behind two stream-ordered 4-byte fills of d_words (NULL: the null stream, and the call
 * synchronises), one thread per element, no atomics, no host synchronisation otherwise.
 *   B, H, D: trajectories, rows, columns;  inp_h, inpaint_per_sample, d_inpaint: as spdm_sample ((B,inp_h,D) or (inp_h,D));
 *   n_steps: rows of d_coef;  step: the loop iteration, 0 <= step < n_steps;  first: the iteration that runs first order
 *     whatever its row says (the first one after a start: x0_prev holds nothing yet), or -1;
 *   d_eps (B,H,D): the predicted noise;  d_x (B,H,D): the iterate, updated in place;  d_x0_prev (B,H,D): read on a
 *     second-order step, always written with this step's x0 (before in-painting);
 *   d_coef [n_steps][6] DEVICE: rows { sigma_s, alpha_s, k_x, k0f, k0, k1 } (spdm_set_schedule_tables);
 *   d_history NULL or (n_steps+1,B,H,D): row step + 1 receives the new iterate;
 *   d_words DEVICE int32[3]: the entry writes {step, first}; word 2 is set to 1 when a new iterate is not finite and is
 *     otherwise left as it is (the caller clears it).
 * Per element, every float32 operation rounded on its own (no FMA), c = d_coef[step]:
 *   1. x0 = (x - c0 eps) / c1;   2. acc = c2 x;
 *   3. first order (step == first, or c5 == 0): acc = acc + c3 x0;  second order: acc = acc + c4 x0, then acc = acc + c5 x0_prev;
 *   4. x0_prev <- x0;  rows h < inp_h of the iterate are d_inpaint's, exactly;  x <- the result.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args; B, H, D or n_steps < 1; B x H x D beyond 31 bits; inp_h outside
 * [0, H]; d_inpaint NULL with inp_h > 0 (or set with inp_h == 0); inpaint_per_sample not 0 or 1; step outside [0, n_steps);
 * first outside [-1, n_steps); a NULL d_eps, d_x, d_x0_prev, d_coef or d_words. */
typedef struct {
    int32_t B;
    int32_t H;
    int32_t D;
    int32_t inp_h;
    int32_t inpaint_per_sample;
    int32_t n_steps;
    int32_t step;
    int32_t first;
    const float* d_eps;
    float* d_x;
    float* d_x0_prev;
    const float* d_coef;
    const float* d_inpaint;
    float* d_history;
    int32_t* d_words;
} spdm_solver_step_args;
int  spdm_solver_step(int32_t device, const spdm_solver_step_args* a, void* stream);

/* The per-sample terms of a validation pass's loss in ONE launch (train_metrics.hip).  Replaces: nn.MSELoss
 * of the reference's validation_step (models/diffusion_ddpm.py:175-214, :49) as Lightning averages it over an epoch, weighted by
 * batch size: with H x D elements in every sample that is the mean over the samples of each sample's own mean squared error.
 * Stateless: there is no handle.  Enqueued on `stream`, no atomics, no host synchronisation (NULL stream: the null stream, and
 * the call synchronises).
 *   d_eps, d_noise (B,H,D) fp32: the predicted and the drawn noise of one batch;
 *   d_terms (n_slots) float64: sample b writes d_terms[slot_offset + b] = (sum over its H x D elements e of
 *     ((double)noise[e] - (double)eps[e])^2) / (double)(H x D);  slots outside [slot_offset, slot_offset + B) are not touched;
 *   d_t_in (B) int32 with d_slot_t (n_slots) int32, both or neither: d_slot_t[slot_offset + b] = d_t_in[b].
 * Every operation is a float64 operation rounded on its own (no FMA).  The summation order is a function of H x D alone: element
 * e (row-major in the sample) belongs to partial e mod 64; a partial adds its elements in ascending order starting from 0.0; the
 * 64 partials p[0..63] are combined by  for off in 32, 16, 8, 4, 2, 1: p[i] = p[i] + p[i + off], i < off;  the term is
 * p[0] / (double)(H x D).  (One wave per sample, lane = partial, the tree by wave shuffles; several samples per workgroup.)
 * The mean over a pass is spdm_eval_reduce over the (N, 1) terms with runs = 1: its d_mean.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args or a NULL d_eps, d_noise or d_terms; B, H or D < 1; H x D beyond 31
 * bits; slot_offset < 0; slot_offset + B > n_slots; exactly one of d_t_in / d_slot_t set. */
typedef struct {
    int32_t B;
    int32_t H;
    int32_t D;
    int32_t reserved;
    const float* d_eps;
    const float* d_noise;
    int64_t slot_offset;
    int64_t n_slots;
    double* d_terms;
    const int32_t* d_t_in;
    int32_t* d_slot_t;
} spdm_loss_terms_args;
int  spdm_loss_terms(int32_t device, const spdm_loss_terms_args* a, void* stream);

/* The per-frame reconstruction error of one validation batch of the frame autoencoder in ONE launch (DESIGN.md 8.23,
 * train_metrics.hip).  Replaces: nn.MSELoss(recon, batch) of the reference's validation_step (models/encoder/autoencoder.py:48,
 * 64-71) as Lightning averages it over an epoch, weighted by batch size: every frame has 27648 elements, so that is the mean
 * over the frames of each frame's own mean squared error.  Stateless: there is no handle.  Enqueued on `stream`, no atomics,
 * no host synchronisation (NULL stream: the null stream, and the call synchronises).
 *   n: frames in the batch;  d_recon, d_target (n,3,96,96) fp32, planar, 16-byte aligned;
 *   d_terms (n_slots) float64: frame b writes d_terms[slot_offset + b];  slots outside [slot_offset, slot_offset + n) are not
 *     touched;  reserved: ignored (keeps the pointers 8-byte aligned without implicit padding).
 * Every operation is a float64 operation rounded on its own (no FMA).  The order is a function of the frame size alone,
 * 27648 elements = 6912 quads of four consecutive floats (row-major in the frame): quad q belongs to partial q mod 256; a
 * partial starts at 0.0 and takes its quads in ascending order and within a quad the four elements in ascending order, as
 * d = (double)target - (double)recon;  p = p + d * d;  the 256 partials p[0..255] are combined by
 * for off in 128, 64, 32, 16, 8, 4, 2, 1: p[i] = p[i] + p[i + off], i < off;  the term is p[0] / 27648.0.  (One 256-thread
 * workgroup per frame, thread = partial, 16-byte loads; the tree's first two steps through LDS, the rest by wave shuffles.)
 * The mean over a pass is spdm_eval_reduce over the (N, 1) terms with runs = 1: its d_mean.
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args or a NULL d_recon, d_target or d_terms; n < 1; slot_offset < 0;
 * slot_offset + n > n_slots; a misaligned d_recon or d_target. */
typedef struct {
    int32_t n;
    int32_t reserved;
    const float* d_recon;
    const float* d_target;
    int64_t slot_offset;
    int64_t n_slots;
    double* d_terms;
} spdm_recon_terms_args;
int  spdm_recon_terms(int32_t device, const spdm_recon_terms_args* a, void* stream);

/* PositionalEncoding's Dropout(p) in training mode (simple_Unet.py:226-257) for the NEXT spdm_train_loss_grad call on a
 * SPDM_FLAG_TRAIN_SIMPLE handle (SPDM_ERR_STATE on any other): d_scale is a (B, time_dim) device array -- the dropout mask
 * divided by (1 - p) -- and that call evaluates the network on pe[t_b] * d_scale[b].  The call consumes the setting, whatever
 * its outcome; it fails with SPDM_ERR_INVALID if its B differs.  d_scale == NULL clears the setting now.  The array is read by
 * that call, on its stream: it must stay valid until then. */
int  spdm_train_set_time_scale(spdm_handle* h, const float* d_scale, int32_t B);

/* The same loop in three pieces, so a caller (bench.py) can time an exact range
 * of denoise steps: begin() hoists the step-invariant FiLM projections and
 * loads x_T; run() executes loop iterations [step_begin, step_end); result()
 * copies the current iterate out. */
int  spdm_sample_begin(spdm_handle* h, int32_t B, const float* d_cond,
                       const float* d_inpaint, int32_t inp_h, int32_t inpaint_per_sample,
                       const float* d_xT, const float* d_noise, uint64_t seed,
                       uint64_t sample_offset, float* d_history, void* stream);
int  spdm_sample_run(spdm_handle* h, int32_t step_begin, int32_t step_end, void* stream);
int  spdm_sample_result(spdm_handle* h, float* d_out, void* stream);

/* How many times this handle has captured its denoise step into a hipGraph.  spdm_sample_run replays one captured step
 * for every iteration; the capture is keyed by the session's SHAPE (batch, inpaint horizon, scheduler, switches), not by
 * the addresses of the caller's buffers or the seed -- so the closed-loop caller (run_predictions.py:151-156: one
 * model.sample() per control period, fresh tensors every time) captures once and replays ever after. */
int64_t spdm_graph_captures(const spdm_handle* h);

/* Introspection for tests: copy a named intermediate of the LAST
 * spdm_unet_forward (handle created with SPDM_FLAG_DEBUG_KEEP) to d_out in
 * channels-last (B, H_l*W_l, C) order; shape_out = {B, H_l, W_l, C}.
 * Names: x1 d1 x2 d2 x3 d3 x4 x5 u1 a4 u2 a5 u3 a6. */
int  spdm_debug_tensor(spdm_handle* h, const char* name, float* d_out, size_t cap_floats,
                       int32_t shape_out[4]);

/* Range guard of the split-precision contractions.  The split-fp16 path represents |weight| < 511 and
 * |activation| < 4094.  Weights: spdm_load_weights checks every tensor and keeps a layer whose
 * tensor exceeds the bound on the exact fp32 kernels (spdm_demoted_tensors counts them; results stay within the
 * parity tolerance, that layer runs slower).  Activations: the step-update kernel raises a device flag when an
 * updated iterate (or, for spdm_unet_forward, an eps value) is not finite; spdm_nonfinite synchronises `stream`
 * and returns it (reset by spdm_sample_begin / spdm_unet_forward).  The reference's fp32 torch path
 * (models/diffusion_ddpm.py:261-263) has neither limit; a caller that hits the flag re-creates the handle with
 * SPDM_FLAG_EXACT_FP32. */
int32_t spdm_demoted_tensors(const spdm_handle* h);
int  spdm_nonfinite(spdm_handle* h, int32_t* flag_out, void* stream);

/* Flip one kernel-selection switch ("SPDM_NO_GRAPH", "SPDM_NO_WIDE", ... -- the names the environment is read for,
 * ONCE, at spdm_create) on a live handle.  Test / tuning hook: the product path never calls it.  The workspace is
 * re-planned for the new kernel selection (the unfused fallbacks need more scratch) and grown if it has to be. */
int  spdm_set_switch(spdm_handle* h, const char* name, int32_t on);

/* 1 if the handle's contractions run on the split-fp16 MFMA path, 0 on the exact fp32 MFMA path. */
int32_t spdm_uses_split_precision(const spdm_handle* h);

/* Workspace bytes currently reserved on the device (weights + arena). */
size_t spdm_device_bytes(const spdm_handle* h);

/* Device time of the dominant kernel class, measured with HIP events on the
 * launch stream: when enabled, every conv3x3 implicit-GEMM launch is bracketed
 * by events; spdm_profile_read returns launches, total ms and total FLOPs
 * since the last reset.  For bench.py's roofline leg only (adds sync points).
 * on = 1: instrument from now on (runs are plain launches, not graph replays);
 * on = 0: stop; on = 2: only create the events ahead of time (nothing is
 * instrumented, graph replay stays on) so that a later on = 1 costs nothing. */
int  spdm_profile_enable(spdm_handle* h, int32_t on);
int  spdm_profile_read(spdm_handle* h, int64_t* launches, double* total_ms, double* total_flops);

/* Micro-benchmark of ONE fused conv_chain.hip launch on synthetic data (tools/bench_chain.py; kernel tuning only, not on the
 * product path): B samples of HW rows through the n_layers 3-tap layers of widths chan[0 .. n_layers], the plan's GELU pattern.
 * debug: ablation bits (1: no MFMAs -- timing only, wrong results), honoured by diagnostic builds (SPDM_DIAG) only.
 * *ms_out: ms per launch. */
int  spdm_bench_chain(int32_t device, int32_t B, int32_t HW, int32_t n_layers, const int32_t* chan, int32_t iters,
                      int32_t debug, double* ms_out);

/* Micro-benchmark of ONE implicit-GEMM launch shape on synthetic data (tools/bench_gemm.py; kernel tuning
 * only, not on the product path): conv taps in {1,3,9} over (B, H*W, Cin) -> (B, H*W, Cout).  pro: 0 none,
 * 1 GroupNorm, 2 GroupNorm+GELU; epi: 0 GN stats, 1 bias, 2 bias+GELU, 3 bias+residual; debug: ablation bits. */
int  spdm_bench_gemm(int32_t device, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t taps,
                     int32_t pro, int32_t epi, int32_t split, int32_t iters, int32_t debug,
                     double* ms_out /* [3]: ms per launch; max |out - exact-fp32 out|; worst deviation of the per-sample
                                        GroupNorm mean (in sigmas) / variance (relative) the launch reported from the
                                        values recomputed from its own output (both: debug == 0, else -1) */);

/* Observation front end (widened scope).  Replaces: self.vision_encoder(img.flatten(end_dim=1))
 * in prepare_obs_cond_vectors (models/diffusion_ddpm.py:317-321), i.e. Autoencoder.encoder of
 * models/encoder/autoencoder.py:11-20: Conv2d(3,16,2,2,p1) ReLU Conv2d(16,32,2,2) ReLU Conv2d(32,64,2,2) ReLU Flatten
 * Linear(9216,128).  Weights: the encoder's own state_dict (names "0.weight" "0.bias" "2.*" "4.*" "7.*", torch layouts)
 * as a host blob + index, like spdm_load_weights.  d_images: (n,3,96,96) fp32 on the device; d_latent: (n,128). */
typedef struct spdm_encoder spdm_encoder;
int  spdm_encoder_create(int32_t device, const float* h_blob, size_t n_floats, const spdm_tensor_index* h_index,
                         int32_t n_index, spdm_encoder** out);
int  spdm_encoder_forward(spdm_encoder* e, int32_t n_images, const float* d_images, float* d_latent, void* stream);
void spdm_encoder_destroy(spdm_encoder* e);

/* Joint training of the encoder.  The reference optimises self.vision_encoder together with the U-Net:
 * configure_optimizers is Adam(self.parameters()) (models/diffusion_ddpm.py:115-116), the encoder is a registered submodule
 * (:84-88) and prepare_obs_cond_vectors (:317-330) runs it with autograd on.  Every contraction is exact fp32 and every
 * reduction runs in a fixed order without atomics: two calls on the same inputs give the same bits.  A handle that never
 * calls these allocates nothing for them.
 *
 * spdm_encoder_train_forward.  Replaces: self.vision_encoder(img.flatten(end_dim=1)) (:317-321) inside training_step
 * (:128-173).  The latents of spdm_encoder_forward, bit for bit; keeps per frame the conv-2 and conv-3 maps (73 KB + 37 KB)
 * for ONE following spdm_encoder_backward.  conv 1's map is not kept: the backward pass recomputes it from the frames.
 * The kept maps' ReLU masks are settled by a second, float64 evaluation of the three convolutions: a unit whose fp32
 * pre-activation rounded to the other side of zero would otherwise carry a whole unit's gradient the wrong way.
 *
 * spdm_encoder_backward.  Replaces: loss.backward() through models/encoder/autoencoder.py:11-20.  d_images are the frames
 * of the pending train_forward, d_grad_latent is d loss / d latent (n_images,128), d_grad a device blob of the n_floats
 * given to spdm_encoder_create: every tensor's gradient at that tensor's offset in torch layout, zeros between.  Frames go
 * through in chunks of 2048 whose gradients are added in chunk order.  There is no gradient with respect to the frames.
 * SPDM_ERR_STATE: no train_forward pending (none yet, already consumed by a backward, or followed by
 * spdm_encoder_update_weights), or n_images differs from it.  SPDM_ERR_INVALID: null pointer, n_images <= 0.
 *
 * spdm_encoder_update_weights.  Replaces: optimizer.step() on the encoder's parameters (:115-116); the encoder's
 * counterpart of spdm_update_weights.  d_blob is a DEVICE blob in the layout given to spdm_encoder_create; its values go
 * into the handle in place (and into the transposed copies a training handle keeps), enqueued on `stream`.  Afterwards
 * spdm_encoder_forward equals a new handle created on those values, bit for bit.  SPDM_ERR_INVALID: null pointer, or
 * n_floats differs from spdm_encoder_create's. */
int  spdm_encoder_train_forward(spdm_encoder* e, int32_t n_images, const float* d_images, float* d_latent, void* stream);
int  spdm_encoder_backward(spdm_encoder* e, int32_t n_images, const float* d_images, const float* d_grad_latent,
                           float* d_grad, void* stream);
int  spdm_encoder_update_weights(spdm_encoder* e, const float* d_blob, size_t n_floats, void* stream);

/* The autoencoder's decoder and its reconstruction training: the stage that produces the encoder
 * checkpoint Diffusion_DDPM loads (models/diffusion_ddpm.py:84-88), models/encoder/train_autoencoder.py on
 * models/encoder/autoencoder.py.  Autoencoder.decoder (:23-32) is Linear(128,9216) Unflatten(64,12,12)
 * ConvTranspose2d(64,32,2,2) ReLU ConvTranspose2d(32,16,2,2) ReLU ConvTranspose2d(16,3,2,2) Sigmoid; the loss is
 * MSELoss(recon, batch) (:48,55-58).  Every contraction is exact fp32 and every reduction runs in a fixed order without
 * atomics: two calls on the same inputs give the same bits.  A handle that never trains allocates nothing for training.
 * The saved maps' ReLU masks are settled by a second, float64 evaluation of the pre-activations, as the encoder's are.
 *
 * spdm_decoder_create.  Replaces: the construction of Autoencoder.decoder (:23-32) and load_state_dict on it.  Weights: the
 * decoder's own state_dict (names "0.weight" (9216,128) "0.bias" "2.weight" (64,32,2,2) "2.bias" "4.weight" (32,16,2,2)
 * "4.bias" "6.weight" (16,3,2,2) "6.bias", torch layouts) as a host blob + index, like spdm_encoder_create.
 * SPDM_ERR_INVALID: null pointer, or a name or shape that is not the decoder's.
 *
 * spdm_decoder_forward.  Replaces: self.decoder(encoded) of Autoencoder.forward (:34-37), as eval_autoencoder.py uses it.
 * d_latent (n,128) -> d_recon (n,3,96,96), fp32 on the device.
 *
 * spdm_decoder_train_loss.  Replaces: recon = self.model(batch) past the encoder and loss = self.loss(recon, batch) of
 * onepass (:55-58).  d_target (n,3,96,96); d_loss one float on the device = sum (recon - target)^2 / (n 27648), the squares
 * added in float64 in a fixed order; d_recon NULL or (n,3,96,96): the reconstruction, spdm_decoder_forward's bit for bit.
 * Keeps per frame the Linear's output, the two post-ReLU maps and the reconstruction (37 + 74 + 147 + 111 KB) for ONE
 * following spdm_decoder_backward.
 *
 * spdm_decoder_backward.  Replaces: loss.backward() through the decoder (training_step :61-65 under Lightning's automatic
 * optimisation).  d_latent and d_target are those of the pending train_loss.  d_grad: device blob of the n_floats given to
 * create, every tensor's gradient at that tensor's offset in torch layout, zeros between.  d_grad_latent (n,128):
 * d loss / d latent, what spdm_encoder_backward takes.  Frames go through in chunks of 2048 whose gradients are added in
 * chunk order.  SPDM_ERR_STATE: no train_loss pending (none yet, already consumed by a backward, or followed by
 * spdm_decoder_update_weights), or n differs from it.
 *
 * spdm_decoder_update_weights.  Replaces: optimizer.step() on the decoder's parameters (configure_optimizers :73-74).
 * d_blob is a DEVICE blob in the layout given to create; afterwards spdm_decoder_forward equals a new handle created on
 * those values, bit for bit.  A pending train_loss is dropped.
 *
 * All: SPDM_ERR_INVALID on a null pointer (d_recon of train_loss excepted), n <= 0, or an n_floats that differs from create's. */
typedef struct spdm_decoder spdm_decoder;
int  spdm_decoder_create(int32_t device, const float* h_blob, size_t n_floats, const spdm_tensor_index* h_index,
                         int32_t n_index, spdm_decoder** out);
int  spdm_decoder_forward(spdm_decoder* d, int32_t n, const float* d_latent, float* d_recon, void* stream);
int  spdm_decoder_train_loss(spdm_decoder* d, int32_t n, const float* d_latent, const float* d_target,
                             float* d_recon /* may be NULL */, float* d_loss, void* stream);
int  spdm_decoder_backward(spdm_decoder* d, int32_t n, const float* d_latent, const float* d_target, float* d_grad,
                           float* d_grad_latent, void* stream);
int  spdm_decoder_update_weights(spdm_decoder* d, const float* d_blob, size_t n_floats, void* stream);
void spdm_decoder_destroy(spdm_decoder* d);

/* The optimiser step on the device.  Replaces: configure_optimizers' torch.optim.Adam(self.parameters(),
 * lr) (models/diffusion_ddpm.py:114-124; models/encoder/autoencoder.py:73-74) as Lightning steps it, preceded by the
 * global-norm gradient clipping that train.py / train_autoencoder.py ask for with gradient_clip_val=0.5
 * (torch.nn.utils.clip_grad_norm_).  Stateless: there is no handle; the moments are the caller's arrays (torch.optim.Adam's
 * exp_avg / exp_avg_sq, so checkpoints interchange) and the step count is an argument.
 *
 * A segment is one flat fp32 device array of numel floats with its gradient and its two moments: the U-Net blob of
 * spdm_train_loss_grad, the encoder's of spdm_encoder_backward, the decoder's of spdm_decoder_backward.  All four pointers
 * must be 16-byte aligned.
 *
 * spdm_adam_workspace_doubles.  Pure host call: the doubles the caller provides as d_workspace (16-byte aligned, contents
 * need not be initialised): one partial sum of g^2 per workgroup, then the gradient norm at spdm_adam_norm_index().
 *
 * spdm_adam_step.  One step over h_segments[0 .. n_segments) (a HOST array), enqueued on `stream` (NULL: the null stream,
 * and the call synchronises).  `step` >= 1 is the count INCLUDING this step (state['step'] after torch's increment).
 *  max_norm > 0: the norm of ALL segments' gradients together is taken in float64 -- per-workgroup partial sums over ranges
 *    that depend on the segment sizes only, added in index order -- stored at d_workspace[spdm_adam_norm_index()], and every
 *    gradient enters the update as g * coef with coef = min(1, max_norm / (norm + 1e-6)) evaluated in float64 and rounded once:
 *    clip_grad_norm_'s semantics, a non-finite norm propagating as there.  d_grad itself is only read and is NOT rescaled
 *    (clip_grad_norm_ rescales .grad in place).
 *  max_norm <= 0: no clipping, one launch, the workspace is not written.
 *  Then per element in fp32 (torch's Adam with amsgrad=False, weight_decay=0; each of the three right-hand sides ends in ONE
 *  fused multiply-add, division and square root are correctly rounded):
 *    m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *    p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),   bc1 = 1 - beta1^step, bc2 = 1 - beta2^step,
 *  with 1 - beta, lr / bc1 and sqrt(bc2) evaluated on the host in double and rounded once.  A beta is read as the shortest
 *  decimal that rounds to the given float (0.999f is 0.999): 1 - beta would otherwise carry beta's own rounding, 1e-5
 *  relative; and it multiplies m and v as an fp32 pair hi + lo, so that its rounding does not bias every step the same way.  d_param, d_exp_avg and d_exp_avg_sq are updated in place; an element with g = m = v = 0 keeps its bits (the
 *  `pos_encoding.pos_encoding` slot of a simple_Unet.py blob).
 * Deterministic: no atomics; two calls on the same inputs give bit-identical results.
 * SPDM_ERR_INVALID, before the GPU is touched: a null pointer; n_segments outside 1 .. SPDM_OPTIM_MAX_SEGMENTS; numel == 0;
 * step < 1; a pointer that is not 16-byte aligned; lr, eps or a beta that is not finite; a beta outside [0, 1); max_norm NaN.
 *
 * spdm_adam_norm_index.  Pure host call: the index (in doubles) of the gradient norm inside the workspace. */
#define SPDM_OPTIM_MAX_SEGMENTS 4
typedef struct { float* d_param; const float* d_grad; float* d_exp_avg; float* d_exp_avg_sq; uint64_t numel; } spdm_optim_segment;
size_t spdm_adam_workspace_doubles(void);
int  spdm_adam_step(int32_t device, const spdm_optim_segment* h_segments, int32_t n_segments, int64_t step,
                    float lr, float beta1, float beta2, float eps, float max_norm,
                    double* d_workspace, void* stream);
size_t spdm_adam_norm_index(void);

/* The exponential moving average of the weights on the device.  Replaces: the EMA that diffusion-policy code
 * bases keep beside their optimiser (diffusers' EMAModel.step: s.sub_(one_minus_decay * (s - p)) per parameter), which the
 * reference's train.py does not have and whose users validate and sample from the average.  Stateless: there is no handle;
 * the shadow is the caller's arrays and the decay is an argument (the warm-up schedule lives in optim.ema_decay).
 *
 * A segment is one flat fp32 device array of numel shadow floats with the parameter array it follows: the same segments
 * spdm_adam_step steps.  Both pointers must be 16-byte aligned and the two ranges disjoint.
 *
 * spdm_ema_step.  One update of h_segments[0 .. n_segments) (a HOST array) in ONE launch enqueued on `stream` (NULL: the null
 * stream, and the call synchronises); no workspace, nothing is read back.  Per element in fp32
 *    ema = ema - one_minus_decay * (ema - p)
 *  as three operations each rounded on its own (a subtraction, a multiplication, a subtraction; no fused multiply-add), which
 *  is bit for bit what torch's e.sub_((e - p) * one_minus_decay) computes -- and not what torch.lerp_ computes.
 *  one_minus_decay is float32(1.0 - decay) with the subtraction in double, rounded once by the caller.  one_minus_decay = 0
 *  leaves d_ema's bits; a NaN or an infinity in d_param reaches its own element only.  d_param is only read.
 * Deterministic: no atomics, no reduction, one thread per element; two calls on the same inputs give bit-identical results.
 * SPDM_ERR_INVALID, before the GPU is touched: h_segments null; n_segments outside 1 .. SPDM_OPTIM_MAX_SEGMENTS; a null
 * pointer; numel == 0; a pointer that is not 16-byte aligned; d_ema == d_param or overlapping ranges within a segment;
 * one_minus_decay NaN or outside [0, 1]. */
typedef struct { float* d_ema; const float* d_param; uint64_t numel; } spdm_ema_segment;
int  spdm_ema_step(int32_t device, const spdm_ema_segment* h_segments, int32_t n_segments, float one_minus_decay,
                   void* stream);

/* Host-only test hook (no GPU call): the launch geometry chosen for a split-precision 3x3 / 3x1 convolution with the
 * statistics epilogue -- out = {m_tile, n_tile, n_tiles, slots, ksplit, kernel, st_m_tile, st_n_tiles, reserved_slots,
 * combine_rows}; kernel: bit 0 = the small-grid kernel (conv_skinny.hip), bit 1 = the register-resident kernel (conv_reg.hip).
 * `switches` = 0 for the defaults. */
int  spdm_debug_geometry(int32_t M, int32_t N, int32_t K, int32_t HW, int32_t W, int32_t taps, uint32_t switches,
                         int32_t out[10]);

/* Host-only test hook (no GPU call): how the launch of the most recent spdm_op_gemm call on this process staged its input
 * slab -- 0: with halo rows (every kernel but conv_wide.hip's, its ragged or non-dividing tilings, SPDM_NO_WHOLE_TILES);
 * 1: whole-sample tiles (the tile is a whole number of samples: no halo rows, no clamps); 2: the same with ONE sample per tile
 * and a GroupNorm prologue (its statistics in scalar registers); -1: no spdm_op_gemm call has launched yet. */
int  spdm_debug_whole_tiles(void);

/* Host-only test hook (no GPU call): how many implicit-GEMM launches this process has enqueued, from a plan or from
 * spdm_op_gemm, that read torch.cat([upsample(x), skip]) through conv_wide.hip's slab loader (pro 4 on whole-sample two-source
 * tiles at large batch) instead of a materialised upsampled tensor.  A captured step counts once, not per replay.
 * SPDM_TUNE22=0 keeps it at 0. */
int  spdm_debug_fused_upsample_launches(void);

/* Host-only test hook (no GPU call): how many launches this process has enqueued from a plan whose epilogue also wrote the
 * MaxPool2d(2) of their output for the next Down block (conv_reg.hip on width-8 maps at large batch: pool 1, raw with the
 * GroupNorm still pending; sa_tail.hip: pools 2 and 3), in place of a pool_kernel launch.  A captured step counts once, not
 * per replay.  SPDM_TUNE23 (read once per process) selects the pools: bit 0, 1, 2 = pool 1, 2, 3; default 7; 0 keeps it at 0. */
int  spdm_debug_pooled_epilogue_launches(void);

/* Host-only test hook (no GPU call, nothing launched): the kernel routes the plan of one U-Net evaluation at batch B chooses
 * on this handle (its config, switches and weight copies), as SPDM_PLAN_ROUTES_INTS values in out[0 .. cap):
 *   [0..2]   pool 1, 2, 3:     0 pool_kernel, 1 read through by the next convolution (pro 3), 2 written by the producer's epilogue
 *   [3..5]   up block 1, 2, 3: 0 upsample + concat kernel, 1 read through by the next convolution (pro 4), 2 upsample kernel +
 *            two-source convolution
 *   [6..11]  the FiLM tail of down1..3, up1..3: 0 film_apply, 1 film_coef, 2 coefficients evaluated in the consumers
 *   [12..41] sa1..6, five values each: {fused, crop, outc, in, tail} -- fused 1: sa_fused64 takes the block, crop 1: for the
 *            tokens outc reads only, outc 1: with outc in its epilogue; fused 0: in = 0 in_proj GEMM, 1 sa_qkv, 2 sa_head (core
 *            included) feeds the attention core, tail = 1 sa_tail, 0 the three GEMMs after it.
 *   [42..43] the level-3 convolution chains (conv_chain.hip): down block 3, the bottleneck -- 1: one fused launch, 0: one
 *            launch per convolution
 * All zero for a handle without attention (sa values) or a SPDM_FLAG_SIMPLE_UNET handle (everything).  SPDM_ERR_STATE before
 * spdm_load_weights, SPDM_ERR_INVALID for a null handle, B outside [1, max_batch] or cap < SPDM_PLAN_ROUTES_INTS. */
#define SPDM_PLAN_ROUTES_INTS 44
int  spdm_debug_plan_routes(const spdm_handle* h, int32_t B, int32_t* out, int32_t cap);

/* Op-level test hook: d_y = GELU(d_x) evaluated with the device erf that the conv prologues use
 * (nn.GELU(), models/Unet_FiLmLayer.py:104). */
int  spdm_op_gelu(const float* d_x, float* d_y, size_t n, void* stream);

/* Op-level test hook: ONE implicit-GEMM launch of the product (a 3x3 / 3x1 convolution or a Linear layer, with its load
 * prologue and store epilogue) on caller-supplied device tensors, synchronously.  The launch is built as the plan builds it:
 * geometry, split-K + combine (on a partial buffer the hook allocates), the split and fragment-order weight copies packed by
 * the weight loader's own code from the torch-layout host weight, and the kernel-selection switches read from the
 * environment (SPDM_NO_WIDE, SPDM_NO_SKINNY, ... as spdm_create reads them).  Not on the product path.
 * Shapes: the output is B x (H x W) rows of N channels; K = input channels per tap; taps 9 (3x3 conv, weight (N, K, 3, 3)),
 * 3 (3x1 conv of a W == 1 map, the centre column of a (N, K, 3, 3) weight) or 1 (Linear, weight (N, K), H = W = 1).
 * Statistics buffers are the kernels' raw fp64 partials: [sample][slot][2] = {sum x, sum x^2}, `slots` per sample, slot of
 * tile (mt, nt) = (mt - first m-tile of the sample) * n_tiles + nt; a Linear's per-row statistics use sample = row.
 * Invalid combinations (the plan's own guards: fused sources, two-source inputs, K % 32, N % 64, ...) return
 * SPDM_ERR_INVALID without launching anything. */
typedef struct {
    int32_t B, H, W, K, N, taps;
    int32_t split;                  /* 1: split-fp16 MFMA path, 0: exact fp32 path */
    int32_t pro;                    /* 0 none, 1 GroupNorm, 2 GroupNorm + GELU, 3 MaxPool2d(2) read-through, 4 upsample + concat */
    int32_t epi;                    /* 0 GroupNorm statistics, 1 bias, 2 bias + GELU, 3 bias + residual, 4 plain */
    const float* d_src;  int32_t src_ld;          /* pro 3: the (2H x 2W) map; pro 4: the (H/2 x W/2) map of up_C channels */
    const float* d_skip; int32_t skip_ld;  int32_t up_C;   /* two-source / pro 4 input: channels [up_C, K) from skip */
    const float* h_weight;          /* HOST, torch layout */
    /* pending GroupNorm (or, taps == 1, LayerNorm) of src and of skip: partials as a producer wrote them (d_*_stats NULL: none) */
    const double* d_src_stats; int32_t src_slots, src_m_tile, src_n_tiles, src_cnorm;   /* cnorm: channels the statistics divide by */
    const float* d_gamma; const float* d_beta;
    const double* d_skip_stats; int32_t skip_slots, skip_m_tile, skip_n_tiles, skip_cnorm;
    const float* d_skip_gamma; const float* d_skip_beta;
    const float* d_bias; const float* d_resid; int32_t resid_ld;
    float* d_dst; int32_t dst_ld;
    double* d_stats; size_t stats_cap;            /* epi 0: output partials, capacity in doubles */
    double* d_row_stats; size_t row_stats_cap;    /* optional (taps == 1): per-row partials of the stored values */
    int32_t out[10];                /* as recorded by the launch that ran: {kernel (0 conv_gemm, 1 conv_skinny, 2 conv_reg64,
                                       3 conv3x3_wide), variant (0 plain, 1 width-2 zero-tap skipping, 2 / 3 width-4 / width-8 row
                                       classes, 4 pipelined slab hand-over, 5 two chunks per hand-over), m_tile, n_tile of the
                                       kernel, ksplit, two_source, fused_source, stats slots, stats m_tile, stats n_tiles} */
} spdm_op_gemm_args;

int  spdm_op_gemm(spdm_op_gemm_args* args);

/* Op-level test hook: ONE fused launch of csrc/conv_chain.hip -- a list of 3-tap convolutions of a width-1 map (split
 * precision) with the GroupNorm(1, C) [-> GELU] between two layers applied inside the kernel -- on caller-supplied tensors,
 * synchronously.  The weights are laid out by the weight loader's own code (the fragment-order split copies).  Not on the
 * product path.
 *   B samples of HW rows (HW a power of two in [4, 64]); chan[0 .. n_layers]: the widths, input first (multiples of 64, <= 512);
 *   layer i maps chan[i] -> chan[i + 1] channels with the HOST weight h_weight[i], laid out [3][chan[i + 1]][chan[i]];
 *   d_gamma[i] / d_beta[i] (i >= 1, DEVICE, chan[i] floats): the GroupNorm pending on layer i's input; gelu[i] != 0: GELU
 *   follows it.  Entry 0 of the three is not read: d_src is a finished tensor.
 *   d_dst: the raw output of the last layer, [B x HW][dst_ld]; d_stats: its GroupNorm partials, [sample][slots][2] fp64 =
 *   {sum x, sum x^2} in slot 0 (stats m_tile 64, one n-tile), stats_cap in doubles; unwritten slots read as NaN.
 *   out: {workgroups, slots, stats m_tile, stats n_tiles}.
 * SPDM_ERR_INVALID, nothing launched, for shapes the kernel's predicate refuses or weights outside the split format's range. */
#define SPDM_OP_CHAIN_MAX_LAYERS 8
typedef struct {
    int32_t B, HW, n_layers;
    int32_t chan[SPDM_OP_CHAIN_MAX_LAYERS + 1];
    int32_t gelu[SPDM_OP_CHAIN_MAX_LAYERS];
    const float* d_src;  int32_t src_ld;
    const float* h_weight[SPDM_OP_CHAIN_MAX_LAYERS];
    const float* d_gamma[SPDM_OP_CHAIN_MAX_LAYERS];
    const float* d_beta[SPDM_OP_CHAIN_MAX_LAYERS];
    float* d_dst;  int32_t dst_ld;
    double* d_stats;  size_t stats_cap;
    int32_t out[4];
} spdm_op_chain_args;

int  spdm_op_chain(spdm_op_chain_args* args);

/* Host-only test hook (no GPU call): how many fused conv_chain.hip launches this process has enqueued from a plan (down block 3
 * and the bottleneck of a U-Net evaluation: two per evaluation where both routes are taken).  A captured step counts once, not
 * per replay.  SPDM_TUNE25 (read once per process) selects the sites: bit 0 down block 3, bit 1 the bottleneck, bit 2 takes
 * them at any batch (otherwise only from 256 blocks of 64 rows on); 0 keeps it at 0. */
int  spdm_debug_conv_chain_launches(void);

/* Op-level test hook: ONE launch of the training pass (launch_* of csrc/train.hip, train_attn.hip, train_simple.hip) exactly
 * as spdm_train_loss_grad calls it, on caller-supplied tensors, synchronously on the current device.  Not on the product path.
 * The hook validates, uploads the host integer arrays, calls the launcher and synchronises -- nothing else.
 *   d_buf[i] / cap[i]   DEVICE float arrays and their capacities in floats; every array an op reads or writes must be non-NULL
 *                       and at least as large as the extent given below (optional ones may be NULL, cap ignored)
 *   h_idx[i] / n_idx[i] HOST int32 arrays (indices a kernel dereferences with): range-checked, then uploaded by the hook
 *   info[]              filled by the hook (-1 where unused)
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args, an unknown op, a dimension that is not positive or outside the
 * launcher's limits, a capacity below the extent, an index outside its range, an extent beyond 31 (element counts the kernels
 * index with int) or 63 bits.  SPDM_ERR_HIP: the launch or the final synchronise failed.
 * Deterministic: every op gives the same bits on the same inputs.  Tensors are channels-last, rows of `ld` floats.
 *
 * op, dim[] (all others 0), buffers with their extents; M = B H W throughout:
 *  WGRAD         dim {B, H, W, taps, Co, Ci, conv9, ldy, ldx}; taps 9, 3 (W == 1) or 1 (H == W == 1, conv9 == 0); conv9 == 1 for
 *                taps 9 / 3.  buf {dy [(M-1) ldy + Co], x [(M-1) ldx + Ci], dst [Co Ci (conv9 ? 9 : 1)] out}.
 *                info {chunks, rows per chunk} as wgrad_chunks chose them under the product's slab budget; the slabs are the hook's.
 *  WGRAD_MAPPED  dim {B, H, W, taps, Co, Ci, no, ni}; taps 9 or 3 (W == 1).  buf {dy [M Co], x [M Ci], dst [no ni 9] out};
 *                h_idx {pos_o [no] in [0, Co), pos_i [ni] in [0, Ci)}.  info as WGRAD.
 *  COLSUM        dim {M, C, ld}, ld >= C.  buf {src [(M-1) ld + C], dst [C] out}.
 *  GN_STATS      dim {B, n, cnt}; cnt == 0: launch_gn_stats (divisor n), else launch_gn_stats_real with 1 <= cnt <= n.
 *                buf {y [B n], mean [B] out, rstd [B] out}.
 *  GN_BWD        dim {B, HW, C, gelu}; C a power of two <= 512.  buf {y [B HW C], mean [B], rstd [B], gamma [C], beta [C],
 *                g [B HW C], dy [B HW C] out, dgb [B C 2] out}.
 *  FILM_BWD      dim {B, HW, C, t_count, T}; C as GN_BWD; t_count 1 or B.  buf {z [B HW C], temb [T C], film [B 2C] or NULL,
 *                dout [B HW C], dz [B HW C] out, de [B C] out, dfilm [B 2C] out (NULL exactly when film is)};
 *                h_idx {t [t_count] in [0, T)}.
 *  MSE           dim {B, H0, D, Hp, Wp, lh, lw}; lh, lw >= 0, lh + H0 <= Hp, lw + D <= Wp.  buf {eps_pad [B Hp Wp],
 *                noise [B H0 D], loss [1] out, deps_pad [B Hp Wp] out, eps_out [B H0 D] out or NULL}.
 *  POOL_BWD      dim {B, H, W, C}; H, W even.  buf {in [B H W C], dout [B H/2 W/2 C], din [B H W C] in/out (accumulated into)}.
 *  UP_BWD        dim {B, h, w, C, ld}; ld >= C.  buf {dcat [(4 B h w - 1) ld + C], dx [B h w C] in/out (accumulated into)}.
 *  MISH_BWD      dim {nblk, B, ld, cond_dim}; ld >= cond_dim.  buf {dm [(nblk B - 1) ld + cond_dim], cond [B cond_dim],
 *                grad_cond [B cond_dim] out}.
 *  LN_FWD        dim {rows, C}; C 64, 128 or 256.  buf {x [rows C], gamma [C], beta [C], y [rows C] out, mean [rows] out,
 *                rstd [rows] out}.
 *  LN_BWD        dim {rows, C}.  buf {x [rows C], mean [rows], rstd [rows], gamma [C], gy [rows C], add [rows C] or NULL,
 *                dx [rows C] out, part [blocks 2C] out}.  info {blocks = ln_bwd_blocks(rows)}.
 *  GELU_BWD      dim {n}.  buf {u [n], dh [n], du [n] out}.
 *  ATTN_FWD_LSE  dim {B, L, C, heads}; attn_train_supported(L, C, heads).  buf {qkv [B L 3C], out [B L C] out,
 *                lse [B heads L] out}.
 *  ATTN_BWD      dim as ATTN_FWD_LSE.  buf {qkv [B L 3C], out [B L C], dout [B L C], lse [B heads L], dqkv [B L 3C] out}.
 *  GN_BWD_MAPPED dim {B, HW, C, gelu, nreal}; C a multiple of 64 <= 512.  buf as GN_BWD; h_idx {pos [nreal], distinct, in [0, C)}.
 *  SIMPLE_TAIL_BWD  dim {B, HW, Co, Cr, Cz, cemb_ld}; Co a multiple of 64 <= 512, Cr <= Cz <= Co, Cr + 32 <= Co, cemb_ld >= 32.
 *                buf {dout [B HW Co], dz [B HW Cz] out, dtemb [B Cr] out, dcemb [(B-1) cemb_ld + 32] out}.
 *  SILU_BWD      dim {B, cond_dim, ld}; ld >= cond_dim.  buf {ds [(B-1) ld + cond_dim], cond [B cond_dim],
 *                grad_cond [B cond_dim] out}. */
enum {
    SPDM_OPT_WGRAD = 0, SPDM_OPT_WGRAD_MAPPED, SPDM_OPT_COLSUM, SPDM_OPT_GN_STATS, SPDM_OPT_GN_BWD, SPDM_OPT_FILM_BWD,
    SPDM_OPT_MSE, SPDM_OPT_POOL_BWD, SPDM_OPT_UP_BWD, SPDM_OPT_MISH_BWD, SPDM_OPT_LN_FWD, SPDM_OPT_LN_BWD, SPDM_OPT_GELU_BWD,
    SPDM_OPT_ATTN_FWD_LSE, SPDM_OPT_ATTN_BWD, SPDM_OPT_GN_BWD_MAPPED, SPDM_OPT_SIMPLE_TAIL_BWD, SPDM_OPT_SILU_BWD,
    SPDM_OPT_COUNT
};
#define SPDM_OP_TRAIN_DIMS 10
#define SPDM_OP_TRAIN_BUFS 8
#define SPDM_OP_TRAIN_IDX 2
typedef struct {
    int32_t op;
    int32_t reserved;
    int64_t dim[SPDM_OP_TRAIN_DIMS];
    float* d_buf[SPDM_OP_TRAIN_BUFS];
    uint64_t cap[SPDM_OP_TRAIN_BUFS];
    const int32_t* h_idx[SPDM_OP_TRAIN_IDX];
    int64_t n_idx[SPDM_OP_TRAIN_IDX];
    int32_t info[4];
} spdm_op_train_args;

int  spdm_op_train(spdm_op_train_args* args);

/* Op-level test hook: ONE launch of a streaming kernel of the forward / sampling path (launch_* of csrc/elementwise.hip) exactly
 * as the plan calls it, on caller-supplied tensors, synchronously on the current device.  Not on the product path.
 * The hook validates, uploads the host integers (index arrays, the step word, the Philox words, the ptrs_dev block), builds
 * AffineSrc / StatsRef / StepArgs, calls the launcher and synchronises -- nothing else; it has no arithmetic of its own.
 *   d_buf[i] / cap[i]   DEVICE float arrays and capacities in floats, as for spdm_op_train (optional ones may be NULL)
 *   h_idx[i] / n_idx[i] HOST int32 arrays: range-checked where a kernel dereferences with them, then uploaded
 *   gn[k]               a GroupNorm(1, C) still pending on source k, described as spdm_op_gemm describes it: d_stats the raw
 *                       fp64 partials [B][slots][2] a producer left (NULL: no GroupNorm; every other field of gn[k] then 0 / NULL),
 *                       stats_cap in doubles, the producer's m_tile and n_tiles, cnorm the channels the statistics divide by
 *                       (1 <= cnorm <= C; inv_count = 1 / (cnorm HW)), gamma and beta of affine_cap floats each (>= the channels
 *                       the op applies them to).  The consumer reads, for sample b, slots [0, ((b HW + HW - 1) / m_tile -
 *                       b HW / m_tile + 1) n_tiles): `slots` must be at least the largest such count.
 *   d_stats_out / stats_out_cap   DEVICE fp64 partials a producer op writes (capacity in doubles)
 *   d_words             DEVICE int32[3] = {step word, t word, flag}: written by the hook before the launch ({step0 or step, -1, 0}),
 *                       then by the kernel; required by CONV_IN (adv >= -1) and OUT_STEP, NULL otherwise
 *   info[]              filled by the hook (-1 where unused)
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args, an unknown op, a dimension that is not positive or outside its range
 * below, a capacity below the extent, a buffer an op does not take, an index or timestep outside its range, a slot count smaller
 * than the consumer reads, an extent beyond 31 bits, anything the launcher refuses -- and what a launcher accepts but its kernel
 * cannot run (DESIGN.md 8.16 lists those).  SPDM_ERR_HIP: the launch or the final synchronise failed.
 * Deterministic: every op gives the same bits on the same inputs.  Tensors are channels-last.
 *
 * op, dim[] (all others 0), buffers with their extents:
 *  CONV_IN       dim {B, H0, D, Hp, Wp, lh, lw, B_geom, adv, n_steps, step0}; lh, lw >= 0, lh + H0 <= Hp, lw + D <= Wp,
 *                (Hp Wp + 8) floats within 64 KiB of LDS; B_geom >= 0 (0: row parts as for B); adv -2 (no bookkeeping: n_steps =
 *                step0 = 0, no h_idx, no d_words), -1 (step <- step0 + 1) or 0 .. n_steps (step <- adv); 0 <= step0 < n_steps.
 *                buf {x [B H0 D], w [9 64] = [tap][channel], dst [B Hp Wp 64] out}; h_idx {timesteps [n_steps], >= 0};
 *                d_stats_out [B slots 2], of which the kernel writes slots [0, parts) of each sample.  info {parts, slots}.
 *  POOL          dim {B, H, W, C}; H, W even, C a multiple of 4 <= 1024.  buf {src [B H W C], dst [B H/2 W/2 C] out}; gn[0].
 *  UPCAT         dim {B, Hin, Win, Cu, Cs}; Cu >= 4, Cs >= 0 (0: no skip source), both multiples of 4, Cu + Cs <= 1024.
 *                buf {up [B Hin Win Cu], skip [B 4 Hin Win Cs] (NULL exactly when Cs == 0), dst [B 4 Hin Win (Cu + Cs)] out};
 *                gn[0] on up (HW = Hin Win), gn[1] on skip (HW = 4 Hin Win).
 *  FILM_APPLY    dim {B, HW, C, t_count, T}; C in {4, 8, ..., 1024} (C / 4 divides 256); t_count 1 or B.
 *                buf {src [B HW C], temb [T C] or NULL, film [B 2C] or NULL, dst [B HW C] out}; h_idx {t [t_count] in [0, T)}
 *                exactly when temb is given (without temb: t_count = T = 1); gn[0]; d_stats_out [B HW 2] or NULL: per-row
 *                {sum, sum^2} of dst, C in {64, 128, 256} only.  With temb, film, gn[0] and d_stats_out all absent: launch_gn_apply.
 *  FILM_COEF     dim as FILM_APPLY, any C >= 1.  buf {temb [T C] or NULL, film [B 2C] or NULL, ab [B 2C] out}; h_idx as FILM_APPLY;
 *                gn[0] (no tensor is read: the statistics, gamma and beta only).
 *  LAYERNORM     dim {rows, C}; C 64, 128, 256 or 512.  buf {x [rows C], gamma [C], beta [C], y [rows C] out}.
 *  MISH_PAD, SILU_PAD  dim {B, cond_dim, Kp}; Kp >= cond_dim.  buf {cond [B cond_dim], dst [B Kp] out}.
 *  SILU          dim {n}.  buf {x [n], y [n] out}.
 *  DC_FINISH     dim {B, HW, C}; C a multiple of 4 <= 1024.  buf {src [B HW C], res [B HW C] or NULL, dst [B HW C] out}; gn[0].
 *  SIMPLE_TAIL   dim {B, HW, Co, Cr, src_C, temb_ld, cemb_ld, t_count, T}; Co, Cr, src_C, temb_ld, cemb_ld multiples of 4,
 *                Co <= 1024, 4 <= Cr <= src_C, Cr + 32 <= Co, temb_ld >= Cr, cemb_ld >= 32, t_count 1 or B.
 *                buf {src [B HW src_C], temb [(T-1) temb_ld + Cr], cemb [(B-1) cemb_ld + 32], dst [B HW Co] out};
 *                h_idx {t [t_count] in [0, T)}; gn[0] (gamma, beta: >= Cr floats; cnorm <= src_C).
 *  SPLITK_COMBINE  dim {B, HW, N, ksplit}; N a multiple of 4, ksplit >= 2.  buf {partial [ksplit][B HW N], dst [B HW N] out};
 *                d_stats_out [B slots 2], of which the kernel writes slots [0, HW / rows).  info {rows = combine_rows(HW, N), slots}.
 *  OUT_STEP      dim {B, H0, D, Hp, Wp, lh, lw, kind, mode, step, n_steps, inp_h, inpaint_per_sample, indirect}; padding as
 *                CONV_IN; kind 0 DDPM, 1 DDIM; mode 0 eps only (eps written, nothing else touched), 1 the full step from the
 *                features, 2 the full step from a given eps; 0 <= step < n_steps; 0 <= inp_h <= H0; the two flags 0 / 1.
 *                buf {feat [B Hp Wp 64] (modes 0, 1), w [64] (modes 0, 1), eps [B H0 D] (mode 0: out, mode 2: in, mode 1: NULL),
 *                x [B H0 D] in/out (modes 1, 2), coef [n_steps 6] (modes 1, 2), noise [n_steps B H0 D] or NULL (NULL: the Philox
 *                stream {seed, first_index} is handed to the kernel instead), inpaint [inp_h D], or [B inp_h D] with
 *                inpaint_per_sample (exactly when inp_h > 0), history [(n_steps + 1) B H0 D] in/out or NULL}; `bias` is outc's.
 *                indirect 1 hands inpaint / noise / history to the kernel through a ptrs_dev block the hook writes.
 *                d_words: {step (unchanged), -1, flag}. */
enum {
    SPDM_OPS_CONV_IN = 0, SPDM_OPS_POOL, SPDM_OPS_UPCAT, SPDM_OPS_FILM_APPLY, SPDM_OPS_FILM_COEF, SPDM_OPS_LAYERNORM,
    SPDM_OPS_MISH_PAD, SPDM_OPS_SILU_PAD, SPDM_OPS_SILU, SPDM_OPS_DC_FINISH, SPDM_OPS_SIMPLE_TAIL, SPDM_OPS_SPLITK_COMBINE,
    SPDM_OPS_OUT_STEP,
    SPDM_OPS_COUNT
};
#define SPDM_OP_STREAM_DIMS 14
#define SPDM_OP_STREAM_BUFS 8
#define SPDM_OP_STREAM_IDX 1
#define SPDM_OP_STREAM_GN 2
typedef struct {
    const double* d_stats;
    uint64_t stats_cap;
    int32_t slots;
    int32_t m_tile;
    int32_t n_tiles;
    int32_t cnorm;
    const float* d_gamma;
    const float* d_beta;
    uint64_t affine_cap;
} spdm_op_stream_gn;
typedef struct {
    int32_t op;
    int32_t reserved;
    int64_t dim[SPDM_OP_STREAM_DIMS];
    float* d_buf[SPDM_OP_STREAM_BUFS];
    uint64_t cap[SPDM_OP_STREAM_BUFS];
    const int32_t* h_idx[SPDM_OP_STREAM_IDX];
    int64_t n_idx[SPDM_OP_STREAM_IDX];
    spdm_op_stream_gn gn[SPDM_OP_STREAM_GN];
    double* d_stats_out;
    uint64_t stats_out_cap;
    int32_t* d_words;
    uint64_t seed;
    uint64_t first_index;
    float bias;
    int32_t info[4];
    int32_t reserved2;
} spdm_op_stream_args;

int  spdm_op_stream(spdm_op_stream_args* args);

/* Op-level test hook: ONE launch of the observation encoder or of the autoencoder's decoder (launch_* of csrc/encoder.hip,
 * csrc/encoder_train.hip, csrc/decoder.hip, and launch_wgrad under the slab budgets of the two passes) exactly as
 * spdm_encoder_* / spdm_decoder_* call it, on caller-supplied tensors, synchronously on the current device.  Not on the
 * product path.  The hook validates, allocates the scratch the product allocates (the partial rows of conv 1 and of layer 6,
 * the column-sum slabs, the weight gradient's slabs: its own, within the product's sizes, filled with NaN first), calls the
 * launcher and synchronises -- nothing else; it has no arithmetic of its own.
 *   d_buf[i] / cap[i]   DEVICE float arrays and capacities in floats, as for spdm_op_train (optional ones may be NULL)
 *   d_sq / sq_cap       DEVICE float64 array: the per-frame sums of squared errors (DEC_CONVS with train: out; DEC_LOSS: in)
 *   scale               DEC_BWD6: the factor of (recon - target), 2 / (n 27648) in the product
 *   info[]              filled by the hook (-1 where unused)
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args, an unknown op, a dimension that is not positive or outside what the
 * two passes produce, a capacity below the extent, a buffer the op does not take, an extent beyond 31 bits, a scale that is
 * not finite.  SPDM_ERR_HIP: the launch or the final synchronise failed.  Deterministic: the same bits on the same inputs.
 * Weights are in the KERNEL layouts the launchers read.  Encoder: torch's own (cout, cin, 2, 2).  Decoder: a transposed
 * convolution (cin, cout, 2, 2) as w[ci][kk][co], kk = ky 2 + kx; the Linear's rows and bias as q 64 + c (Flatten order is
 * c 144 + q).  Row orders (csrc/decoder.hip): h0 [n 144][64], a1 [n 576][32] with row r2 = (n 144 + q) 4 + kk1, a2 [n 2304][16]
 * with row r3 = r2 4 + kk2, recon NCHW.  Encoder (csrc/encoder_train.hip): feat [n][co 144 + q], x3 [n 144][ci 4 + ky 2 + kx],
 * x2 [(n 144 + q) 4 + kk][c1 4 + ky 2 + kx].  n <= 2048 frames (one chunk of the passes) for every per-frame op but DEC_LOSS.
 *
 * op, dim[] (all others 0), buffers with their extents:
 *  ENC_CONVS     dim {n, train}; train 0: launch_encoder_convs, 1: launch_encoder_train_convs.  buf {img [n 27648], w1 [192],
 *                b1 [16], w2 [2048], b2 [32], w3 [8192], b3 [64], feat [n 9216] out, x3 [n 18432] out (train == 1, else NULL)}.
 *  ENC_KINKS     dim {n}.  buf as ENC_CONVS with train; feat and x3 in/out.
 *  ENC_X2        dim {n}.  buf {img [n 27648], w1 [192], b1 [16], x2 [n 36864] out}.
 *  ENC_DZ3       dim {n}.  buf {dfeat [n 9216], feat [n 9216], dz3 [n 9216] out}.
 *  ENC_DZ2       dim {n}.  buf {dx3 [n 18432], x3 [n 18432], dz2 [n 18432] out}.
 *  ENC_CONV1_WGRAD  dim {n}.  buf {img [n 27648], dx2 [n 36864], x2 [n 36864], dw [192] out, db [16] out}.  info {blocks}.
 *  ADD           dim {n} (elements, not frames).  buf {src [n], dst [n] in/out}.
 *  DEC_CONVS     dim {n, train}; train 0: launch_decoder_convs, 1: launch_decoder_train_convs.  buf {h0 [n 9216], w2 [8192],
 *                b2 [32], w4 [2048], b4 [16], w6 [192], b6 [3], recon [n 27648] out, target [n 27648], a1 [n 18432] out,
 *                a2 [n 36864] out}; d_sq [n] out.  target, a1, a2 and d_sq go with train == 1 and must be NULL otherwise.
 *  DEC_KINKS     dim {n}.  buf {latent [n 128], w0 [9216 128], b0 [9216], w2, b2, w4, b4, a1 [n 18432] in/out,
 *                a2 [n 36864] in/out}.
 *  DEC_LOSS      dim {n}, any n > 0 (the loss is formed over all frames of a call).  d_sq [n] in; buf {loss [1] out}.
 *  DEC_BWD6      dim {n}; scale.  buf {recon [n 27648], target [n 27648], a2 [n 36864], w6 [192], dz4 [n 36864] out,
 *                dw [192] out (torch order ci 12 + co 4 + kk), db [3] out}.
 *  DEC_DGRAD4    dim {n}.  buf {dz4 [n 576 64], a1 [n 576 32], w4 [2048], dz2 [n 576 32] out}.
 *  DEC_COLSUM    dim {M, C, fold}; fold 4: C 64 (M <= 2048 576) or 128 (M <= 2048 144), dst [C / 4]; fold 1: C 9216, M <= 2048,
 *                dst [9216] in Flatten order.  buf {src [M C], dst out}.  info {slab_rows, slabs}.
 *  DEC_UNPERM_CONV    dim {cin, cout}: (64, 32), (32, 16) or (16, 3).  buf {src [cin 4 cout], dst [cin cout 4] out}.
 *  DEC_UNPERM_LINEAR  no dims.  buf {src [9216 128], dst [9216 128] out}.
 *  FRAME_WGRAD   dim {M, which}; launch_wgrad with taps 1 on dy [M Co], x [M Ci] under the budget of the pass that runs it:
 *                which 0 encoder Linear (Co 128, Ci 9216, M <= 2048), 1 encoder conv 3 (64, 128, M <= 2048 144), 2 encoder
 *                conv 2 (32, 64, M <= 2048 576) -- all under ENC_WG_FLOATS; 3 decoder layer 4 (32, 64, M <= 2048 576, 256 slabs),
 *                4 decoder layer 2 (64, 128, M <= 2048 144, 256 slabs), 5 decoder Linear (9216, 128, M <= 2048, DEC_WG_FLOATS).
 *                buf {dy [M Co], x [M Ci], dst [Co Ci] out}.  info {chunks, rows per chunk, Co, Ci}. */
enum {
    SPDM_OPF_ENC_CONVS = 0, SPDM_OPF_ENC_KINKS, SPDM_OPF_ENC_X2, SPDM_OPF_ENC_DZ3, SPDM_OPF_ENC_DZ2, SPDM_OPF_ENC_CONV1_WGRAD,
    SPDM_OPF_ADD, SPDM_OPF_DEC_CONVS, SPDM_OPF_DEC_KINKS, SPDM_OPF_DEC_LOSS, SPDM_OPF_DEC_BWD6, SPDM_OPF_DEC_DGRAD4,
    SPDM_OPF_DEC_COLSUM, SPDM_OPF_DEC_UNPERM_CONV, SPDM_OPF_DEC_UNPERM_LINEAR, SPDM_OPF_FRAME_WGRAD,
    SPDM_OPF_COUNT
};
#define SPDM_OP_FRAME_DIMS 4
#define SPDM_OP_FRAME_BUFS 11
typedef struct {
    int32_t op;
    int32_t reserved;
    int64_t dim[SPDM_OP_FRAME_DIMS];
    float* d_buf[SPDM_OP_FRAME_BUFS];
    uint64_t cap[SPDM_OP_FRAME_BUFS];
    double* d_sq;
    uint64_t sq_cap;
    float scale;
    int32_t info[4];
    int32_t reserved2;
} spdm_op_frame_args;

int  spdm_op_frame(spdm_op_frame_args* args);

/* Op-level test hook: ONE launch of a forward SelfAttention kernel (launch_* of csrc/sa_fused.hip, sa_tail.hip, attention.hip)
 * exactly as the plan's attention block calls it, on caller-supplied tensors, synchronously on the current device.  Not on the
 * product path.  The hook validates, lays the block's weights out with the weight loader's own code (as spdm_op_gemm does: the
 * hi / lo fp16 halves in sa_fused.hip's fragment order for C = 64, the fragment-order split copy for C = 128 / 256), uploads the
 * host timesteps, builds FilmSpec / SaCrop, calls the launcher and synchronises -- nothing else; no arithmetic of its own.
 * heads = 4 as in the product; d = C / 4.
 *   d_buf[i] / cap[i]   DEVICE float arrays and capacities in floats, as for spdm_op_train (a buffer an op does not take: NULL)
 *   h_w[i]              HOST weights in torch layout: {in_proj (3C, C), out_proj (C, C), ff_self.1 (C, C), ff_self.3 (C, C)};
 *                       exactly those the op reads (below), the others NULL.  A weight outside the split format's range is
 *                       refused as the plan refuses it (its block runs on the GEMM chain): SPDM_ERR_INVALID, nothing launched.
 *   d_vec[i] / vec_cap[i]   DEVICE vectors: {ln gain [C], ln bias [C], in_proj bias [3C], out_proj bias [C], ff_self.0 gain [C],
 *                       ff_self.0 bias [C], ff_self.1 bias [C], ff_self.3 bias [C]}; exactly those the op reads
 *   d_ab / ab_cap       optional [B 2C]: the block input is A x + B per (sample, channel), rows [A (C) | B (C)] as FILM_COEF of
 *                       spdm_op_stream writes them
 *   film_on             1: the kernel evaluates those coefficients itself (FilmSpec), from what spdm_op_stream's FILM_COEF
 *                       takes: gn (a pending GroupNorm(1, C) of the raw tensor, HW = L), d_temb [T C] with h_t, t_count (1 or B)
 *                       HOST timesteps in [0, T) (without temb: h_t NULL, t_count = T = 1), d_film [B 2C] or NULL.
 *                       d_ab and film_on are mutually exclusive; film_on 0: every FilmSpec field 0 / NULL.  CORE takes neither.
 *   d_outc_w, outc_b    FUSED64 with outc: outc's weight [64] (DEVICE) and bias
 *   info[]              filled by the hook (-1 where unused): {kernel (0 sa_fused64, 1 sa_fused64 on two workgroups per sample,
 *                       2 sa_crop64, 3 sa_qkv, 4 sa_head, 5 sa_tail, 6 attention_ds, 7 attention (VALU), 8 attention_mfma), waves
 *                       per workgroup, workgroups, wlds (sa_fused64: weights staged in LDS, persistent workgroups), qw (sa_crop64:
 *                       queries per wave)} -- recorded by the launcher that ran
 * Row order: every tensor is channels-last with row b L + token (rows = B L); qkv rows are [q (C) | k (C) | v (C)], each head h
 * in channels [h d, (h + 1) d); the q that QKV writes and CORE reads does NOT carry 1 / sqrt d (the core applies it).
 * SPDM_ERR_INVALID, before the GPU is touched: NULL args, an unknown op, a dimension outside its range below, a flag that is not
 * 0 / 1, a capacity below the extent, a buffer, weight or vector the op does not take, a timestep outside [0, T), a pending
 * GroupNorm with fewer slots than the consumer reads, an extent beyond 31 bits, everything the launcher itself refuses (asked of
 * the launcher, which decides before it touches the device) and what a launcher accepts but its kernel cannot run.
 * SPDM_ERR_HIP: the launch or the final synchronise failed.  Deterministic: every op gives the same bits on the same inputs.
 *
 * op, dim[] (all others 0), buffers with their extents:
 *  FUSED64  dim {B, L, no_wlds, crop, H0, D, Wp, lh, lw, outc}; C = 64, 1 <= L <= 512 (with d_ab / film_on: L <= 256).  no_wlds 1 =
 *           SPDM_SA_NO_WLDS.  crop 0: H0 = D = Wp = lh = lw = outc = 0.  crop 1: the tokens (lh + i) Wp + lw + j, i < H0, j < D only;
 *           L <= 256, Q = H0 D with 1 <= Q < L and Q <= 32 min(4, ceil(L / 32)), lw + D <= Wp, (lh + H0) Wp <= L.
 *           buf {x [B L 64], out [B L 64] out (crop: only the rows of the Q tokens are written; NULL with outc),
 *           eps [B H0 D] out (outc 1: eps = outc_w . out + outc_b; else NULL)}; h_w all four; d_vec all eight.
 *  QKV      dim {C, B, L}; C 128 or 256.  buf {x [B L C], qkv [B L 3C] out}; h_w {in_proj}; d_vec {0, 1, 2}.  film_on: the
 *           coefficient rows of the samples a tile touches must fit 24 KiB ((ceil((TM + L - 2) / L)) + 1) 2C floats, TM = 8192 / C).
 *  HEAD     dim {C, B, L}; C 128 or 256, L divides 8192 / C.  buf {x [B L C], att [B L C] out}; h_w {in_proj}; d_vec {0, 1, 2}.
 *  TAIL     dim {C, B, L}; C 128 or 256.  buf {att [B L C], x [B L C], out [B L C] out}; h_w {out_proj, ff_self.1, ff_self.3};
 *           d_vec {3, 4, 5, 6, 7}.  d_ab / film_on as QKV (they finish x, the residual).
 *  CORE     dim {B, L, C, valu}; C 64, 128 or 256; valu 1 = SPDM_ATTN_VALU.  launch_attention_auto: L >= 32 without valu runs
 *           attention_mfma, everything else the VALU kernels; a shape beyond 160 KiB of LDS is refused.
 *           buf {qkv [B L 3C], out [B L C] out}; no weights, no vectors. */
enum { SPDM_OPA_FUSED64 = 0, SPDM_OPA_QKV, SPDM_OPA_HEAD, SPDM_OPA_TAIL, SPDM_OPA_CORE, SPDM_OPA_COUNT };
#define SPDM_OP_SA_DIMS 10
#define SPDM_OP_SA_BUFS 3
#define SPDM_OP_SA_WEIGHTS 4
#define SPDM_OP_SA_VECS 8
typedef struct {
    int32_t op;
    int32_t reserved;
    int64_t dim[SPDM_OP_SA_DIMS];
    float* d_buf[SPDM_OP_SA_BUFS];
    uint64_t cap[SPDM_OP_SA_BUFS];
    const float* h_w[SPDM_OP_SA_WEIGHTS];
    const float* d_vec[SPDM_OP_SA_VECS];
    uint64_t vec_cap[SPDM_OP_SA_VECS];
    const float* d_ab;
    uint64_t ab_cap;
    int32_t film_on;
    int32_t t_count;
    int64_t T;
    spdm_op_stream_gn gn;
    const float* d_temb;
    uint64_t temb_cap;
    const int32_t* h_t;
    const float* d_film;
    uint64_t film_cap;
    const float* d_outc_w;
    uint64_t outc_w_cap;
    float outc_b;
    int32_t info[5];
} spdm_op_sa_args;

int  spdm_op_sa(spdm_op_sa_args* args);

#ifdef __cplusplus
}
#endif
#endif /* SPDM_H */
