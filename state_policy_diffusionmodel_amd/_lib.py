"""ctypes binding of libspdm_hip.so (include/spdm.h).  Fails loudly: there is no CPU
fallback and no alternative backend -- if the HIP library is missing or does not export
the ABI, importing the product path raises."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint64, c_void_p

from .weights import TensorIndex

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPDM_LIB") or os.path.join(HERE, "libspdm_hip.so")     # (SPDM_LIB: A/B builds during kernel tuning)

SPDM_DDPM, SPDM_DDIM, SPDM_DPMPP_2M = 0, 1, 2
SPDM_FLAG_DEBUG_KEEP = 1
SPDM_FLAG_EXACT_FP32 = 2
SPDM_FLAG_SIMPLE_UNET = 4
SPDM_FLAG_TRAIN = 8
SPDM_FLAG_TRAIN_ATTENTION = 16
SPDM_FLAG_TRAIN_SIMPLE = 32
SPDM_SELECT_MEDOID, SPDM_SELECT_COHERENT = 0, 1
SPDM_ERR_INVALID = -1
SPDM_ERR_STATE = -3
ABI_VERSION = 2


class SpdmOpGemmArgs(ctypes.Structure):
    """spdm_op_gemm_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("B", "H", "W", "K", "N", "taps", "split", "pro", "epi")] +
                [("d_src", c_void_p), ("src_ld", c_int32), ("d_skip", c_void_p), ("skip_ld", c_int32), ("up_C", c_int32),
                 ("h_weight", c_void_p),
                 ("d_src_stats", c_void_p)] + [(n, c_int32) for n in ("src_slots", "src_m_tile", "src_n_tiles", "src_cnorm")] +
                [("d_gamma", c_void_p), ("d_beta", c_void_p),
                 ("d_skip_stats", c_void_p)] + [(n, c_int32) for n in ("skip_slots", "skip_m_tile", "skip_n_tiles", "skip_cnorm")] +
                [("d_skip_gamma", c_void_p), ("d_skip_beta", c_void_p),
                 ("d_bias", c_void_p), ("d_resid", c_void_p), ("resid_ld", c_int32),
                 ("d_dst", c_void_p), ("dst_ld", c_int32),
                 ("d_stats", c_void_p), ("stats_cap", c_size_t), ("d_row_stats", c_void_p), ("row_stats_cap", c_size_t),
                 ("out", c_int32 * 10)])


OP_CHAIN_MAX_LAYERS = 8


class SpdmOpChainArgs(ctypes.Structure):
    """spdm_op_chain_args (include/spdm.h)."""
    _fields_ = [("B", c_int32), ("HW", c_int32), ("n_layers", c_int32), ("chan", c_int32 * (OP_CHAIN_MAX_LAYERS + 1)),
                ("gelu", c_int32 * OP_CHAIN_MAX_LAYERS), ("d_src", c_void_p), ("src_ld", c_int32),
                ("h_weight", c_void_p * OP_CHAIN_MAX_LAYERS), ("d_gamma", c_void_p * OP_CHAIN_MAX_LAYERS),
                ("d_beta", c_void_p * OP_CHAIN_MAX_LAYERS), ("d_dst", c_void_p), ("dst_ld", c_int32),
                ("d_stats", c_void_p), ("stats_cap", c_size_t), ("out", c_int32 * 4)]


# spdm_op_train op codes (include/spdm.h: SPDM_OPT_*), in enum order
OP_TRAIN_OPS = ("wgrad", "wgrad_mapped", "colsum", "gn_stats", "gn_bwd", "film_bwd", "mse", "pool_bwd", "up_bwd", "mish_bwd",
                "ln_fwd", "ln_bwd", "gelu_bwd", "attn_fwd_lse", "attn_bwd", "gn_bwd_mapped", "simple_tail_bwd", "silu_bwd")
OP_TRAIN_DIMS, OP_TRAIN_BUFS, OP_TRAIN_IDX = 10, 8, 2


class SpdmOpTrainArgs(ctypes.Structure):
    """spdm_op_train_args (include/spdm.h)."""
    _fields_ = [("op", c_int32), ("reserved", c_int32), ("dim", c_int64 * OP_TRAIN_DIMS), ("d_buf", c_void_p * OP_TRAIN_BUFS),
                ("cap", c_uint64 * OP_TRAIN_BUFS), ("h_idx", c_void_p * OP_TRAIN_IDX), ("n_idx", c_int64 * OP_TRAIN_IDX),
                ("info", c_int32 * 4)]


# spdm_op_stream op codes (include/spdm.h: SPDM_OPS_*), in enum order
OP_STREAM_OPS = ("conv_in", "pool", "upcat", "film_apply", "film_coef", "layernorm", "mish_pad", "silu_pad", "silu", "dc_finish",
                 "simple_tail", "splitk_combine", "out_step")
OP_STREAM_DIMS, OP_STREAM_BUFS, OP_STREAM_IDX, OP_STREAM_GN = 14, 8, 1, 2


class SpdmOpStreamGn(ctypes.Structure):
    """spdm_op_stream_gn (include/spdm.h)."""
    _fields_ = [("d_stats", c_void_p), ("stats_cap", c_uint64), ("slots", c_int32), ("m_tile", c_int32), ("n_tiles", c_int32),
                ("cnorm", c_int32), ("d_gamma", c_void_p), ("d_beta", c_void_p), ("affine_cap", c_uint64)]


class SpdmOpStreamArgs(ctypes.Structure):
    """spdm_op_stream_args (include/spdm.h)."""
    _fields_ = [("op", c_int32), ("reserved", c_int32), ("dim", c_int64 * OP_STREAM_DIMS), ("d_buf", c_void_p * OP_STREAM_BUFS),
                ("cap", c_uint64 * OP_STREAM_BUFS), ("h_idx", c_void_p * OP_STREAM_IDX), ("n_idx", c_int64 * OP_STREAM_IDX),
                ("gn", SpdmOpStreamGn * OP_STREAM_GN), ("d_stats_out", c_void_p), ("stats_out_cap", c_uint64),
                ("d_words", c_void_p), ("seed", c_uint64), ("first_index", c_uint64), ("bias", c_float), ("info", c_int32 * 4),
                ("reserved2", c_int32)]


# spdm_op_frame op codes (include/spdm.h: SPDM_OPF_*), in enum order
OP_FRAME_OPS = ("enc_convs", "enc_kinks", "enc_x2", "enc_dz3", "enc_dz2", "enc_conv1_wgrad", "add", "dec_convs", "dec_kinks",
                "dec_loss", "dec_bwd6", "dec_dgrad4", "dec_colsum", "dec_unperm_conv", "dec_unperm_linear", "frame_wgrad")
OP_FRAME_DIMS, OP_FRAME_BUFS = 4, 11


class SpdmOpFrameArgs(ctypes.Structure):
    """spdm_op_frame_args (include/spdm.h)."""
    _fields_ = [("op", c_int32), ("reserved", c_int32), ("dim", c_int64 * OP_FRAME_DIMS), ("d_buf", c_void_p * OP_FRAME_BUFS),
                ("cap", c_uint64 * OP_FRAME_BUFS), ("d_sq", c_void_p), ("sq_cap", c_uint64), ("scale", c_float),
                ("info", c_int32 * 4), ("reserved2", c_int32)]


# spdm_op_sa op codes (include/spdm.h: SPDM_OPA_*), in enum order, and the kernels info[0] names
OP_SA_OPS = ("fused64", "qkv", "head", "tail", "core")
OP_SA_KERNELS = ("fused", "fused_pair", "crop", "qkv", "head", "tail", "core_ds", "core_valu", "core_mfma")
OP_SA_DIMS, OP_SA_BUFS, OP_SA_WEIGHTS, OP_SA_VECS = 10, 3, 4, 8


class SpdmOpSaArgs(ctypes.Structure):
    """spdm_op_sa_args (include/spdm.h)."""
    _fields_ = [("op", c_int32), ("reserved", c_int32), ("dim", c_int64 * OP_SA_DIMS), ("d_buf", c_void_p * OP_SA_BUFS),
                ("cap", c_uint64 * OP_SA_BUFS), ("h_w", c_void_p * OP_SA_WEIGHTS), ("d_vec", c_void_p * OP_SA_VECS),
                ("vec_cap", c_uint64 * OP_SA_VECS), ("d_ab", c_void_p), ("ab_cap", c_uint64), ("film_on", c_int32),
                ("t_count", c_int32), ("T", c_int64), ("gn", SpdmOpStreamGn), ("d_temb", c_void_p), ("temb_cap", c_uint64),
                ("h_t", c_void_p), ("d_film", c_void_p), ("film_cap", c_uint64), ("d_outc_w", c_void_p), ("outc_w_cap", c_uint64),
                ("outc_b", c_float), ("info", c_int32 * 5)]


class SpdmOptimSegment(ctypes.Structure):
    """spdm_optim_segment (include/spdm.h)."""
    _fields_ = [("d_param", c_void_p), ("d_grad", c_void_p), ("d_exp_avg", c_void_p), ("d_exp_avg_sq", c_void_p),
                ("numel", c_uint64)]


class SpdmEmaSegment(ctypes.Structure):
    """spdm_ema_segment (include/spdm.h)."""
    _fields_ = [("d_ema", c_void_p), ("d_param", c_void_p), ("numel", c_uint64)]


class SpdmForwardProcessArgs(ctypes.Structure):
    """spdm_forward_process_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("B", "H", "D", "inp_h", "T", "time_dim")] +
                [(n, c_void_p) for n in ("d_x0", "d_inpaint", "d_sqrt_abar", "d_sqrt_1m_abar")] +
                [("seed", c_uint64), ("sample_offset", c_uint64), ("step", ctypes.c_uint32), ("dropout_p", c_float)] +
                [(n, c_void_p) for n in ("d_t_in", "d_noise_in", "d_t", "d_noise", "d_x_noisy", "d_time_scale", "d_clamped")])


class SpdmDatasetGatherArgs(ctypes.Structure):
    """spdm_dataset_gather_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("T", "n_windows", "B", "seq_len", "step_size", "n_frames", "img_dtype", "reserved")] +
                [(n, c_void_p) for n in ("d_img", "d_position", "d_velocity", "d_action", "d_window_start", "h_window_start",
                                         "d_window_id")] +
                [("pos_min", c_double), ("pos_max", c_double)] +
                [(n, c_void_p) for n in ("d_image_out", "d_position_out", "d_velocity_out", "d_action_out", "d_translation_out",
                                         "d_start_out", "d_bad")])


class SpdmEvalErrorsArgs(ctypes.Structure):
    """spdm_eval_errors_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("B", "H", "D", "n_slots", "seq", "obs_h", "inp_h", "P", "runs", "window_base")] +
                [("first_traj", c_int64)] +
                [(n, c_void_p) for n in ("d_pred", "d_truth_pos", "d_truth_act", "d_translation")] +
                [("pos_min", c_double), ("pos_max", c_double), ("act_min", c_double * 3), ("act_max", c_double * 3)] +
                [("d_pos_err", c_void_p), ("d_act_err", c_void_p)])


class SpdmEvalReduceArgs(ctypes.Structure):
    """spdm_eval_reduce_args (include/spdm.h)."""
    _fields_ = ([("N", c_int64), ("C", c_int32), ("runs", c_int32)] +
                [(n, c_void_p) for n in ("d_err", "d_window_mean", "d_window_std", "d_mean", "d_std", "d_workspace")] +
                [("workspace_doubles", c_uint64)])


class SpdmObsNoiseTensor(ctypes.Structure):
    """spdm_obs_noise_tensor (include/spdm.h)."""
    _fields_ = [("d_src", c_void_p), ("d_dst", c_void_p), ("inner", c_int64), ("src_stride", c_int64), ("dst_stride", c_int64)]


class SpdmObsNoiseArgs(ctypes.Structure):
    """spdm_obs_noise_args (include/spdm.h)."""
    _fields_ = [("n_rows", c_int64), ("row_offset", c_int64), ("seed", c_uint64), ("draw", ctypes.c_uint32), ("alpha", c_float),
                ("n_tensors", c_int32), ("reserved", c_int32), ("tensors", SpdmObsNoiseTensor * 4)]


class SpdmPolicyPushArgs(ctypes.Structure):
    """spdm_policy_push_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("E", "L", "img_dtype", "reserved")] + [("n", c_int64)] +
                [(n, c_void_p) for n in ("d_img_in", "d_pos_in", "d_vel_in", "d_act_in", "d_fill", "d_ring_img", "d_ring_pos",
                                         "d_ring_vel", "d_ring_act")])


class SpdmPolicyWindowArgs(ctypes.Structure):
    """spdm_policy_window_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("E", "L", "obs_h", "step_size", "img_dtype", "stats_f32")] + [("n", c_int64)] +
                [(n, c_void_p) for n in ("d_ring_img", "d_ring_pos", "d_ring_vel", "d_ring_act")] +
                [("pos_min", c_double), ("pos_max", c_double), ("vel_min", c_double * 2), ("vel_max", c_double * 2),
                 ("act_min", c_double * 3), ("act_max", c_double * 3)] +
                [(n, c_void_p) for n in ("d_image_out", "d_position_out", "d_velocity_out", "d_action_out", "d_translation_out")])


class SpdmPolicyUnnormalizeArgs(ctypes.Structure):
    """spdm_policy_unnormalize_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("E", "H", "D", "inp_h")] + [("d_x0", c_void_p), ("d_translation", c_void_p)] +
                [("pos_min", c_double), ("pos_max", c_double), ("act_min", c_double * 3), ("act_max", c_double * 3)] +
                [("d_waypoints", c_void_p), ("d_actions", c_void_p)])


class SpdmPolicyWarmStartArgs(ctypes.Structure):
    """spdm_policy_warm_start_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("E", "H", "D", "inp_h", "step_size")] + [("draw", ctypes.c_uint32)] +
                [("delta", c_int64), ("seed", c_uint64), ("env_offset", c_uint64), ("sa", c_float), ("sb", c_float)] +
                [(n, c_void_p) for n in ("d_prev_x0", "d_prev_translation", "d_translation", "d_inpaint", "d_noise_in", "d_x", "d_guess",
                                         "d_noise")])


class SpdmPolicySelectArgs(ctypes.Structure):
    """spdm_policy_select_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("E", "K", "H", "D", "inp_h", "cols", "mode", "rows")] + [("guess_row_stride", c_int64)] +
                [(n, c_void_p) for n in ("d_x0", "d_guess", "d_translation")] + [("pos_min", c_double), ("pos_max", c_double)] +
                [(n, c_void_p) for n in ("d_chosen", "d_x0_out", "d_scores", "d_spread")])


class SpdmSolverStepArgs(ctypes.Structure):
    """spdm_solver_step_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("B", "H", "D", "inp_h", "inpaint_per_sample", "n_steps", "step", "first")] +
                [(n, c_void_p) for n in ("d_eps", "d_x", "d_x0_prev", "d_coef", "d_inpaint", "d_history", "d_words")])


class SpdmLossTermsArgs(ctypes.Structure):
    """spdm_loss_terms_args (include/spdm.h)."""
    _fields_ = ([(n, c_int32) for n in ("B", "H", "D", "reserved")] + [("d_eps", c_void_p), ("d_noise", c_void_p)] +
                [("slot_offset", c_int64), ("n_slots", c_int64)] +
                [(n, c_void_p) for n in ("d_terms", "d_t_in", "d_slot_t")])


class SpdmReconTermsArgs(ctypes.Structure):
    """spdm_recon_terms_args (include/spdm.h)."""
    _fields_ = [("n", c_int32), ("reserved", c_int32), ("d_recon", c_void_p), ("d_target", c_void_p),
                ("slot_offset", c_int64), ("n_slots", c_int64), ("d_terms", c_void_p)]


class SpdmFramesToBytesArgs(ctypes.Structure):
    """spdm_frames_to_bytes_args (include/spdm.h)."""
    _fields_ = [("n", c_int32), ("cols", c_int32), ("tile_offset", c_int64), ("n_tiles", c_int64),
                ("d_frames", c_void_p), ("d_out", c_void_p)]


class SpdmConfig(ctypes.Structure):
    _fields_ = [(n, c_int32) for n in ("horizon", "state_dim", "cond_dim", "time_dim", "attention", "max_batch",
                                        "device", "num_train_timesteps", "flags")]


# every symbol include/spdm.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "spdm_abi_version": (c_int32, []),
    "spdm_last_error": (c_char_p, []),
    "spdm_create": (c_int32, [POINTER(SpdmConfig), POINTER(c_void_p)]),
    "spdm_destroy": (None, [c_void_p]),
    "spdm_load_weights": (c_int32, [c_void_p, c_void_p, c_size_t, POINTER(TensorIndex), c_int32]),
    "spdm_update_weights": (c_int32, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "spdm_debug_weight_digest": (c_int32, [c_void_p, POINTER(c_uint64)]),
    "spdm_set_time_table": (c_int32, [c_void_p, c_void_p, c_int32]),
    "spdm_set_schedule": (c_int32, [c_void_p, c_int32, c_int32, c_int32, c_float, c_float]),
    "spdm_set_schedule_tables": (c_int32, [c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "spdm_schedule_tables": (c_int32, [c_int32, c_int32, c_int32, c_float, c_float, c_void_p, c_void_p]),
    "spdm_unet_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "spdm_unet_forward_dt": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "spdm_sample": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_uint64,
                              c_uint64, c_void_p, c_void_p, c_void_p]),
    "spdm_train_loss_grad": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "spdm_train_loss_grad_dt": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
    "spdm_train_forward_process": (c_int32, [c_int32, POINTER(SpdmForwardProcessArgs), c_void_p]),
    "spdm_dataset_gather": (c_int32, [c_int32, POINTER(SpdmDatasetGatherArgs), c_void_p]),
    "spdm_eval_errors": (c_int32, [c_int32, POINTER(SpdmEvalErrorsArgs), c_void_p]),
    "spdm_eval_reduce": (c_int32, [c_int32, POINTER(SpdmEvalReduceArgs), c_void_p]),
    "spdm_eval_reduce_workspace_doubles": (c_size_t, [c_int64, c_int32]),
    "spdm_obs_noise": (c_int32, [c_int32, POINTER(SpdmObsNoiseArgs), c_void_p]),
    "spdm_policy_push": (c_int32, [c_int32, POINTER(SpdmPolicyPushArgs), c_void_p]),
    "spdm_policy_window": (c_int32, [c_int32, POINTER(SpdmPolicyWindowArgs), c_void_p]),
    "spdm_policy_unnormalize": (c_int32, [c_int32, POINTER(SpdmPolicyUnnormalizeArgs), c_void_p]),
    "spdm_policy_warm_start": (c_int32, [c_int32, POINTER(SpdmPolicyWarmStartArgs), c_void_p]),
    "spdm_policy_select": (c_int32, [c_int32, POINTER(SpdmPolicySelectArgs), c_void_p]),
    "spdm_solver_step": (c_int32, [c_int32, POINTER(SpdmSolverStepArgs), c_void_p]),
    "spdm_loss_terms": (c_int32, [c_int32, POINTER(SpdmLossTermsArgs), c_void_p]),
    "spdm_recon_terms": (c_int32, [c_int32, POINTER(SpdmReconTermsArgs), c_void_p]),
    "spdm_frames_to_bytes": (c_int32, [c_int32, POINTER(SpdmFramesToBytesArgs), c_void_p]),
    "spdm_train_set_time_scale": (c_int32, [c_void_p, c_void_p, c_int32]),
    "spdm_sample_begin": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p,
                                    c_uint64, c_uint64, c_void_p, c_void_p]),
    "spdm_sample_run": (c_int32, [c_void_p, c_int32, c_int32, c_void_p]),
    "spdm_sample_result": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "spdm_graph_captures": (c_int64, [c_void_p]),
    "spdm_debug_tensor": (c_int32, [c_void_p, c_char_p, c_void_p, c_size_t, POINTER(c_int32 * 4)]),
    "spdm_uses_split_precision": (c_int32, [c_void_p]),
    "spdm_demoted_tensors": (c_int32, [c_void_p]),
    "spdm_nonfinite": (c_int32, [c_void_p, POINTER(c_int32), c_void_p]),
    "spdm_set_switch": (c_int32, [c_void_p, c_char_p, c_int32]),
    "spdm_device_bytes": (c_size_t, [c_void_p]),
    "spdm_profile_enable": (c_int32, [c_void_p, c_int32]),
    "spdm_profile_read": (c_int32, [c_void_p, POINTER(c_int64), POINTER(c_double), POINTER(c_double)]),
    "spdm_encoder_create": (c_int32, [c_int32, c_void_p, c_size_t, POINTER(TensorIndex), c_int32, POINTER(c_void_p)]),
    "spdm_encoder_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "spdm_encoder_destroy": (None, [c_void_p]),
    "spdm_encoder_train_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "spdm_encoder_backward": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spdm_encoder_update_weights": (c_int32, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "spdm_decoder_create": (c_int32, [c_int32, c_void_p, c_size_t, POINTER(TensorIndex), c_int32, POINTER(c_void_p)]),
    "spdm_decoder_forward": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "spdm_decoder_train_loss": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spdm_decoder_backward": (c_int32, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "spdm_decoder_update_weights": (c_int32, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "spdm_decoder_destroy": (None, [c_void_p]),
    "spdm_adam_workspace_doubles": (c_size_t, []),
    "spdm_adam_step": (c_int32, [c_int32, POINTER(SpdmOptimSegment), c_int32, c_int64, c_float, c_float, c_float, c_float, c_float,
                                 c_void_p, c_void_p]),
    "spdm_adam_norm_index": (c_size_t, []),
    "spdm_ema_step": (c_int32, [c_int32, POINTER(SpdmEmaSegment), c_int32, c_float, c_void_p]),
    "spdm_op_gelu": (c_int32, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "spdm_op_gemm": (c_int32, [POINTER(SpdmOpGemmArgs)]),
    "spdm_op_chain": (c_int32, [POINTER(SpdmOpChainArgs)]),
    "spdm_op_train": (c_int32, [POINTER(SpdmOpTrainArgs)]),
    "spdm_op_stream": (c_int32, [POINTER(SpdmOpStreamArgs)]),
    "spdm_op_frame": (c_int32, [POINTER(SpdmOpFrameArgs)]),
    "spdm_op_sa": (c_int32, [POINTER(SpdmOpSaArgs)]),
    "spdm_debug_geometry": (c_int32, [c_int32] * 6 + [ctypes.c_uint32, POINTER(c_int32 * 10)]),
    "spdm_debug_whole_tiles": (c_int32, []),
    "spdm_debug_fused_upsample_launches": (c_int32, []),
    "spdm_debug_pooled_epilogue_launches": (c_int32, []),
    "spdm_debug_conv_chain_launches": (c_int32, []),
    "spdm_debug_plan_routes": (c_int32, [c_void_p, c_int32, POINTER(c_int32), c_int32]),
    "spdm_bench_gemm": (c_int32, [c_int32] * 12 + [POINTER(c_double)]),
    "spdm_bench_chain": (c_int32, [c_int32] * 4 + [POINTER(c_int32), c_int32, c_int32, POINTER(c_double)]),   # ms_out[2]: {ms per launch, max|split - fp32|}
}

_lib = None


def load() -> ctypes.CDLL:
    """dlopen the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built "
            "(run `python -m state_policy_diffusionmodel_amd.build`); there is no CPU fallback")
    import torch  # noqa: F401  -- FIRST: the library binds to the HIP runtime instance torch has loaded
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.spdm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"ABI version mismatch: library {lib.spdm_abi_version()}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().spdm_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
