"""ctypes binding of libdm_hip.so (C ABI declared in include/dm_hip.h).

There is no CPU fallback: if the shared library is missing or a call fails the
error is raised, never swallowed.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# DM_LIB selects another build of the same ABI (tools/conv_stamps.py loads the stamped diagnostic build)
LIB_PATH = os.environ.get("DM_LIB") or os.path.join(_HERE, "libdm_hip.so")
DM_MAX_STAGES = 8
DM_COEFS = 8
DM_EDM_COEFS = 16
EDM_HEUN, EDM_DPMPP = 0, 1
DM_CT_COEFS = 16
CT_PRED_NOISE, CT_PRED_V = 0, 1
DM_REPAINT_COEFS = 16
DM_LV_COEFS = 16
DM_LV_TRAIN_COEFS = 12
DM_WO_COEFS = 16
DM_WO_TRAIN_COEFS = 12
DM_CG_COEFS = 16
DM_BPD_COEFS = 16
DM_BPD_CHUNK = 1024
ABI_VERSION = 9
DDIM_NO_CLAMP, DDIM_RAW_NOISE = 1, 2  # DM_DDIM_* of include/dm_hip.h

# every symbol include/dm_hip.h declares (tests check the library exports all of them)
EXPORTS = (
    "dm_last_error", "dm_abi_version",
    "dm_unet_create", "dm_unet_destroy", "dm_unet_set_param", "dm_unet_missing_params", "dm_unet_get_param_host", "dm_unet_finalize",
    "dm_unet_update_param", "dm_unet_refresh", "dm_unet_graph_captures", "dm_unet_workspace_bytes",
    "dm_unet_forward", "dm_unet_forward_masked", "dm_sample", "dm_sample_cond", "dm_sample_ex", "dm_randn",
    "dm_decoder_create", "dm_decoder_destroy", "dm_decoder_set_param", "dm_decoder_missing_params",
    "dm_decoder_finalize", "dm_decoder_forward",
    "dm_encoder_create", "dm_encoder_destroy", "dm_encoder_set_param", "dm_encoder_missing_params",
    "dm_encoder_finalize", "dm_encoder_forward",
    "dm_encoder_forward_kl", "dm_encoder_quantize", "dm_encoder_embed_code",
    "dm_op_conv2d", "dm_op_downsample", "dm_op_rmsnorm", "dm_op_block", "dm_op_linear_attention",
    "dm_op_attention", "dm_op_sampler_update", "dm_op_cfg_combine",
    "dm_op_sampler_update_ex", "dm_op_conv1d", "dm_op_block1d",
    "dm_op_group_norm", "dm_op_vae_attention", "dm_op_vq_nearest",
    "dm_op_vq_nearest_nchw", "dm_op_kl_posterior", "dm_op_embed_code",
    "dm_op_vae_conv", "dm_op_vae_resblock", "dm_op_vae_attn_block",
    "dm_conv_create", "dm_conv_destroy", "dm_conv_forward", "dm_op_pool2d", "dm_op_resize_bilinear",
    "dm_op_copy_channels_nhwc", "dm_op_global_avgpool", "dm_op_linear",
    "dm_unet_train_enable", "dm_unet_grad_floats", "dm_unet_grads_flat", "dm_unet_train_buckets", "dm_unet_train_bucket", "dm_unet_get_grad", "dm_unet_loss_backward", "dm_unet_loss_backward_ex", "dm_unet_loss_backward_masked", "dm_op_q_sample", "dm_op_linear_bwd",
    "dm_op_offset_noise", "dm_op_cdist", "dm_op_gather_rows", "dm_op_lincomb", "dm_op_mask_mix",
    "dm_op_mse_loss", "dm_op_adam_step", "dm_op_ema_lerp",
    "dm_unet_optimizer_step", "dm_unet_train_scalar", "dm_unet_ema_update", "dm_unet_get_param", "dm_unet_set_train_tensor", "dm_unet_adam_step",
    "dm_unet_train_sync", "dm_unet_check_device_pack",
    "dm_unet_train_dropout", "dm_op_dropout_mask",
    "dm_op_conv2d_bwd", "dm_op_downsample_bwd", "dm_op_block_bwd", "dm_op_rmsnorm_bwd", "dm_op_linear_attention_bwd",
    "dm_op_attention_bwd", "dm_op_cross_attention", "dm_op_cross_attention_bwd",
    "dm_op_linear_attention_core_bwd", "dm_op_attention_core_bwd",
    "dm_profile_enable", "dm_profile_read",
    "dm_unet_forward_ft", "dm_sample_edm",
    "dm_op_edm_churn_in", "dm_op_edm_euler", "dm_op_edm_heun", "dm_op_edm_dpmpp", "dm_op_edm_finalize",
    "dm_unet_train_enable_ft", "dm_unet_loss_backward_edm",
    "dm_op_edm_noise_in", "dm_op_edm_loss", "dm_op_sinusoid_ft_bwd",
    "dm_sample_ct", "dm_unet_loss_backward_ct", "dm_op_ct_step", "dm_op_ct_noise_in", "dm_op_ct_loss",
    "dm_unet_loss_backward_ct_ig", "dm_op_conv7_dgrad", "dm_op_sinusoid_ft_tgrad", "dm_op_ct_sched_reduce",
    "dm_sample_ct_dpmpp", "dm_op_ct_dpmpp_step",
    "dm_unet_optimizer_step_ex",
    "dm_sample_repaint", "dm_op_repaint_step",
    "dm_sample_lv", "dm_unet_loss_backward_lv", "dm_op_lv_step", "dm_op_lv_loss",
    "dm_sample_wo", "dm_unet_loss_backward_wo", "dm_op_wo_step", "dm_op_wo_loss",
    "dm_sample_classifier_guided", "dm_op_cg_mean", "dm_op_cg_finish",
    "dm_op_dpmpp_update",
    "dm_sample_ex_dyn", "dm_op_dyn_threshold", "dm_op_sampler_update_dyn", "dm_op_dpmpp_update_dyn",
    "dm_unet_cond_forward", "dm_unet_cond_backward", "dm_op_deferred_reduce",
    "dm_eval_bpd", "dm_op_bpd_step_in", "dm_op_bpd_terms", "dm_op_bpd_prior",
    "dm_kunet_create", "dm_kunet_set_class_labels",
    "dm_op_kunet_pixelnorm", "dm_op_kunet_avgpool2", "dm_op_kunet_bilinear_up2", "dm_op_kunet_act", "dm_op_kunet_attention",
    "dm_op_kunet_head", "dm_op_kunet_input_block", "dm_op_kunet_output_block", "dm_op_kunet_block",
)


class UnetCfg(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("init_dim", C.c_int32), ("out_dim", C.c_int32), ("channels", C.c_int32),
        ("input_channels", C.c_int32), ("n_stages", C.c_int32),
        ("dim_mults", C.c_int32 * DM_MAX_STAGES), ("full_attn", C.c_int32 * DM_MAX_STAGES),
        ("attn_heads", C.c_int32), ("attn_dim_head", C.c_int32),
        ("text_mode", C.c_int32), ("text_emb_dim", C.c_int32), ("sinusoidal_theta", C.c_float),
        ("learned_sinusoidal_dim", C.c_int32), ("attn_heads_stage", C.c_int32 * DM_MAX_STAGES),
        ("seq1d", C.c_int32),
    ]


class KunetCfg(C.Structure):
    """dm_kunet_cfg (include/dm_hip.h)."""
    _fields_ = [
        ("image_size", C.c_int32), ("dim", C.c_int32), ("dim_max", C.c_int32), ("num_classes", C.c_int32),
        ("channels", C.c_int32), ("input_channels", C.c_int32), ("num_downsamples", C.c_int32),
        ("num_blocks_per_stage", C.c_int32), ("n_attn_res", C.c_int32), ("attn_res", C.c_int32 * DM_MAX_STAGES),
        ("fourier_dim", C.c_int32), ("attn_dim_head", C.c_int32),
        ("mp_cat_t", C.c_float), ("mp_add_emb_t", C.c_float), ("attn_res_mp_add_t", C.c_float), ("resnet_mp_add_t", C.c_float),
    ]


class KunetBlockOp(C.Structure):
    """dm_kunet_block_op (include/dm_hip.h): one Encoder / Decoder of KarrasUnet on its own."""
    _fields_ = [
        ("decoder", C.c_int32), ("down", C.c_int32), ("up", C.c_int32), ("skip", C.c_int32), ("attn", C.c_int32),
        ("din", C.c_int32), ("dout", C.c_int32), ("skip_channels", C.c_int32), ("dh", C.c_int32),
        ("mp_cat_t", C.c_float), ("attn_res_mp_add_t", C.c_float), ("resnet_mp_add_t", C.c_float),
        ("x", C.c_void_p), ("skip_x", C.c_void_p), ("emb_scale", C.c_void_p), ("down_w", C.c_void_p), ("w1", C.c_void_p),
        ("w2", C.c_void_p), ("res_w", C.c_void_p), ("mem_kv", C.c_void_p), ("qkv_w", C.c_void_p), ("out_w", C.c_void_p),
        ("out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
    ]


class DecoderCfg(C.Structure):
    _fields_ = [
        ("ch", C.c_int32), ("out_ch", C.c_int32), ("n_levels", C.c_int32), ("ch_mult", C.c_int32 * DM_MAX_STAGES),
        ("num_res_blocks", C.c_int32), ("n_attn_res", C.c_int32), ("attn_resolutions", C.c_int32 * DM_MAX_STAGES),
        ("resolution", C.c_int32), ("z_channels", C.c_int32), ("embed_dim", C.c_int32),
    ]


class EncoderCfg(C.Structure):
    _fields_ = [
        ("ch", C.c_int32), ("in_channels", C.c_int32), ("n_levels", C.c_int32), ("ch_mult", C.c_int32 * DM_MAX_STAGES),
        ("num_res_blocks", C.c_int32), ("n_attn_res", C.c_int32), ("attn_resolutions", C.c_int32 * DM_MAX_STAGES),
        ("resolution", C.c_int32), ("z_channels", C.c_int32), ("embed_dim", C.c_int32), ("n_embed", C.c_int32),
        ("double_z", C.c_int32),
    ]


class SampleArgs(C.Structure):
    """dm_sample_args (include/dm_hip.h)."""
    _fields_ = [
        ("kind", C.c_int32), ("objective", C.c_int32), ("self_condition", C.c_int32), ("n_steps", C.c_int32),
        ("times_host", C.POINTER(C.c_int64)), ("coefs_host", C.POINTER(C.c_float)),
        ("x_T", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("ctx", C.c_void_p), ("ctx_tokens", C.c_int32), ("cond_channels", C.c_int32), ("cond", C.c_void_p),
        ("out", C.c_void_p), ("all_steps", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("unnormalize", C.c_int32), ("use_graph", C.c_int32),
        ("ddim_flags", C.c_int32), ("stream", C.c_void_p),
        ("cfg", C.c_int32), ("cfg_scale", C.c_float), ("cfg_rescaled_phi", C.c_float),
        ("cfg_keep_parallel_frac", C.c_float), ("cfg_remove_parallel", C.c_int32), ("cfg_reserved_", C.c_int32),
    ]


class SampleDynArgs(C.Structure):
    """dm_sample_dyn_args (include/dm_hip.h): dynamic thresholding, behind dm_sample_args in dm_sample_ex_dyn."""
    _fields_ = [("dyn_threshold", C.c_int32), ("dyn_percentile", C.c_float)]


class EdmArgs(C.Structure):
    """dm_edm_args (include/dm_hip.h)."""
    _fields_ = [
        ("kind", C.c_int32), ("n_steps", C.c_int32), ("table_host", C.POINTER(C.c_float)),
        ("x_init", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("out", C.c_void_p), ("sigma_init", C.c_float), ("clamp", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("use_graph", C.c_int32), ("stream", C.c_void_p),
    ]


class EdmTrainArgs(C.Structure):
    """dm_edm_train_args (include/dm_hip.h)."""
    _fields_ = [
        ("images", C.c_void_p), ("noise", C.c_void_p), ("coef_host", C.POINTER(C.c_float)), ("coef_stride", C.c_int32),
        ("loss_scale", C.c_float), ("accumulate", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("loss_out_host", C.POINTER(C.c_float)), ("denoised_out", C.c_void_p), ("stream", C.c_void_p),
    ]


class CtArgs(C.Structure):
    """dm_ct_args (include/dm_hip.h)."""
    _fields_ = [
        ("objective", C.c_int32), ("clip", C.c_int32), ("n_steps", C.c_int32), ("table_host", C.POINTER(C.c_float)),
        ("x_init", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("use_graph", C.c_int32),
        ("stream", C.c_void_p),
    ]


class CtDpmppArgs(C.Structure):
    """dm_ct_dpmpp_args (include/dm_hip.h)."""
    _fields_ = [
        ("objective", C.c_int32), ("clip", C.c_int32), ("n_steps", C.c_int32), ("table_host", C.POINTER(C.c_float)),
        ("x_init", C.c_void_p), ("out", C.c_void_p), ("x_out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("use_graph", C.c_int32), ("stream", C.c_void_p),
    ]


class CtTrainArgs(C.Structure):
    """dm_ct_train_args (include/dm_hip.h)."""
    _fields_ = [
        ("images", C.c_void_p), ("noise", C.c_void_p), ("coef_host", C.POINTER(C.c_float)), ("coef_stride", C.c_int32),
        ("objective", C.c_int32), ("loss_scale", C.c_float), ("accumulate", C.c_int32), ("B", C.c_int32), ("H", C.c_int32),
        ("W", C.c_int32), ("normalize", C.c_int32), ("loss_out_host", C.POINTER(C.c_float)), ("stream", C.c_void_p),
    ]


class CtTrainIgArgs(C.Structure):
    """dm_ct_train_ig_args (include/dm_hip.h): dm_ct_train_args, then the three outputs."""
    _fields_ = CtTrainArgs._fields_ + [
        ("sched_out_host", C.POINTER(C.c_float)), ("dx_out", C.c_void_p), ("dtime_out", C.c_void_p),
    ]


class RepaintArgs(C.Structure):
    """dm_repaint_args (include/dm_hip.h)."""
    _fields_ = [
        ("objective", C.c_int32), ("n_rows", C.c_int32), ("times_host", C.POINTER(C.c_int64)),
        ("table_host", C.POINTER(C.c_float)), ("x_T", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64),
        ("sample_offset", C.c_uint64), ("gt", C.c_void_p), ("mask", C.c_void_p), ("mask_channels", C.c_int32),
        ("unnormalize", C.c_int32), ("out", C.c_void_p), ("all_steps", C.c_void_p), ("n_frames", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("use_graph", C.c_int32), ("stream", C.c_void_p),
    ]


class LvArgs(C.Structure):
    """dm_lv_args (include/dm_hip.h)."""
    _fields_ = [
        ("n_steps", C.c_int32), ("times_host", C.POINTER(C.c_int64)), ("table_host", C.POINTER(C.c_float)),
        ("x_T", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("out", C.c_void_p), ("all_steps", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("unnormalize", C.c_int32), ("use_graph", C.c_int32), ("stream", C.c_void_p),
    ]


class LvTrainArgs(C.Structure):
    """dm_lv_train_args (include/dm_hip.h)."""
    _fields_ = [
        ("x_start", C.c_void_p), ("t_host", C.POINTER(C.c_int64)), ("coef_host", C.POINTER(C.c_float)),
        ("coef_stride", C.c_int32), ("noise", C.c_void_p), ("vb_loss_weight", C.c_float), ("clip_denoised", C.c_int32),
        ("loss_scale", C.c_float), ("accumulate", C.c_int32), ("loss_out_host", C.POINTER(C.c_float)),
        ("model_out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("stream", C.c_void_p),
    ]


class BpdArgs(C.Structure):
    """dm_bpd_args (include/dm_hip.h)."""
    _fields_ = [
        ("learned", C.c_int32), ("objective", C.c_int32), ("clip_denoised", C.c_int32), ("n_steps", C.c_int32),
        ("times_host", C.POINTER(C.c_int64)), ("table_host", C.POINTER(C.c_float)),
        ("x0", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("ctx", C.c_void_p), ("ctx_tokens", C.c_int32), ("cond_channels", C.c_int32), ("cond", C.c_void_p),
        ("prior_sqrt_ac", C.c_float), ("prior_logvar", C.c_float), ("terms_out", C.c_void_p), ("prior_out", C.c_void_p),
        ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("use_graph", C.c_int32), ("stream", C.c_void_p),
    ]


# int (*cond_cb)(void* user, int step, int64_t t) of dm_cguide_args
CondCallback = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64)


class CguideArgs(C.Structure):
    """dm_cguide_args (include/dm_hip.h)."""
    _fields_ = [
        ("objective", C.c_int32), ("self_condition", C.c_int32), ("n_steps", C.c_int32), ("reserved_", C.c_int32),
        ("times_host", C.POINTER(C.c_int64)), ("table_host", C.POINTER(C.c_float)),
        ("x_T", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("mean", C.c_void_p), ("grad", C.c_void_p), ("cond_cb", CondCallback), ("user", C.c_void_p),
        ("out", C.c_void_p), ("all_steps", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("unnormalize", C.c_int32), ("use_graph", C.c_int32), ("reserved2_", C.c_int32), ("stream", C.c_void_p),
    ]


class WoArgs(C.Structure):
    """dm_wo_args (include/dm_hip.h)."""
    _fields_ = [
        ("n_steps", C.c_int32), ("times_host", C.POINTER(C.c_int64)), ("table_host", C.POINTER(C.c_float)),
        ("x_T", C.c_void_p), ("noise", C.c_void_p), ("seed", C.c_uint64), ("sample_offset", C.c_uint64),
        ("out", C.c_void_p), ("all_steps", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
        ("unnormalize", C.c_int32), ("use_graph", C.c_int32), ("stream", C.c_void_p),
    ]


class WoTrainArgs(C.Structure):
    """dm_wo_train_args (include/dm_hip.h)."""
    _fields_ = [
        ("x_start", C.c_void_p), ("t_host", C.POINTER(C.c_int64)), ("coef_host", C.POINTER(C.c_float)),
        ("coef_stride", C.c_int32), ("noise", C.c_void_p), ("pred_noise_loss_weight", C.c_float),
        ("pred_x_start_loss_weight", C.c_float), ("loss_scale", C.c_float), ("accumulate", C.c_int32),
        ("loss_out_host", C.POINTER(C.c_float)), ("model_out", C.c_void_p), ("B", C.c_int32), ("H", C.c_int32),
        ("W", C.c_int32), ("stream", C.c_void_p),
    ]


KL_NCHW, KL_ROWS = 0, 1  # DM_KL_* of dm_op_kl_posterior


OBJECTIVES = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


COND_WALK_INFER, COND_WALK_TRAIN = 0, 1
COND_TIME_INT, COND_TIME_FLOAT, COND_TIME_INT_SHARED, COND_TIME_FLOAT_SHARED = 0, 1, 2, 3
REDUCE_NORM_BWD, REDUCE_COLSUM = 0, 1


class CondBufs(C.Structure):
    """dm_cond_bufs (include/dm_hip.h): the intermediates of the conditioning head, device pointers or None."""
    _fields_ = [(n, C.c_void_p) for n in ("e0", "h1pre", "h1", "temb", "te0pre", "te0", "cat", "tfinal", "tact", "ss")]


class ReduceLayer(C.Structure):
    """dm_reduce_layer (include/dm_hip.h): one layer of dm_op_deferred_reduce."""
    _fields_ = [("kind", C.c_int32), ("C", C.c_int32), ("silu", C.c_int32), ("ss_stride", C.c_int32),
                ("dss_stride", C.c_int32), ("reserved", C.c_int32),
                ("rows", C.c_int64), ("row_stride", C.c_int64), ("col_stride", C.c_int64),
                ("dy", C.c_void_p), ("u", C.c_void_p), ("g", C.c_void_p), ("ss", C.c_void_p), ("x", C.c_void_p),
                ("du", C.c_void_p), ("dg", C.c_void_p), ("dbias", C.c_void_p), ("dss", C.c_void_p), ("out", C.c_void_p)]


class ProfileRow(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("launches", C.c_int64), ("total_ms", C.c_double),
                ("total_flops", C.c_double), ("total_bytes", C.c_double)]


_lib: Optional[C.CDLL] = None


def _declare(lib: C.CDLL) -> None:
    vp, i32, i64, u64, fp = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_void_p
    lib.dm_last_error.restype = C.c_char_p
    lib.dm_last_error.argtypes = []
    lib.dm_abi_version.restype = i32
    lib.dm_unet_create.argtypes = [C.POINTER(UnetCfg), i32, C.POINTER(vp)]
    lib.dm_unet_destroy.argtypes = [vp]
    lib.dm_unet_destroy.restype = None
    lib.dm_unet_set_param.argtypes = [vp, C.c_char_p, fp, C.POINTER(i64), i32]
    lib.dm_unet_missing_params.argtypes = [vp]
    lib.dm_unet_finalize.argtypes = [vp]
    lib.dm_unet_get_param_host.argtypes = [vp, C.c_char_p, vp, i64]
    lib.dm_unet_forward.argtypes = [vp, fp, vp, fp, i32, fp, i32, i32, i32, vp]
    lib.dm_unet_forward_masked.argtypes = [vp, fp, vp, fp, i32, vp, fp, i32, i32, i32, vp]
    lib.dm_unet_update_param.argtypes = [vp, C.c_char_p, fp, C.POINTER(i64), i32]
    lib.dm_unet_refresh.argtypes = [vp]
    lib.dm_unet_graph_captures.argtypes = [vp]
    lib.dm_unet_workspace_bytes.argtypes = [vp]
    lib.dm_unet_workspace_bytes.restype = i64
    lib.dm_sample.argtypes = [vp, i32, i32, C.POINTER(i64), C.POINTER(C.c_float), fp, fp, u64, u64, fp, i32, fp, fp,
                              i32, i32, i32, i32, i32, vp]
    lib.dm_sample_cond.argtypes = [vp, i32, i32, C.POINTER(i64), C.POINTER(C.c_float), fp, fp, u64, u64, fp, i32, fp,
                                   i32, fp, fp, i32, i32, i32, i32, i32, vp]
    lib.dm_sample_ex.argtypes = [vp, C.POINTER(SampleArgs)]
    lib.dm_sample_ex_dyn.argtypes = [vp, C.POINTER(SampleArgs), C.POINTER(SampleDynArgs)]
    lib.dm_randn.argtypes = [fp, i64, u64, u64, u64, vp]
    lib.dm_decoder_create.argtypes = [C.POINTER(DecoderCfg), i32, C.POINTER(vp)]
    lib.dm_decoder_destroy.argtypes = [vp]
    lib.dm_decoder_destroy.restype = None
    lib.dm_decoder_set_param.argtypes = [vp, C.c_char_p, fp, C.POINTER(i64), i32]
    lib.dm_decoder_missing_params.argtypes = [vp]
    lib.dm_decoder_finalize.argtypes = [vp]
    lib.dm_decoder_forward.argtypes = [vp, fp, fp, i32, i32, i32, vp]
    lib.dm_encoder_create.argtypes = [C.POINTER(EncoderCfg), i32, C.POINTER(vp)]
    lib.dm_encoder_destroy.argtypes = [vp]
    lib.dm_encoder_destroy.restype = None
    lib.dm_encoder_set_param.argtypes = [vp, C.c_char_p, fp, C.POINTER(i64), i32]
    lib.dm_encoder_missing_params.argtypes = [vp]
    lib.dm_encoder_finalize.argtypes = [vp]
    lib.dm_encoder_forward.argtypes = [vp, fp, fp, fp, vp, i32, i32, i32, vp]
    lib.dm_encoder_forward_kl.argtypes = [vp, fp, fp, fp, fp, fp, u64, u64, u64, i32, i32, i32, i32, vp]
    lib.dm_encoder_quantize.argtypes = [vp, fp, fp, vp, i32, i32, i32, vp]
    lib.dm_encoder_embed_code.argtypes = [vp, vp, fp, i32, i32, i32, vp]
    lib.dm_op_conv2d.argtypes = [fp, i32, fp, i32, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dm_op_downsample.argtypes = [fp, i32, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_rmsnorm.argtypes = [fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_block.argtypes = [fp, i32, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_linear_attention.argtypes = [fp, fp, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, vp]
    lib.dm_op_attention.argtypes = [fp, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, vp]
    lib.dm_op_sampler_update.argtypes = [i32, i32, fp, fp, fp, C.POINTER(C.c_float), fp, fp, i64, vp]
    lib.dm_op_sampler_update_ex.argtypes = [i32, i32, i32, fp, fp, fp, C.POINTER(C.c_float), fp, fp, i64, vp]
    lib.dm_op_conv1d.argtypes = [fp, i32, fp, i32, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dm_op_block1d.argtypes = [fp, i32, fp, i32, fp, fp, fp, fp, fp, fp, fp, i32, i32, i32, vp]
    lib.dm_op_dpmpp_update.argtypes = [i32, fp, fp, fp, C.POINTER(C.c_float), fp, i64, vp]
    lib.dm_op_dyn_threshold.argtypes = [i32, fp, fp, C.POINTER(C.c_float), i32, i64, C.c_double, fp, vp]
    lib.dm_op_sampler_update_dyn.argtypes = [i32, i32, fp, fp, fp, C.POINTER(C.c_float), fp, i32, i64, fp, fp, vp]
    lib.dm_op_dpmpp_update_dyn.argtypes = [i32, fp, fp, fp, C.POINTER(C.c_float), fp, i32, i64, fp, vp]
    lib.dm_op_cfg_combine.argtypes = [fp, fp, fp, i32, i64, C.c_float, C.c_float, i32, C.c_float, vp]
    lib.dm_op_group_norm.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, C.c_float, i32, vp]
    lib.dm_op_vae_attention.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_vae_conv.argtypes = [fp] * 4 + [i32] * 12 + [vp]
    lib.dm_op_vae_resblock.argtypes = [fp] * 12 + [i32] * 5 + [vp]
    lib.dm_op_vae_attn_block.argtypes = [fp] * 12 + [i32] * 4 + [vp]
    lib.dm_op_vq_nearest.argtypes = [fp, fp, fp, vp, i64, i32, i32, i32, vp]
    lib.dm_op_vq_nearest_nchw.argtypes = [fp, fp, fp, vp, i64, i32, i32, i32, vp]
    lib.dm_op_kl_posterior.argtypes = [fp, i32, fp, u64, u64, u64, i32, fp, fp, fp, i32, i32, i32, vp]
    lib.dm_op_embed_code.argtypes = [vp, i32, fp, fp, i64, i32, i32, i32, vp]
    lib.dm_conv_create.argtypes = [fp, fp, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    lib.dm_conv_destroy.argtypes = [vp]
    lib.dm_conv_destroy.restype = None
    lib.dm_conv_forward.argtypes = [vp, fp, i32, i32, i32, i32, fp, vp]
    lib.dm_op_pool2d.argtypes = [fp, fp, i32, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dm_op_resize_bilinear.argtypes = [fp, fp, i32, i32, i32, i32, i32, i32, fp, fp, vp]
    lib.dm_op_copy_channels_nhwc.argtypes = [fp, i32, fp, i32, i32, i64, vp]
    lib.dm_op_global_avgpool.argtypes = [fp, fp, i32, i32, i32, vp]
    lib.dm_op_linear.argtypes = [fp, fp, fp, fp, i32, i32, i32, vp]
    lib.dm_unet_train_enable.argtypes = [vp]
    lib.dm_unet_grad_floats.argtypes = [vp]
    lib.dm_unet_grad_floats.restype = i64
    lib.dm_unet_get_grad.argtypes = [vp, C.c_char_p, fp, vp]
    lib.dm_unet_grads_flat.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    lib.dm_unet_train_buckets.argtypes = [vp, i32]
    lib.dm_unet_train_bucket.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64), i32, vp]
    lib.dm_unet_loss_backward.argtypes = [vp, fp, C.POINTER(i64), C.POINTER(C.c_float), fp, fp, fp, i32, fp, i32, i32, i32,
                                          C.c_float, i32, C.POINTER(C.c_float), fp, i32, i32, i32, vp]
    lib.dm_unet_loss_backward_ex.argtypes = [vp, C.POINTER(TrainArgs)]
    lib.dm_unet_loss_backward_masked.argtypes = [vp, C.POINTER(TrainArgs), C.POINTER(C.c_int32)]
    lib.dm_unet_optimizer_step.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, C.POINTER(C.c_float), vp]
    lib.dm_unet_train_scalar.argtypes = [vp, i32, fp, vp]
    lib.dm_unet_ema_update.argtypes = [vp, C.c_double, i32, vp]
    lib.dm_unet_get_param.argtypes = [vp, C.c_char_p, i32, fp, vp]
    lib.dm_unet_set_train_tensor.argtypes = [vp, C.c_char_p, i32, fp, vp]
    lib.dm_unet_adam_step.argtypes = [vp, C.c_longlong]
    lib.dm_unet_adam_step.restype = C.c_longlong
    lib.dm_unet_train_sync.argtypes = [vp]
    lib.dm_unet_train_dropout.argtypes = [vp, C.c_float, u64]
    lib.dm_op_dropout_mask.argtypes = [fp, i64, C.c_float, u64, u64, i32, vp]
    lib.dm_unet_check_device_pack.argtypes = [vp]
    lib.dm_op_q_sample.argtypes = [fp, fp, C.POINTER(C.c_float), fp, i32, i32, vp]
    lib.dm_op_offset_noise.argtypes = [fp, fp, C.c_float, i32, i32, vp]
    lib.dm_op_lincomb.argtypes = [fp, fp, C.POINTER(C.c_float), fp, i32, i64, i32, i32, vp]
    lib.dm_op_mask_mix.argtypes = [fp, fp, fp, fp, i64, vp]
    lib.dm_op_cdist.argtypes = [fp, fp, fp, i32, i32, i64, vp]
    lib.dm_op_gather_rows.argtypes = [fp, C.POINTER(i64), fp, i32, i64, vp]
    lib.dm_op_mse_loss.argtypes = [fp, fp, fp, fp, C.POINTER(C.c_float), i32, i32, C.c_float, C.c_float, fp, C.POINTER(C.c_float),
                                   fp, fp, i32, i32, vp]
    lib.dm_op_adam_step.argtypes = [fp, fp, fp, fp, i64, C.c_double, C.c_double, C.c_double, C.c_double, i32, C.c_float,
                                    C.POINTER(C.c_float), vp]
    lib.dm_op_ema_lerp.argtypes = [fp, fp, i64, C.c_double, vp]
    lib.dm_op_linear_bwd.argtypes = [fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_conv2d_bwd.argtypes = [fp, i32, fp, i32, fp, fp, fp, fp, fp, fp, i32, i32, i32, i32, i32, i32, i32, vp]
    lib.dm_op_downsample_bwd.argtypes = [fp, i32, fp, fp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_block_bwd.argtypes = [fp, i32] + [fp] * 12 + [i32, i32, i32, i32, vp]
    lib.dm_op_rmsnorm_bwd.argtypes = [fp, fp, fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_linear_attention_bwd.argtypes = [fp] * 15 + [i32] * 6 + [vp]
    lib.dm_op_attention_bwd.argtypes = [fp] * 13 + [i32] * 6 + [vp]
    lib.dm_op_linear_attention_core_bwd.argtypes = [fp] * 9 + [i32] * 4 + [vp]
    lib.dm_op_attention_core_bwd.argtypes = [fp] * 7 + [i32] * 4 + [vp]
    lib.dm_op_cross_attention.argtypes = [fp] * 8 + [vp, fp] + [i32] * 7 + [vp]
    lib.dm_op_cross_attention_bwd.argtypes = [fp] * 8 + [vp] + [fp] * 9 + [i32] * 7 + [vp]
    lib.dm_profile_enable.argtypes = [i32]
    lib.dm_unet_forward_ft.argtypes = [vp, fp, fp, fp, i32, fp, i32, i32, i32, vp]
    lib.dm_sample_edm.argtypes = [vp, C.POINTER(EdmArgs)]
    lib.dm_op_edm_churn_in.argtypes = [fp, fp, C.POINTER(C.c_float), i32, u64, u64, u64, fp, fp, i32, i64, vp]
    lib.dm_op_edm_euler.argtypes = [fp, fp, C.POINTER(C.c_float), i32, i32, fp, fp, fp, fp, i32, i64, vp]
    lib.dm_op_edm_heun.argtypes = [fp, fp, fp, fp, C.POINTER(C.c_float), i32, i32, fp, i32, i64, vp]
    lib.dm_op_edm_dpmpp.argtypes = [fp, fp, fp, C.POINTER(C.c_float), i32, fp, i32, i64, vp]
    lib.dm_op_edm_finalize.argtypes = [fp, fp, i64, vp]
    lib.dm_unet_train_enable_ft.argtypes = [vp, i32]
    lib.dm_unet_loss_backward_edm.argtypes = [vp, C.POINTER(EdmTrainArgs)]
    lib.dm_op_edm_noise_in.argtypes = [fp, fp, C.POINTER(C.c_float), i32, fp, fp, fp, i32, i64, vp]
    lib.dm_op_edm_loss.argtypes = [fp, fp, fp, C.POINTER(C.c_float), C.c_float, fp, fp, C.POINTER(C.c_float), i32, i64, vp]
    lib.dm_op_sinusoid_ft_bwd.argtypes = [fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_sample_ct.argtypes = [vp, C.POINTER(CtArgs)]
    lib.dm_sample_ct_dpmpp.argtypes = [vp, C.POINTER(CtDpmppArgs)]
    lib.dm_op_ct_dpmpp_step.argtypes = [fp, fp, fp, C.POINTER(C.c_float), i32, i32, i32, fp, i32, i64, vp]
    lib.dm_unet_loss_backward_ct.argtypes = [vp, C.POINTER(CtTrainArgs)]
    lib.dm_op_ct_step.argtypes = [fp, fp, fp, C.POINTER(C.c_float), i32, i32, i32, u64, u64, u64, fp, fp, i32, i64, vp]
    lib.dm_op_ct_noise_in.argtypes = [fp, fp, C.POINTER(C.c_float), i32, i32, i32, fp, fp, i32, i64, vp]
    lib.dm_op_ct_loss.argtypes = [fp, fp, C.POINTER(C.c_float), C.c_float, fp, C.POINTER(C.c_float), i32, i64, vp]
    lib.dm_unet_loss_backward_ct_ig.argtypes = [vp, C.POINTER(CtTrainIgArgs)]
    lib.dm_op_conv7_dgrad.argtypes = [fp, fp, fp, i32, i32, i32, i32, i32, vp]
    lib.dm_op_sinusoid_ft_tgrad.argtypes = [fp, fp, fp, fp, i32, i32, vp]
    lib.dm_op_ct_sched_reduce.argtypes = [fp, fp, fp, fp, fp, fp, i32, fp, i32, i64, vp]
    lib.dm_unet_optimizer_step_ex.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float,
                                              C.POINTER(C.c_float), vp]
    lib.dm_sample_repaint.argtypes = [vp, C.POINTER(RepaintArgs)]
    lib.dm_op_repaint_step.argtypes = [i32, i32, fp, fp, fp, fp, i32, fp, fp, fp, C.POINTER(C.c_float), i32, u64, u64, u64, fp, fp,
                                       i32, i32, i32, vp]
    lib.dm_sample_lv.argtypes = [vp, C.POINTER(LvArgs)]
    lib.dm_unet_loss_backward_lv.argtypes = [vp, C.POINTER(LvTrainArgs)]
    lib.dm_op_lv_step.argtypes = [fp, fp, fp, C.POINTER(C.c_float), u64, u64, u64, fp, fp, fp, fp, i32, i64, vp]
    lib.dm_op_lv_loss.argtypes = [fp, fp, fp, fp, C.POINTER(C.c_float), C.c_float, i32, C.c_float, fp, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), i32, i64, vp]
    lib.dm_sample_classifier_guided.argtypes = [vp, C.POINTER(CguideArgs)]
    lib.dm_op_cg_mean.argtypes = [fp, fp, C.POINTER(C.c_float), i32, fp, fp, i32, i64, vp]
    lib.dm_op_cg_finish.argtypes = [fp, fp, fp, C.POINTER(C.c_float), u64, u64, u64, fp, fp, i32, i64, vp]
    lib.dm_sample_wo.argtypes = [vp, C.POINTER(WoArgs)]
    lib.dm_unet_loss_backward_wo.argtypes = [vp, C.POINTER(WoTrainArgs)]
    lib.dm_op_wo_step.argtypes = [fp, fp, fp, C.POINTER(C.c_float), i32, u64, u64, u64, fp, fp, fp, i32, i32, i64, vp]
    lib.dm_op_wo_loss.argtypes = [fp, fp, fp, fp, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float, fp, C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), i32, i32, i64, vp]
    lib.dm_eval_bpd.argtypes = [vp, C.POINTER(BpdArgs)]
    lib.dm_op_bpd_step_in.argtypes = [fp, fp, C.POINTER(C.c_float), u64, u64, u64, fp, i32, i64, vp]
    lib.dm_op_bpd_terms.argtypes = [fp, fp, fp, fp, C.POINTER(C.c_float), i32, i32, i32, C.POINTER(C.c_float), i32, i64, vp]
    lib.dm_op_bpd_prior.argtypes = [fp, C.c_float, C.c_float, fp, i32, i64, vp]
    lib.dm_profile_read.argtypes = [C.POINTER(ProfileRow), i32, C.POINTER(i32)]
    lib.dm_unet_cond_forward.argtypes = [vp, i32, i32, vp, fp, vp, C.POINTER(CondBufs), i32, vp]
    lib.dm_unet_cond_backward.argtypes = [vp, C.POINTER(CondBufs), fp, vp, fp, fp, i32, i32, vp]
    lib.dm_op_deferred_reduce.argtypes = [C.POINTER(ReduceLayer), i32, i32, i32, i32, vp]
    lib.dm_kunet_create.argtypes = [C.POINTER(KunetCfg), i32, C.POINTER(vp)]
    lib.dm_kunet_set_class_labels.argtypes = [vp, fp, i32]
    lib.dm_op_kunet_pixelnorm.argtypes = [fp, fp, fp, i64, i32, C.c_float, vp]
    lib.dm_op_kunet_avgpool2.argtypes = [fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_kunet_bilinear_up2.argtypes = [fp, fp, fp, fp, i32, i32, i32, i32, C.c_float, vp]
    lib.dm_op_kunet_act.argtypes = [fp, i32, C.c_float, fp, i32, C.c_float, fp, fp, C.c_float, i64, vp]
    lib.dm_op_kunet_attention.argtypes = [fp, fp, fp, i32, i32, i32, i32, vp]
    lib.dm_op_kunet_head.argtypes = [fp, fp, fp, fp, fp, fp, C.POINTER(C.c_int32), C.POINTER(C.c_float), i32, i32, i32, i32,
                                     C.c_float, fp, i32, vp]
    lib.dm_op_kunet_input_block.argtypes = [fp, fp, fp, i32, i32, i32, i32, i32, vp]
    lib.dm_op_kunet_output_block.argtypes = [fp, fp, C.c_float, fp, i32, i32, i32, i32, i32, vp]
    lib.dm_op_kunet_block.argtypes = [C.POINTER(KunetBlockOp), vp]


class TrainArgs(C.Structure):
    """``dm_train_args`` of include/dm_hip.h (dm_unet_loss_backward_ex)."""
    _fields_ = [("x_start", C.c_void_p), ("t_host", C.POINTER(C.c_int64)), ("coef_host", C.POINTER(C.c_float)),
                ("coef_stride", C.c_int), ("noise", C.c_void_p), ("noise_q", C.c_void_p), ("cond", C.c_void_p),
                ("cond_channels", C.c_int), ("ctx", C.c_void_p), ("ctx_tokens", C.c_int), ("self_cond", C.c_int),
                ("objective", C.c_int), ("loss_scale", C.c_float), ("accumulate", C.c_int),
                ("loss_out_host", C.POINTER(C.c_float)), ("model_out", C.c_void_p), ("B", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("stream", C.c_void_p), ("loss_terms", C.c_int), ("kl_scale", C.c_float)]


def load() -> C.CDLL:
    """Load libdm_hip.so; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C diffusion-models_amd/csrc`). "
            "There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    _declare(lib)
    if lib.dm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libdm_hip.so ABI {lib.dm_abi_version()} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def profile_enable(on: bool, detail: bool = False) -> None:
    """detail: one row per layer shape (the row names its shape, epilogue and K split) instead of one per kernel instance."""
    check(load().dm_profile_enable((2 if detail else 1) if on else 0))


def profile_read():
    """[{kernel, launches, total_ms, total_flops, total_bytes}] since the last read (synchronises)."""
    rows = (ProfileRow * 64)()
    n = C.c_int(0)
    check(load().dm_profile_read(rows, 64, C.byref(n)))
    return [dict(kernel=rows[i].kernel.decode(), launches=int(rows[i].launches), total_ms=float(rows[i].total_ms),
                 total_flops=float(rows[i].total_flops), total_bytes=float(rows[i].total_bytes))
            for i in range(n.value)]


def check(rc: int) -> None:
    if rc != 0:
        msg = load().dm_last_error().decode(errors="replace")
        raise RuntimeError(f"libdm_hip: {msg}")


def ptr(t) -> Optional[int]:
    """Device (or host) address of a contiguous fp32 / int64 torch tensor, None passes NULL."""
    if t is None:
        return None
    assert t.is_contiguous(), "tensor must be contiguous at the C ABI"
    return t.data_ptr()


def fptr(t):
    """``const float*`` of a contiguous fp32 host tensor (the step and coefficient tables)."""
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def default_seed() -> int:
    """A Philox key from torch's global CPU generator (reproducible under torch.manual_seed)."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def randn(lib, device, shape, seed, draw, sample_offset=0):
    """``dm_randn``: draw ``draw`` of the Philox stream ``seed`` as a ``shape`` tensor on ``device``; ``sample_offset`` is the
    index of the first sample in a global batch."""
    out = torch.empty(tuple(shape), device=device, dtype=torch.float32)
    per_sample = out.numel() // max(int(shape[0]), 1)
    check(lib.dm_randn(ptr(out), out.numel(), C.c_uint64(seed), C.c_uint64(draw),
                       C.c_uint64(int(sample_offset) * per_sample), torch.cuda.current_stream(device).cuda_stream))
    return out
