"""ctypes binding of libvqae_hip.so (include/vqae_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or a call fails, this module
raises.  Error codes are mapped back to the exception types the reference raises for the same
conditions (SURVEY.md §8b "Error conventions").
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# VQAE_HIP_LIB: developer override to time an alternative build of the same library (kernel experiments)
LIB_PATH = os.environ.get("VQAE_HIP_LIB") or os.path.join(_HERE, "libvqae_hip.so")

# enums of vqae_hip.h
LAYOUT_NHWC, LAYOUT_NCHW = 0, 1
IDX_I64, IDX_U8, IDX_U16, IDX_I32 = 0, 1, 2, 3
PAD_NONE, PAD_CIRCULAR, PAD_ZEROS = 0, 1, 2
PRE_NONE, PRE_BIAS, PRE_BIAS_ELU_BIAS, PRE_CHANNEL_GATE = 0, 1, 2, 3
ACT_NONE, ACT_ELU, ACT_SILU = 0, 1, 2
DW_SAME, DW_DOWN, DW_UP = 0, 1, 2
MBT_ROWS, MBT_FIN_LANES = 256, 64       # VQAE_MBT_ROWS, VQAE_MBT_FIN_LANES: the reduction geometry of csrc/mbconv_train.hip
BLOCK_FIXUP, BLOCK_MBCONV = 0, 1
DT_F32, DT_BF16, DT_F16 = 0, 1, 2
MAX_PIXEL_LEVEL = 6                     # VQAE_MAX_PIXEL_LEVEL: overview levels 0 .. 6 (vqae_pixels_u8_level)
# VQAE_METRIC_*: columns of the vqae_recon_metrics_f32 output rows
METRIC_NAMES = ("mse", "huber", "psnr", "ssim", "pred_min", "pred_max", "target_min", "target_max")
# VQAE_CLS_*: columns of the vqae_classifier_forward stats rows
CLS_STATS_NAMES = ("tp", "fp", "fn", "tn", "n_valid", "loss_sum")
# VQAE_CE_*: a cross-entropy stats row is 16 confusion counts at [label * 4 + prediction], then these four columns
CE_STATS_K, CE_WEIGHT_SUM, CE_NLL_SUM, CE_SMOOTH_SUM, CE_N_BAD = 20, 16, 17, 18, 19
DTYPES = {"f32": DT_F32, "fp32": DT_F32, "float32": DT_F32, "bf16": DT_BF16, "bfloat16": DT_BF16,
          "f16": DT_F16, "fp16": DT_F16, "float16": DT_F16, "half": DT_F16}


def dtype_code(dt):
    """'bf16' / torch.bfloat16 / None ... -> VQAE_DT_* (autocast semantics, see include/vqae_hip.h)."""
    if dt is None:
        return DT_F32
    if isinstance(dt, int):
        return dt
    name = str(dt).replace("torch.", "")
    try:
        return DTYPES[name]
    except KeyError:
        raise AssertionError(f"unsupported compute dtype {dt}")


class VqaeHipError(RuntimeError):
    pass


class ConvArgs(Structure):
    _fields_ = [("batch", c_int), ("in_h", c_int), ("in_w", c_int), ("cin", c_int), ("cout", c_int),
                ("ksize", c_int), ("stride", c_int), ("pad", c_int), ("pad_mode", c_int),
                ("pre_mode", c_int), ("pre_a", c_float), ("pre_b", c_float),
                ("has_scale", c_int), ("has_bias_s", c_int), ("has_act", c_int),
                ("scale", c_float), ("bias_s", c_float), ("act_a", c_float), ("act_b", c_float), ("dtype", c_int)]


class Config(Structure):
    _fields_ = [("in_channels", c_int), ("stem", c_int), ("n_down", c_int), ("n_pre", c_int), ("n_post", c_int),
                ("n_enc", c_int), ("num_embeddings", c_int), ("projection_dim", c_int),
                ("commitment_cost", c_float), ("compute_dtype", c_int),
                ("block_kind", c_int), ("expand_ratio", c_int), ("se_divisor", c_int), ("bn_eps", c_float)]


class Tensor(Structure):
    _fields_ = [("name", c_char_p), ("data", c_void_p), ("numel", c_int64)]


OPTIM_KINDS = {"adam": 0, "adamw": 1, "lamb": 2}          # VQAE_OPTIM_*
OPTIM_CHUNK, OPTIM_SMALL = 4096, 64                       # VQAE_OPTIM_CHUNK, VQAE_OPTIM_SMALL (vqae_optim_step's work split)


class ClassifierOptimConfig(Structure):
    _fields_ = [("kind", c_int), ("lr", c_double), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("weight_decay", c_double), ("sam_rho", c_double), ("sam_adaptive", c_int)]


# name -> (restype, argtypes); every symbol include/vqae_hip.h declares
SYMBOLS = {
    "vqae_last_error": (c_char_p, []),
    "vqae_build_info": (c_char_p, []),
    "vqae_vq_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "vqae_vq_forward_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_vq_forward_p_f32": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_vq_projected_workspace_bytes": (c_size_t, [c_int64]),
    "vqae_vq_projected_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                      c_float, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_vq_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int64, c_int, c_void_p, c_void_p]),
    "vqae_vq_projected_backward_workspace_bytes": (c_size_t, [c_int64, c_int]),
    "vqae_vq_projected_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                               c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p]),
    "vqae_embed_code_f32": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "vqae_vq_code_stats_f32": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vqae_vq_ema_update_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_double, c_double,
                                       c_void_p, c_void_p]),
    "vqae_conv_packed_floats": (c_size_t, [c_int, c_int, c_int]),
    "vqae_conv_pack_weight_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_conv2d_f32": (c_int, [POINTER(ConvArgs), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_conv2d_gated_f32": (c_int, [POINTER(ConvArgs), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p]),
    "vqae_dw_partial_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "vqae_dwconv_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                c_void_p, c_void_p]),
    "vqae_se_gate_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "vqae_pixel_shuffle2_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_fixup_same_supported": (c_int, [c_int, c_int, c_int]),
    "vqae_fixup_same_block_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                          POINTER(c_float), c_int, c_void_p]),
    "vqae_round_inplace_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p]),
    "vqae_conv3x3_direct_f32": (c_int, [c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), c_void_p, c_void_p,
                                        c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "vqae_bicubic_up2_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "vqae_nchw_to_nhwc_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_nhwc_to_nchw_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_label_maxpool_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_stitch_tiles": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                  c_void_p]),
    "vqae_unstitch_tiles": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                    c_void_p]),
    "vqae_pixels_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, POINTER(c_float), POINTER(c_float), c_void_p,
                               c_int, c_int, c_void_p]),
    "vqae_pixels_u8_level": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, POINTER(c_float), POINTER(c_float),
                                     c_void_p, c_int, c_int, c_void_p]),
    "vqae_cut_pixels_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                   c_void_p]),
    "vqae_pool_labels_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "vqae_create": (c_int, [POINTER(Config), POINTER(Tensor), c_int, POINTER(c_void_p)]),
    "vqae_destroy": (None, [c_void_p]),
    "vqae_reserve": (c_int, [c_void_p, c_int, c_int, c_int]),
    "vqae_set_codebook": (c_int, [c_void_p, c_void_p]),
    "vqae_encode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p,
                            c_void_p]),
    "vqae_encode_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p,
                               c_void_p]),
    "vqae_encode_features": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_decode": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_decode_indices": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_decode_indices_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                       c_void_p]),
    "vqae_decode_indices_u8_levels": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_int),
                                              POINTER(c_void_p), POINTER(c_int), POINTER(c_int), c_void_p]),
    "vqae_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p,
                             c_void_p]),
    "vqae_block_count": (c_int, [c_void_p, c_int]),
    "vqae_run_blocks": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, POINTER(c_int),
                                POINTER(c_int), c_void_p]),
    "vqae_block_route": (c_char_p, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "vqae_recon_metrics_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "vqae_recon_metrics_f32": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), c_int, c_int, c_int,
                                       c_int, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(Tensor), c_int, POINTER(c_void_p)]),
    "vqae_classifier_destroy": (None, [c_void_p]),
    "vqae_classifier_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "vqae_classifier_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_float,
                                        c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_update": (c_int, [c_void_p, POINTER(Tensor), c_int]),
    "vqae_classifier_grad_floats": (c_size_t, [c_void_p]),
    "vqae_classifier_train_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "vqae_classifier_loss_grad": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_int,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_optim_create": (c_int, [c_void_p, POINTER(ClassifierOptimConfig), POINTER(c_void_p)]),
    "vqae_classifier_optim_destroy": (None, [c_void_p]),
    "vqae_classifier_optim_set": (c_int, [c_void_p, POINTER(ClassifierOptimConfig)]),
    "vqae_classifier_optim_step": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_optim_sam_first": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_download": (c_int, [c_void_p, POINTER(c_void_p), c_void_p]),
    "vqae_classifier_image_floats": (c_size_t, [c_void_p]),
    "vqae_classifier_image": (c_int, [c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_optim_export": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p]),
    "vqae_classifier_optim_import": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "vqae_classifier_ce_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "vqae_classifier_forward_ce": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                           POINTER(c_float), c_float, c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_ce_train_workspace_bytes": (c_size_t, [c_void_p, c_int, c_int, c_int]),
    "vqae_classifier_loss_grad_ce": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, POINTER(c_float), c_float,
                                             c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_classifier_optim_create_ce": (c_int, [c_void_p, POINTER(ClassifierOptimConfig), POINTER(c_void_p)]),
    "vqae_optim_create": (c_int, [c_int, POINTER(c_int64), POINTER(c_int), c_int, POINTER(ClassifierOptimConfig),
                                  POINTER(c_void_p)]),
    "vqae_optim_destroy": (None, [c_void_p]),
    "vqae_optim_set": (c_int, [c_void_p, POINTER(ClassifierOptimConfig)]),
    "vqae_optim_step": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "vqae_optim_sam_first": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_void_p]),
    "vqae_optim_export": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p]),
    "vqae_optim_import": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_int64), c_void_p]),
    "vqae_fixup_train_workspace_bytes": (c_size_t, [c_int64]),
    "vqae_fixup_act_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_fixup_act_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_fixup_out_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "vqae_fixup_out_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p]),
    # x x_dt a b act halo batch h w c y y_dt stream
    "vqae_fixup_act_io": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int,
                                  c_void_p]),
    # g g_dt x x_dt a act halo batch h w c g_x g_a g_b ws stream
    "vqae_fixup_act_backward_io": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    # t t_dt skip skip_dt scale bias4 bias1d n y y_dt stream
    "vqae_fixup_out_io": (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int,
                                  c_void_p]),
    # g t t_dt scale n g_t g_skip skip_dt g_scale g_bias4 g_bias1d ws stream
    "vqae_fixup_out_backward_io": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_bicubic_up2_bias_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "vqae_bicubic_up2_backward_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_up_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    # t_low a b batch h w c y stream
    "vqae_up2_act_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    # g t_low a batch h w c g_t_low g_a g_b ws stream
    "vqae_up2_act_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
    # t s_low scale bias4 bias1d batch h w c y stream
    "vqae_fixup_out_up_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p]),
    # g t scale batch h w c g_t g_s_low g_scale g_bias4 g_bias1d ws stream
    "vqae_fixup_out_up_backward_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "vqae_bn_act_train_supported": (c_int, [c_int]),
    "vqae_bn_act_train_workspace_bytes": (c_size_t, [c_int, c_int64, c_int]),
    # x gamma beta running_mean running_var training momentum eps act batch hw c y mean invstd pool ws stream
    "vqae_bn_act_train_forward_f32": (c_int, [c_void_p] * 5 + [c_int, c_double, c_double, c_int, c_int, c_int64, c_int]
                                      + [c_void_p] * 6),
    # g x mean invstd gamma beta g_pool training act batch hw c g_x g_beta_gamma ws stream
    "vqae_bn_act_train_backward_f32": (c_int, [c_void_p] * 7 + [c_int, c_int, c_int, c_int64, c_int] + [c_void_p] * 4),
    "vqae_dwconv_train_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "vqae_dwconv_train_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "vqae_dwconv_train_forward_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "vqae_dwconv_train_backward_f32": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 4),
    "vqae_se_scale_workspace_bytes": (c_size_t, [c_int, c_int64, c_int]),
    "vqae_se_scale_forward_f32": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "vqae_se_scale_backward_f32": (c_int, [c_void_p] * 3 + [c_int, c_int64, c_int] + [c_void_p] * 4),
    # the _f32 argument lists with the dtype code(s) in front of the stream (csrc/mbconv_train_io.hip)
    "vqae_bn_act_train_forward_io": (c_int, [c_void_p] * 5 + [c_int, c_double, c_double, c_int, c_int, c_int64, c_int]
                                     + [c_void_p] * 5 + [c_int, c_void_p]),
    "vqae_bn_act_train_backward_io": (c_int, [c_void_p] * 7 + [c_int, c_int, c_int, c_int64, c_int] + [c_void_p] * 3
                                      + [c_int, c_void_p]),
    "vqae_dwconv_train_forward_io": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "vqae_dwconv_train_backward_io": (c_int, [c_void_p] * 3 + [c_int] * 5 + [c_void_p] * 3 + [c_int, c_void_p]),
    "vqae_se_scale_forward_io": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_int, c_void_p]),
    "vqae_se_scale_backward_io": (c_int, [c_void_p] * 3 + [c_int, c_int64, c_int] + [c_void_p] * 3 + [c_int, c_int, c_void_p]),
    "vqae_code_histogram_workspace_bytes": (c_size_t, [c_int, c_int64, c_int, c_int]),
    "vqae_code_histogram": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "vqae_flops_per_patch": (c_double, [c_void_p, c_int, c_int, c_int, c_int]),
    "vqae_prof_begin": (c_int, [c_int, c_int]),
    "vqae_prof_end": (c_int, [POINTER(c_double), POINTER(c_int), POINTER(c_double)]),
}

# The trainable convs of csrc/conv_train.hip and csrc/conv_train_thin.hip: node -> (ABI stem, kernel size, stride, image, bias).
# image: the node is called with (batch, h, w), a weight layout and a forward workspace; without it, with its rows M as given
# and a [Co, Ci] weight.  bias: the forward takes a bias [Co] (or NULL) behind w, the backward writes g_bias behind g_b.
CONV_TRAIN = {"conv1x1": ("vqae_conv1x1_train", 1, 1, False, False), "conv_down": ("vqae_conv_down_train", 2, 2, True, False),
              "conv3x3": ("vqae_conv3x3_train", 3, 1, True, False), "conv3x3z": ("vqae_conv3x3z_train", 3, 1, True, True)}
for _stem, _, _, _image, _bias in CONV_TRAIN.values():
    _geo, _lay = ([c_int64, c_int, c_int], [c_int]) if _image else ([c_int64], [])
    _b = [c_void_p] if _bias else []
    SYMBOLS.update({
        _stem + "_supported": (c_int, [c_int, c_int]),
        _stem + "_wgrad_run": (c_int, []),
        _stem + "_workspace_bytes": (c_size_t, _geo + [c_int, c_int]),
        # x a b pre w [bias] [w_layout] geometry cin cout y [ws] stream
        # g x a b pre w [w_layout] geometry cin cout g_x g_w g_a g_b [g_bias] ws stream
        _stem + "_forward_f32": (c_int, [c_void_p] * 3 + [c_int, c_void_p] + _b + _lay + _geo + [c_int, c_int]
                                 + [c_void_p] * (3 if _image else 2)),
        _stem + "_backward_f32": (c_int, [c_void_p] * 4 + [c_int, c_void_p] + _lay + _geo + [c_int, c_int] + [c_void_p] * 4 + _b
                                  + [c_void_p] * 2),
    })

_lib = None


def lib():
    """The loaded library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VqaeHipError(f"{LIB_PATH} is missing: build it with 2d-vq-ae-2_amd/build.sh "
                               "(__graft_entry__.build()); there is no CPU fallback")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc: int):
    """Map a vqae_status to the reference's exception types."""
    if rc == 0:
        return
    msg = lib().vqae_last_error().decode(errors="replace")
    if rc == -1:
        raise AssertionError(msg)                 # reference: assert (vq.py:98, conv_block.py:148)
    if rc == -2:
        raise NotImplementedError(msg)            # reference: vq.py:100-104
    if rc == -5:
        raise KeyError(msg)                       # missing state-dict entry
    if rc == -4:
        raise MemoryError(msg)
    if rc == -6:
        raise ValueError(msg)                     # reference: torchmetrics' ValueError
    raise VqaeHipError(f"libvqae_hip error {rc}: {msg}")
