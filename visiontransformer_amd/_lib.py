"""ctypes binding of csrc/libvitseg.so (C ABI: include/vitseg.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, importing
this module's `lib()` raises -- the product path must never silently run elsewhere.
"""
from __future__ import annotations

import ctypes as C
import os

from .config import ViTSegConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvitseg.so")

OK, EINVAL, ESHAPE, EWORKSPACE, EHIP = 0, -1, -2, -3, -4
F32, BF16, F16, F32X3 = 0, 1, 2, 3
BUF_TOKENS, BUF_LOWRES = 0, 1

# enum vitseg_tensor
(T_CLS, T_POS, T_PATCH_W, T_PATCH_B, T_LN1_W, T_LN1_B, T_WQKV, T_BQKV, T_WO, T_BO, T_LN2_W, T_LN2_B,
 T_W1, T_B1, T_W2, T_B2, T_LNF_W, T_LNF_B, T_HEAD0_W, T_HEAD0_B, T_HEAD2_W, T_HEAD2_B, T_COUNT) = range(23)

EXPORTS = [
    "vitseg_version", "vitseg_last_error", "vitseg_set_option", "vitseg_get_option", "vitseg_param_count", "vitseg_param_offset", "vitseg_cast_params_bf16",
    "vitseg_query_workspace", "vitseg_workspace_offset", "vitseg_forward", "vitseg_op_layernorm_f32",
    "vitseg_op_linear_f32", "vitseg_op_attention_f32", "vitseg_op_upsample_argmax", "vitseg_op_upsample_bwd",
    "vitseg_profile_enable", "vitseg_profile_collect", "vitseg_op_linear_bf16", "vitseg_op_attention_bf16",
    "vitseg_ce_scratch_bytes", "vitseg_ce_loss",
    "vitseg_train_workspace", "vitseg_forward_train", "vitseg_backward", "vitseg_adam_step",
    "vitseg_grad_bucket_count", "vitseg_grad_bucket_range",
    "vitseg_cast_params_f16", "vitseg_op_linear_f16", "vitseg_op_attention_f16", "vitseg_op_linear_f32x3", "vitseg_op_attention_f32x3", "vitseg_cast_params_split",
    "vitseg_resize_taps", "vitseg_resize_coeffs", "vitseg_nearest_index", "vitseg_preprocess_u8",
    "vitseg_resize_nearest_u8", "vitseg_eval_counts", "vitseg_paed_scratch_bytes", "vitseg_paed_multiclass_loss",
    "vitseg_op_gemm_f32", "vitseg_op_attention_bwd_f32", "vitseg_op_layernorm_bwd_f32", "vitseg_op_linear_h16_ex",
    "vitseg_op_wgrad_bf16", "vitseg_op_wgrad_bf16_scratch_floats", "vitseg_op_attention_bwd_bf16", "vitseg_attention_dropmask_bytes", "vitseg_attention_bwd_scratch_floats", "vitseg_op_colsum_scratch_floats",
    "vitseg_paed_binary_scratch_bytes", "vitseg_paed_binary_loss", "vitseg_op_linear_f32_ex", "vitseg_resize_nearest_i64",
    "vitseg_small_splits", "vitseg_op_linear_f32_small", "vitseg_op_linear_resln_f32_small", "vitseg_op_attention_f32_small", "vitseg_op_attention_bwd_f32_small", "vitseg_op_linear_h16_small", "vitseg_op_attention_h16_small", "vitseg_forward_route", "vitseg_op_layernorm_bwd_f32_small",
    "vitseg_dbg_linear_f32_small", "vitseg_adamw_step", "vitseg_op_dgrad_f32_small", "vitseg_op_wgrad_f32_small", "vitseg_op_layernorm_bwd_scratch_floats",
]
# other input sizes (interpolated position embeddings): bound on first use, so that a library built before them still
# serves everything else; the new path alone raises a "rebuild" error against it (`at_symbol`)
AT_EXPORTS = [
    "vitseg_query_workspace_at", "vitseg_workspace_offset_at", "vitseg_forward_at", "vitseg_train_workspace_at",
    "vitseg_forward_train_at", "vitseg_backward_at", "vitseg_pos_interp", "vitseg_pos_interp_bwd",
]
# connected regions of class masks and their boxes (regions.py): bound on first use, the same way
REGION_EXPORTS = ["vitseg_regions_scratch_bytes", "vitseg_regions"]
# exact distance transforms and the signed-distance targets of binary masks (sdf.py): bound on first use, the same way
SDF_EXPORTS = ["vitseg_sdf_scratch_bytes", "vitseg_sdf"]
# the K-sliced GEMM paths, one entry each, and the router's slice counts (tests/test_splitk_cpu.py, tests/test_gpu_splitk.py):
# bound on first use, the same way
SPLITK_EXPORTS = ["vitseg_op_linear_f32_thin", "vitseg_op_wgrad_f32_scratch_floats", "vitseg_op_wgrad_f32", "vitseg_dbg_gemm_slices"]
# the fused cross-entropy with ignore_index / class weights / label smoothing (model.ce_loss): bound on first use, the same way
CE_OPTS_EXPORTS = ["vitseg_ce_options_scratch_bytes", "vitseg_ce_loss_opts", "vitseg_backward_opts"]
# the embedding, seg-head and training helper kernels, one entry per production launch (csrc/op_helpers.hip,
# tests/test_gpu_helpers.py): bound on first use, the same way
HELPER_EXPORTS = [
    "vitseg_op_patch_embed_f32", "vitseg_op_conv3x3_f32", "vitseg_op_conv3x3_h16", "vitseg_op_head1x1",
    "vitseg_op_head1x1_bwd_scratch_floats", "vitseg_op_head1x1_bwd", "vitseg_op_colsum", "vitseg_op_embed_bwd",
    "vitseg_op_im2col3x3", "vitseg_op_im2col3x3_bf16", "vitseg_op_im2col_patch", "vitseg_op_im2col_patch_bf16",
    "vitseg_op_conv_dgrad_weight", "vitseg_op_transpose_bf16", "vitseg_op_transpose_layers_bf16", "vitseg_op_dropout_rows",
    "vitseg_op_layernorm_h16",
]
# sliding-window inference (model.predict_mask_windowed): the window grid, the tile gather, the forward that stops at the low-res
# head output and the overlapping-tile blend: bound on first use, the same way
WINDOW_EXPORTS = ["vitseg_window_count", "vitseg_window_origins", "vitseg_window_gather", "vitseg_forward_lowres",
                  "vitseg_window_blend"]
# CE + soft Dice in one fused loss (model.ce_dice_loss): bound on first use, the same way
DICE_EXPORTS = ["vitseg_dice_options_scratch_bytes", "vitseg_ce_dice_loss", "vitseg_backward_dice"]
# boundary-distance statistics of class maps: PAED, Hausdorff, HD95, ASSD (metrics.Evaluator.distance_metrics): bound on first
# use, the same way
DISTANCE_EXPORTS = ["vitseg_distance_scratch_bytes", "vitseg_distance_stats"]
# skeletons by Zhang-Suen thinning and the crack statistics on them: clDice, length, width (skeleton.py,
# metrics.Evaluator.crack_metrics): bound on first use, the same way
SKELETON_EXPORTS = ["vitseg_skeleton_scratch_bytes", "vitseg_skeleton", "vitseg_skeleton_stats_scratch_bytes",
                    "vitseg_skeleton_stats"]
SKELETON_AUTO, SKELETON_RESIDENT, SKELETON_GLOBAL = 0, 1, 2   # the `route` argument
# training augmentation: the paired affine warp + colour jitter launch and its host-side matrix composer (augment.py): bound on
# first use, the same way
AUGMENT_EXPORTS = ["vitseg_augment_matrix", "vitseg_augment"]
AUGMENT_CONSTANT, AUGMENT_EDGE = 0, 1      # enum vitseg_augment_border
AUGMENT_U8_NHWC, AUGMENT_F32_NCHW = 0, 1   # enum vitseg_augment_format
# test-time augmentation (model.predict_mask_tta): the exact affine of a flip / quarter-turn view and the launch that merges the
# views' low-res maps: bound on first use, the same way
TTA_EXPORTS = ["vitseg_tta_affine", "vitseg_tta_blend"]
TTA_LOGITS, TTA_PROBS = 0, 1   # the `mode` argument of vitseg_tta_blend
# mask clean-up: regions below a minimum area out, enclosed holes filled (clean.py): bound on first use, the same way
CLEAN_EXPORTS = ["vitseg_clean_scratch_bytes", "vitseg_clean_mask"]
CLEAN_STATS = ("regions_removed", "pixels_removed", "holes_filled", "pixels_filled", "holes_mixed", "holes_over_area")
# region-level detection statistics: predicted regions matched against the true ones, PQ (metrics.Evaluator.region_metrics):
# bound on first use, the same way
MATCH_EXPORTS = ["vitseg_region_match_scratch_bytes", "vitseg_region_match"]
MATCH_STATS = ("n_gt", "n_pred", "tp", "gt_found", "pred_confirmed", "sum_q", "sum_i", "sum_u")
# per-region measurements: moments, perimeter, frame contact, per-region skeleton length and widths (regions.region_props):
# bound on first use, the same way
PROPS_EXPORTS = ["vitseg_region_props_scratch_bytes", "vitseg_region_props"]
PROPS_FIELDS = 20   # include/vitseg.h VITSEG_PROPS_FIELDS
# confidence of a stated mask: per-pixel scores, per-region score rows, calibration histogram (confidence.py): bound on first
# use, the same way
CONFIDENCE_EXPORTS = ["vitseg_confidence"]
CONF_PROB, CONF_MARGIN = 0, 1   # enum vitseg_conf_kind
_LATE_EXPORTS = (AT_EXPORTS + REGION_EXPORTS + SDF_EXPORTS + SPLITK_EXPORTS + CE_OPTS_EXPORTS + HELPER_EXPORTS + WINDOW_EXPORTS
                 + DICE_EXPORTS + DISTANCE_EXPORTS + SKELETON_EXPORTS + AUGMENT_EXPORTS + TTA_EXPORTS + CLEAN_EXPORTS + MATCH_EXPORTS
                 + PROPS_EXPORTS + CONFIDENCE_EXPORTS)
EXPORTS += _LATE_EXPORTS   # every symbol include/vitseg.h declares
# enum vitseg_slices_path
SLICES_WHOLE_F32, SLICES_WHOLE_H16, SLICES_THIN_F32, SLICES_THIN_H16, SLICES_WGRAD_F32, SLICES_WGRAD_BF16_TT, SLICES_WGRAD_BF16_P8 = range(7)
VERSION = 110   # include/vitseg.h VITSEG_VERSION this binding was written against
KERNEL_KINDS = ["gemm_bias", "gemm_gelu", "gemm_resadd", "gemm_patch", "gemm_conv3", "attention", "layernorm",
                "head1x1", "upsample", "train_gemm_fwd", "train_dgrad", "train_wgrad", "train_attn_fwd", "train_attn_bwd"]


class CCEOptions(C.Structure):
    """struct vitseg_ce_options (include/vitseg.h)."""
    _fields_ = [("has_ignore_index", C.c_int32), ("reserved", C.c_int32), ("ignore_index", C.c_int64),
                ("class_weight", C.c_void_p), ("label_smoothing", C.c_float), ("scratch", C.c_void_p),
                ("scratch_bytes", C.c_size_t)]


class CDiceOptions(C.Structure):
    """struct vitseg_dice_options (include/vitseg.h)."""
    _fields_ = [("ce_weight", C.c_float), ("dice_weight", C.c_float), ("smooth", C.c_float),
                ("include_background", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


class CAugmentMask(C.Structure):
    """struct vitseg_augment_mask (include/vitseg.h)."""
    _fields_ = [("src", C.c_void_p), ("matrix", C.c_void_p), ("out", C.c_void_p), ("src_is_i64", C.c_int32),
                ("out_is_i64", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("oh", C.c_int32), ("ow", C.c_int32)]


class CTTAView(C.Structure):
    """struct vitseg_tta_view (include/vitseg.h)."""
    _fields_ = [("lowres", C.c_void_p), ("g", C.c_int32), ("op", C.c_int32), ("weight", C.c_float)]


class CConfig(C.Structure):
    _fields_ = [("num_classes", C.c_int32), ("patch_size", C.c_int32), ("hidden_size", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("image_size", C.c_int32),
                ("intermediate_size", C.c_int32), ("num_channels", C.c_int32), ("layer_norm_eps", C.c_float)]

    @classmethod
    def from_config(cls, cfg: ViTSegConfig) -> "CConfig":
        return cls(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                   cfg.num_attention_heads, cfg.image_size, cfg.intermediate_size, cfg.num_channels,
                   cfg.layer_norm_eps)


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m visiontransformer_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
        l = C.CDLL(LIB_PATH)
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        pcfg, psz = C.POINTER(CConfig), C.POINTER(C.c_size_t)
        l.vitseg_version.restype = i32
        l.vitseg_last_error.restype = C.c_char_p
        l.vitseg_set_option.argtypes = [C.c_char_p, C.c_longlong]
        l.vitseg_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_longlong)]
        l.vitseg_param_count.argtypes = [pcfg, psz]
        l.vitseg_param_offset.argtypes = [pcfg, i32, i32, psz, psz]
        l.vitseg_cast_params_bf16.argtypes = [vp, vp, sz, vp]
        l.vitseg_cast_params_f16.argtypes = [vp, vp, sz, vp]
        l.vitseg_cast_params_split.argtypes = [vp, vp, sz, vp]
        l.vitseg_query_workspace.argtypes = [pcfg, i32, i32, psz]
        l.vitseg_workspace_offset.argtypes = [pcfg, i32, i32, i32, psz, psz]
        l.vitseg_forward.argtypes = [pcfg, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]
        l.vitseg_op_layernorm_f32.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, vp]
        l.vitseg_op_linear_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_linear_f32_ex.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_uint32, C.c_uint32, vp]
        l.vitseg_op_attention_f32.argtypes = [vp, vp, i32, i32, i32, vp]
        l.vitseg_op_attention_f32_small.argtypes = [vp, vp, i32, i32, i32, vp]
        l.vitseg_small_splits.argtypes = [i32, i32]
        l.vitseg_op_layernorm_bwd_scratch_floats.argtypes = [i32, i32]
        l.vitseg_op_layernorm_bwd_scratch_floats.restype = sz
        l.vitseg_op_wgrad_f32_small.argtypes = [vp, vp, vp, i32, i32, i32, vp]
        l.vitseg_op_dgrad_f32_small.argtypes = [vp, vp, vp, vp, vp, sz, i32, i32, i32, i32, vp]
        l.vitseg_dbg_linear_f32_small.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp]
        l.vitseg_op_linear_f32_small.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_linear_resln_f32_small.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, sz, i32, i32, i32, C.c_float, vp]
        l.vitseg_op_linear_bf16.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_attention_bf16.argtypes = [vp, vp, i32, i32, i32, vp]
        l.vitseg_op_linear_f16.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_linear_f32x3.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_wgrad_bf16_scratch_floats.argtypes = [i32, i32, i32]
        l.vitseg_op_wgrad_bf16_scratch_floats.restype = sz
        l.vitseg_op_wgrad_bf16.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, vp]
        l.vitseg_op_linear_h16_ex.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, C.c_float,
                                              C.c_uint32, C.c_uint32, vp, vp, vp]
        l.vitseg_op_colsum_scratch_floats.argtypes = [i32, i32]
        l.vitseg_op_colsum_scratch_floats.restype = sz
        l.vitseg_op_attention_f16.argtypes = [vp, vp, i32, i32, i32, vp]
        l.vitseg_op_attention_f32x3.argtypes = [vp, vp, i32, i32, i32, vp]
        l.vitseg_op_upsample_argmax.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_upsample_bwd.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_ce_scratch_bytes.argtypes = [i32, i32]
        l.vitseg_ce_scratch_bytes.restype = sz
        l.vitseg_ce_loss.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp]
        f32 = C.c_float
        l.vitseg_train_workspace.argtypes = [pcfg, i32, i32, psz]
        l.vitseg_forward_train.argtypes = [pcfg, vp, vp, vp, i32, i32, f32, C.c_uint64, vp, vp, sz, vp]
        l.vitseg_backward.argtypes = [pcfg, vp, vp, vp, i32, i32, f32, C.c_uint64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp]
        l.vitseg_grad_bucket_count.argtypes = [pcfg]
        l.vitseg_resize_taps.argtypes = [i32, i32]
        l.vitseg_paed_scratch_bytes.argtypes = [i32, i32, i32, i32]
        l.vitseg_paed_scratch_bytes.restype = sz
        l.vitseg_paed_multiclass_loss.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, i32, vp, vp, vp, vp]
        l.vitseg_paed_binary_scratch_bytes.argtypes = [i32, i32, i32]
        l.vitseg_paed_binary_scratch_bytes.restype = sz
        l.vitseg_paed_binary_loss.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
        l.vitseg_resize_coeffs.argtypes = [i32, i32, vp, vp]
        l.vitseg_nearest_index.argtypes = [i32, i32, i32, vp]
        l.vitseg_preprocess_u8.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp]
        l.vitseg_resize_nearest_u8.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp]
        l.vitseg_resize_nearest_i64.argtypes = [vp, i32, i32, i32, vp, vp, i32, i32, i32, vp, vp]
        l.vitseg_eval_counts.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
        l.vitseg_grad_bucket_range.argtypes = [pcfg, i32, psz, psz]
        l.vitseg_adam_step.argtypes = [vp, vp, vp, vp, sz, f32, f32, f32, f32, i32, f32, vp]
        l.vitseg_adamw_step.argtypes = [vp, vp, vp, vp, sz, f32, f32, f32, f32, f32, i32, f32, vp]
        l.vitseg_op_gemm_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
        l.vitseg_op_attention_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp]
        l.vitseg_op_layernorm_bwd_f32_small.argtypes = [vp, vp, vp, sz, i32, vp, vp, vp, vp, vp, i32, i32, f32, vp, vp, f32, C.c_uint32, C.c_uint32, vp]
        l.vitseg_forward_route.argtypes = [pcfg, i32, i32]
        l.vitseg_op_attention_h16_small.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        l.vitseg_op_linear_h16_small.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, sz, vp]
        l.vitseg_op_attention_bwd_f32_small.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, f32, C.c_uint32, C.c_uint32, vp]
        l.vitseg_attention_bwd_scratch_floats.argtypes = [i32, i32, i32]
        l.vitseg_attention_bwd_scratch_floats.restype = sz
        l.vitseg_op_attention_bwd_bf16.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, C.c_float, C.c_uint32, C.c_uint32, vp, vp, vp]
        l.vitseg_attention_dropmask_bytes.argtypes = [i32, i32, i32]
        l.vitseg_attention_dropmask_bytes.restype = C.c_size_t
        l.vitseg_op_layernorm_bwd_f32.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, vp]
        l.vitseg_profile_enable.argtypes = [i32]
        l.vitseg_profile_collect.argtypes = [i32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        for name in EXPORTS:
            if name not in _LATE_EXPORTS:
                getattr(l, name)  # raises AttributeError if the build is stale
        for name, args in _at_argtypes(vp, sz, i32, pcfg, psz).items():
            fn = getattr(l, name, None)
            if fn is not None:
                fn.argtypes = args
        if getattr(l, "vitseg_regions", None) is not None:
            l.vitseg_regions_scratch_bytes.argtypes = [i32, i32, i32]
            l.vitseg_regions_scratch_bytes.restype = sz
            l.vitseg_regions.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp, sz, vp]
        if getattr(l, "vitseg_sdf", None) is not None:
            l.vitseg_sdf_scratch_bytes.argtypes = [i32, i32, i32]
            l.vitseg_sdf_scratch_bytes.restype = sz
            l.vitseg_sdf.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]
        if getattr(l, "vitseg_distance_stats", None) is not None:
            l.vitseg_distance_scratch_bytes.argtypes = [i32, i32, i32]
            l.vitseg_distance_scratch_bytes.restype = sz
            l.vitseg_distance_stats.argtypes = [vp, vp, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, i32, i32, vp, vp, vp,
                                                sz, vp]
        if getattr(l, "vitseg_skeleton_stats", None) is not None:
            l.vitseg_skeleton_scratch_bytes.argtypes = [i32, i32, i32, i32]
            l.vitseg_skeleton_scratch_bytes.restype = sz
            l.vitseg_skeleton.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp]
            l.vitseg_skeleton_stats_scratch_bytes.argtypes = [i32, i32, i32, i32]
            l.vitseg_skeleton_stats_scratch_bytes.restype = sz
            l.vitseg_skeleton_stats.argtypes = [vp, vp, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, vp, vp, vp, sz, vp]
        if getattr(l, "vitseg_dbg_gemm_slices", None) is not None:
            l.vitseg_op_linear_f32_thin.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, sz, C.c_float,
                                                    C.c_uint32, C.c_uint32, vp]
            l.vitseg_op_wgrad_f32_scratch_floats.argtypes = [i32, i32, i32]
            l.vitseg_op_wgrad_f32_scratch_floats.restype = sz
            l.vitseg_op_wgrad_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp]
            l.vitseg_dbg_gemm_slices.argtypes = [i32, i32, i32, i32]
        if getattr(l, "vitseg_backward_opts", None) is not None:
            for name, args in _ce_opts_argtypes(vp, sz, i32, pcfg).items():
                getattr(l, name).argtypes = args
            l.vitseg_ce_options_scratch_bytes.restype = sz
        if getattr(l, "vitseg_op_patch_embed_f32", None) is not None:
            for name, args in _helper_argtypes(vp, sz, i32).items():
                getattr(l, name).argtypes = args
            l.vitseg_op_head1x1_bwd_scratch_floats.restype = sz
        if getattr(l, "vitseg_window_blend", None) is not None:
            for name, args in _window_argtypes(vp, sz, i32, pcfg).items():
                getattr(l, name).argtypes = args
        if getattr(l, "vitseg_backward_dice", None) is not None:
            for name, args in _dice_argtypes(vp, sz, i32, pcfg).items():
                getattr(l, name).argtypes = args
            l.vitseg_dice_options_scratch_bytes.restype = sz
        if getattr(l, "vitseg_augment", None) is not None:
            l.vitseg_augment_matrix.argtypes = [vp, i32, i32, i32, i32, vp]   # (double[6] in, int64[6] out)
            l.vitseg_augment.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, C.POINTER(CAugmentMask), i32, i32,
                                         C.POINTER(C.c_float), C.c_int64, vp]
        if getattr(l, "vitseg_tta_blend", None) is not None:
            l.vitseg_tta_affine.argtypes = [i32, vp]   # (double[6] out)
            l.vitseg_tta_blend.argtypes = [C.POINTER(CTTAView), i32, i32, i32, i32, i32, vp, vp, vp]
        if getattr(l, "vitseg_clean_mask", None) is not None:
            l.vitseg_clean_scratch_bytes.argtypes = [i32, i32, i32]
            l.vitseg_clean_scratch_bytes.restype = sz
            l.vitseg_clean_mask.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]
        if getattr(l, "vitseg_region_match", None) is not None:
            l.vitseg_region_match_scratch_bytes.argtypes = [i32, i32, i32]
            l.vitseg_region_match_scratch_bytes.restype = sz
            l.vitseg_region_match.argtypes = [vp, vp, i32, i32, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp,
                                              sz, vp]
        if getattr(l, "vitseg_region_props", None) is not None:
            l.vitseg_region_props_scratch_bytes.argtypes = [i32, i32, i32, i32, i32]
            l.vitseg_region_props_scratch_bytes.restype = sz
            l.vitseg_region_props.argtypes = [vp, i32, i32, i32, i32, i32, C.POINTER(C.c_int32), i32, i32, vp, vp, i32, vp, vp,
                                              sz, vp]
        if getattr(l, "vitseg_confidence", None) is not None:
            l.vitseg_confidence.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, i32, vp, i32, vp, i32, vp]
        if l.vitseg_version() != VERSION:   # argument lists changed between versions: a stale .so would misread them
            raise RuntimeError(f"{LIB_PATH} is version {l.vitseg_version()}, this binding expects {VERSION}: rebuild it "
                               "(python -m visiontransformer_amd.build)")
        _lib = l
    return _lib


def _at_argtypes(vp, sz, i32, pcfg, psz) -> dict:
    f32 = C.c_float
    return {
        "vitseg_query_workspace_at": [pcfg, i32, i32, i32, psz],
        "vitseg_workspace_offset_at": [pcfg, i32, i32, i32, i32, psz, psz],
        "vitseg_forward_at": [pcfg, i32, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp],
        "vitseg_train_workspace_at": [pcfg, i32, i32, i32, psz],
        "vitseg_forward_train_at": [pcfg, i32, vp, vp, vp, i32, i32, f32, C.c_uint64, vp, vp, sz, vp],
        "vitseg_backward_at": [pcfg, i32, vp, vp, vp, i32, i32, f32, C.c_uint64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp],
        "vitseg_pos_interp": [vp, vp, i32, i32, i32, vp],
        "vitseg_pos_interp_bwd": [vp, vp, vp, i32, i32, i32, vp],
    }


def _ce_opts_argtypes(vp, sz, i32, pcfg) -> dict:
    f32, popt = C.c_float, C.POINTER(CCEOptions)
    return {
        "vitseg_ce_options_scratch_bytes": [i32, i32],
        "vitseg_ce_loss_opts": [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, popt, f32, vp],
        "vitseg_backward_opts": [pcfg, i32, vp, vp, vp, i32, i32, f32, C.c_uint64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp,
                                 popt],
    }


def _dice_argtypes(vp, sz, i32, pcfg) -> dict:
    f32, popt, pdice = C.c_float, C.POINTER(CCEOptions), C.POINTER(CDiceOptions)
    return {
        "vitseg_dice_options_scratch_bytes": [i32, i32, i32],
        "vitseg_ce_dice_loss": [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, popt, pdice, f32, vp],
        "vitseg_backward_dice": [pcfg, i32, vp, vp, vp, i32, i32, f32, C.c_uint64, vp, i32, vp, vp, vp, f32, vp, vp, sz, vp,
                                 popt, pdice, vp],
    }


def _window_argtypes(vp, sz, i32, pcfg) -> dict:
    return {
        "vitseg_window_count": [i32, i32, i32],
        "vitseg_window_origins": [i32, i32, i32, vp],
        "vitseg_window_gather": [vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, i32, i32, vp, vp],
        "vitseg_forward_lowres": [pcfg, i32, vp, vp, vp, i32, i32, vp, vp, sz, vp],
        "vitseg_window_blend": [vp, vp, i32, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp],
    }


def _helper_argtypes(vp, sz, i32) -> dict:
    f32, u32 = C.c_float, C.c_uint32
    return {
        "vitseg_op_patch_embed_f32": [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "vitseg_op_conv3x3_f32": [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "vitseg_op_conv3x3_h16": [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp],
        "vitseg_op_head1x1": [vp, vp, vp, vp, i32, i32, i32, vp],
        "vitseg_op_head1x1_bwd_scratch_floats": [i32, i32, i32],
        "vitseg_op_head1x1_bwd": [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp],
        "vitseg_op_colsum": [vp, i32, vp, vp, i32, i32, i32, vp],
        "vitseg_op_embed_bwd": [vp, vp, vp, i32, i32, i32, vp],
        "vitseg_op_im2col3x3": [vp, i32, vp, i32, i32, i32, vp],
        "vitseg_op_im2col3x3_bf16": [vp, vp, i32, i32, i32, vp],
        "vitseg_op_im2col_patch": [vp, vp, i32, i32, i32, i32, vp],
        "vitseg_op_im2col_patch_bf16": [vp, vp, i32, i32, i32, i32, vp],
        "vitseg_op_conv_dgrad_weight": [vp, vp, i32, vp],
        "vitseg_op_transpose_bf16": [vp, vp, i32, i32, i32, i32, vp],
        "vitseg_op_transpose_layers_bf16": [vp, vp, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), sz, i32, vp],
        "vitseg_op_dropout_rows": [vp, vp, i32, i32, i32, f32, u32, u32, vp],
        "vitseg_op_layernorm_h16": [vp, vp, vp, vp, i32, i32, f32, i32, vp],
    }


def helper_symbol(name: str):
    """One of HELPER_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the helper-kernel entry points): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def ce_opts_symbol(name: str):
    """One of CE_OPTS_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the cross-entropy options): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def dice_symbol(name: str):
    """One of DICE_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the CE + Dice loss): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def at_symbol(name: str):
    """One of AT_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before interpolated position embeddings): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def region_symbol(name: str):
    """One of REGION_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before connected regions): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def clean_symbol(name: str):
    """One of CLEAN_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the mask clean-up): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def sdf_symbol(name: str):
    """One of SDF_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before distance transforms): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def match_symbol(name: str):
    """One of MATCH_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the region matching): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def props_symbol(name: str):
    """One of PROPS_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the per-region measurements): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def confidence_symbol(name: str):
    """One of CONFIDENCE_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the confidence scores): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def distance_symbol(name: str):
    """One of DISTANCE_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the boundary-distance metrics): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def skeleton_symbol(name: str):
    """One of SKELETON_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the skeletons): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def augment_symbol(name: str):
    """One of AUGMENT_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the training augmentation): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def augment_matrix(affine, src_hw, dst_hw) -> list:
    """The Q16 int64 matrix (six entries) of one normalised 2x3 affine for one (source, output) size pair
    (vitseg_augment_matrix); ValueError for an extent outside 1..16384 or an entry past the kernel's clamp bounds."""
    a = (C.c_double * 6)(*[float(v) for v in affine])
    out = (C.c_int64 * 6)()
    check(augment_symbol("vitseg_augment_matrix")(a, int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1]), out))
    return list(out)


def tta_symbol(name: str):
    """One of TTA_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before test-time augmentation): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def tta_affine(op: int) -> list:
    """The normalised 2x3 affine (six doubles) of view(., op) for `augment_matrix` (vitseg_tta_affine); ValueError for an
    op outside 0..7."""
    out = (C.c_double * 6)()
    if tta_symbol("vitseg_tta_affine")(int(op), out):
        raise ValueError(lib().vitseg_last_error().decode(errors="replace"))
    return list(out)


def window_symbol(name: str):
    """One of WINDOW_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before sliding-window inference): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def window_origins(extent: int, S: int, stride: int) -> list:
    """Origins of the windows along one axis (vitseg_window_origins): i * stride, the last one shifted back to end at the edge.
    ValueError for an extent shorter than the window, a stride outside 1..S or an extent above 16384."""
    n = int(window_symbol("vitseg_window_count")(int(extent), int(S), int(stride)))
    if n < 0:
        check(n)
    out = (C.c_int32 * n)()
    check(window_symbol("vitseg_window_origins")(int(extent), int(S), int(stride), out))
    return list(out)


def splitk_symbol(name: str):
    """One of SPLITK_EXPORTS, or a RuntimeError naming the rebuild when the loaded library predates it."""
    fn = getattr(lib(), name, None)
    if fn is None:
        raise RuntimeError(f"{LIB_PATH} has no {name} (built before the split-K entry points): rebuild it "
                           "(python -m visiontransformer_amd.build)")
    return fn


def gemm_slices(path: int, M: int, N: int, K: int) -> int:
    """K slices of a GEMM with a dense [M, N] output on one of the router's sliced paths (SLICES_*); 0: the path does not apply."""
    return int(splitk_symbol("vitseg_dbg_gemm_slices")(path, M, N, K))


def _native(cfg: ViTSegConfig, image_size) -> bool:
    return image_size is None or int(image_size) == cfg.image_size


def check(rc: int) -> None:
    """Maps C status codes to the exception types the reference raises
    (ValueError for shapes the reference rejects, modeling_vit.py:63-68,152-156)."""
    if rc == OK:
        return
    msg = lib().vitseg_last_error().decode(errors="replace")
    if rc == ESHAPE:
        raise ValueError(msg)
    raise RuntimeError(f"libvitseg error {rc}: {msg}")


def set_option(name: str, value: int) -> None:
    """Dispatcher switch (include/vitseg.h vitseg_set_option): e.g. set_option("no_f32p", 1)."""
    check(lib().vitseg_set_option(name.encode(), int(value)))


def get_option(name: str) -> int:
    v = C.c_longlong()
    check(lib().vitseg_get_option(name.encode(), C.byref(v)))
    return int(v.value)


class option:
    """`with _lib.option("no_p8", 1): ...` -- the switch is restored on exit."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False


def param_count(cfg: ViTSegConfig) -> int:
    n = C.c_size_t()
    check(lib().vitseg_param_count(C.byref(CConfig.from_config(cfg)), C.byref(n)))
    return n.value


def param_offset(cfg: ViTSegConfig, tensor: int, layer: int = 0):
    off, n = C.c_size_t(), C.c_size_t()
    check(lib().vitseg_param_offset(C.byref(CConfig.from_config(cfg)), tensor, layer, C.byref(off), C.byref(n)))
    return off.value, n.value


def query_workspace(cfg: ViTSegConfig, batch: int, precision: int, image_size=None) -> int:
    """Bytes of the forward workspace; `image_size`: the input's side when it differs from cfg's (vitseg_query_workspace_at)."""
    n = C.c_size_t()
    if _native(cfg, image_size):
        check(lib().vitseg_query_workspace(C.byref(CConfig.from_config(cfg)), batch, precision, C.byref(n)))
    else:
        check(at_symbol("vitseg_query_workspace_at")(C.byref(CConfig.from_config(cfg)), int(image_size), batch, precision,
                                                     C.byref(n)))
    return n.value


def forward_route(cfg: ViTSegConfig, batch: int, precision: int, image_size=None) -> str:
    """"small" (the small-batch route of csrc/small.hpp) or "large": which kernels vitseg_forward takes for this call.  The
    route depends on the activations only, so an input of another size asks with cfg at that size."""
    c = CConfig.from_config(cfg)
    if not _native(cfg, image_size):
        c.image_size = int(image_size)
    rc = lib().vitseg_forward_route(C.byref(c), batch, precision)
    if rc < 0:
        check(rc)
    return "small" if rc == 1 else "large"


def workspace_offset(cfg: ViTSegConfig, batch: int, precision: int, buffer: int, image_size=None):
    off, n = C.c_size_t(), C.c_size_t()
    if _native(cfg, image_size):
        check(lib().vitseg_workspace_offset(C.byref(CConfig.from_config(cfg)), batch, precision, buffer,
                                            C.byref(off), C.byref(n)))
    else:
        check(at_symbol("vitseg_workspace_offset_at")(C.byref(CConfig.from_config(cfg)), int(image_size), batch, precision,
                                                      buffer, C.byref(off), C.byref(n)))
    return off.value, n.value


def train_workspace(cfg: ViTSegConfig, batch: int, precision: int, image_size=None) -> int:
    n = C.c_size_t()
    if _native(cfg, image_size):
        check(lib().vitseg_train_workspace(C.byref(CConfig.from_config(cfg)), batch, precision, C.byref(n)))
    else:
        check(at_symbol("vitseg_train_workspace_at")(C.byref(CConfig.from_config(cfg)), int(image_size), batch, precision,
                                                     C.byref(n)))
    return n.value


def grad_buckets(cfg: ViTSegConfig) -> list:
    """[(offset_floats, n_floats)] of the gradient arena in the order vitseg_backward finishes them
    (0 = final norm + seg_head, 1 .. L = layers L-1 .. 0, L + 1 = embeddings)."""
    c = CConfig.from_config(cfg)
    n = lib().vitseg_grad_bucket_count(C.byref(c))
    if n < 0:
        check(n)
    out = []
    for i in range(n):
        off, cnt = C.c_size_t(), C.c_size_t()
        check(lib().vitseg_grad_bucket_range(C.byref(c), i, C.byref(off), C.byref(cnt)))
        out.append((off.value, cnt.value))
    return out


def profile_enable(on: bool) -> None:
    check(lib().vitseg_profile_enable(1 if on else 0))


def profile_collect() -> dict:
    """kind -> dict(ms, launches, work) for every kernel kind recorded since profile_enable(True)."""
    out = {}
    for i, name in enumerate(KERNEL_KINDS):
        ms, n, w = C.c_double(), C.c_int64(), C.c_double()
        check(lib().vitseg_profile_collect(i, C.byref(ms), C.byref(n), C.byref(w)))
        out[name] = dict(ms=ms.value, launches=n.value, work=w.value)
    return out
