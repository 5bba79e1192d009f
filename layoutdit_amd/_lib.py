"""ctypes binding of ``libldit_hip.so`` (C ABI: ``include/ldit.h``).

The library is the product; this module only loads it and describes its signatures.  There is deliberately no
fallback: if the shared object is missing or a symbol is absent, import of the compute path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LDIT_LIB_PATH (diagnostic): load another BUILD of this same library - an A/B variant compiled with extra -D flags by
# scripts/build_alt.sh - instead of the shipped one.  Still the HIP library or nothing: there is no other implementation.
LIB_PATH = os.environ.get("LDIT_LIB_PATH") or os.path.join(_HERE, "libldit_hip.so")

LDIT_ABI_VERSION = 6
LDIT_MAX_TAPS = 8
DTYPE_F32, DTYPE_BF16, DTYPE_FP8, DTYPE_F32X3, DTYPE_F32X6, DTYPE_MXFP8 = 0, 1, 3, 4, 5, 6
FP8_A_COUNT = 4
LDIT_OK, LDIT_EINVAL, LDIT_EWORKSPACE, LDIT_EHIP, LDIT_EUNSUPPORTED = 0, -1, -2, -3, -4
EPI_BIAS, EPI_BIAS_GELU, EPI_SCALE_RESID, EPI_F32, EPI_GELU_BWD, EPI_BIAS_RELU = 0, 1, 2, 4, 5, 6
K_GEMM, K_ATTENTION, K_LAYERNORM, K_OTHER, K_COUNT = 0, 1, 2, 3, 4
KERNEL_FAMILIES = ("gemm", "attention", "layernorm", "other")


class LditCfg(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("mlp", C.c_int32),
                ("patch", C.c_int32), ("in_ch", C.c_int32), ("img_h", C.c_int32), ("img_w", C.c_int32),
                ("n_taps", C.c_int32), ("taps", C.c_int32 * LDIT_MAX_TAPS), ("ln_eps", C.c_float),
                ("dtype", C.c_int32), ("flags", C.c_int32)]


LAYER_FIELDS = ("ln1_w", "ln1_b", "wq", "bq", "wk", "wv", "bv", "wo", "bo", "lam1",
                "ln2_w", "ln2_b", "w1", "b1", "w2", "b2", "lam2")


class LditLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LAYER_FIELDS]


class LditWeights(C.Structure):
    _fields_ = [("patch_w", C.c_void_p), ("patch_b", C.c_void_p), ("cls", C.c_void_p), ("pos", C.c_void_p),
                ("layer", C.POINTER(LditLayerWeights))]


class LditOptSegment(C.Structure):
    """One parameter tensor of the multi-tensor optimizer step (``ldit_opt_segment``)."""
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("bf16_mirror", C.c_void_p)]


class LditOptState(C.Structure):
    """Host-side picture of the optimizer's device state block (``ldit_opt_state``): field order and sizes only."""
    _fields_ = [("found_inf", C.c_int32), ("skip", C.c_int32), ("step", C.c_int32), ("growth_tracker", C.c_int32),
                ("skipped_steps", C.c_int32), ("scale", C.c_float), ("inv_scale_used", C.c_float), ("lr", C.c_float),
                ("bc1", C.c_float), ("bc2_sqrt", C.c_float)]


class LditClipState(C.Structure):
    """Host-side picture of the clipping block (``ldit_clip_state``, 16 bytes): field order and sizes only."""
    _fields_ = [("max_norm", C.c_float), ("total_norm", C.c_float), ("clip_coef", C.c_float), ("clipped_steps", C.c_int32)]


class LditOptHyper(C.Structure):
    """One segment's hyper-parameters for the grouped update (``ldit_opt_hyper``, 8 bytes)."""
    _fields_ = [("lr_scale", C.c_float), ("weight_decay", C.c_float)]


class LditAccSegment(C.Structure):
    """One gradient tensor and its slice of the accumulation bucket (``ldit_acc_segment``, 24 bytes)."""
    _fields_ = [("acc", C.c_void_p), ("g", C.c_void_p), ("n", C.c_int64)]


class LditSwapSegment(C.Structure):
    """One pair of the weight / shadow exchange and the optional bf16 copy of ``a`` (``ldit_swap_segment``, 32 bytes)."""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("n", C.c_int64), ("bf16_mirror", C.c_void_p)]


OPT_STATE_FIELDS = tuple(n for n, _ in LditOptState._fields_)       # index of a field = its 4-byte slot in the block
CLIP_STATE_FIELDS = tuple(n for n, _ in LditClipState._fields_)
OPT_MAX_SEGMENTS = 64                                               # segments per launch (csrc/optim_multi.hip)
OPT_GROUP_SEGMENTS = 48                                             # of the grouped update, whose hyper-parameters ride beside them
ACC_MAX_SEGMENTS = 127                                              # of the fold into the gradient bucket: 24 bytes a segment
EMA_MAX_SEGMENTS = 52                                               # of the grouped update with an EMA: a shadow pointer rides along too
SWAP_MAX_SEGMENTS = 99                                              # of the weight / shadow exchange: 32 bytes a segment

# name -> (restype, argtypes); every symbol include/ldit.h declares
_vp, _i64, _i32, _f32, _sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
SIGNATURES = {
    "ldit_abi_version": (C.c_int, []),
    "ldit_last_error": (C.c_char_p, []),
    "ldit_debug_reload_env": (C.c_int, []),
    "ldit_packed_bytes": (_sz, [C.POINTER(LditCfg)]),
    "ldit_pack_weights": (C.c_int, [C.POINTER(LditCfg), C.POINTER(LditWeights), _vp, _sz, _vp]),
    "ldit_workspace_bytes": (_sz, [C.POINTER(LditCfg), _i32]),
    "ldit_forward_lanes": (_i32, [C.POINTER(LditCfg), _i32]),
    "ldit_vit_forward": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _i32, C.POINTER(_vp), _vp, _sz, _vp]),
    "ldit_vit_forward_images": (C.c_int, [C.POINTER(LditCfg), _vp, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _f32, _f32, _i32,
                                          C.POINTER(_vp), _vp, _sz, _vp]),
    "ldit_vit_forward_images_u8": (C.c_int, [C.POINTER(LditCfg), _vp, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _f32, _f32, _i32,
                                             C.POINTER(_vp), _vp, _sz, _vp]),
    "ldit_vit_forward_timed": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _i32, C.POINTER(_vp), _vp, _sz, _vp,
                                         C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ldit_linear_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "ldit_layernorm_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _f32, _vp]),
    "ldit_attention_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp]),
    "ldit_embed_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp]),
    "ldit_attention_planes": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp]),
    "ldit_split_f32_planes": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _vp]),
    "ldit_layernorm_f32_planes": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, C.c_float, _i32, _vp]),
    "ldit_linear_planes": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _i32, _vp]),
    "ldit_embed_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp]),
    "ldit_embed_bf16_images": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _i64, _i64, _i64, _i64, _i64, _i64, _vp]),
    "ldit_embed_bf16_images_u8": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _i64, _i64, _i64, _i64, _i64, _i64, _vp]),
    "ldit_tap_to_map_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp]),
    "ldit_tap_to_map_bwd_f32": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp]),
    "ldit_linear_bf16": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "ldit_attention_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp]),
    "ldit_cast_f32_bf16": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ldit_linear_fp8": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _f32, _f32, _vp, _vp]),
    "ldit_quant_rows_f32_fp8": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "ldit_set_fp8_act_scales": (C.c_int, [C.POINTER(LditCfg), _vp, C.c_size_t, C.POINTER(C.c_float), _vp]),
    "ldit_quant_f32_fp8": (C.c_int, [_vp, _vp, _i64, _f32, _vp]),
    "ldit_quant_mx_f32_fp8": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i64, _vp]),
    "ldit_linear_mxfp8": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "ldit_layernorm_mxfp8": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _vp]),
    "ldit_amax_f32": (C.c_int, [_vp, _i64, _vp, _vp]),
    "ldit_preprocess_f32": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _f32, _f32, _i32, _i32,
                                      _vp, _vp]),
    "ldit_preprocess_f16": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _f32, _f32, _i32, _i32,
                                      _vp, _vp]),
    "ldit_preprocess_u8": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _i32, _f32, _f32, _i32, _i32,
                                     _vp, _vp]),
    "ldit_preprocess_win_f32": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _f32, _f32, _i32,
                                          _i32, _vp, _vp]),
    "ldit_preprocess_win_f16": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _f32, _f32, _i32,
                                          _i32, _vp, _vp]),
    "ldit_preprocess_win_u8": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _i32, _f32, _f32,
                                         _i32, _i32, _vp, _vp]),
    "ldit_augment_targets_f32": (C.c_int, [_vp, _vp, _vp, C.POINTER(_i32), _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp]),
    # test-time augmentation
    "ldit_tta_pool_f32": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32,
                                    _i32, _vp, _vp, _vp, _vp]),
    "ldit_box_vote_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "ldit_cast_f16_f32": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ldit_cast_f32_f16": (C.c_int, [_vp, _vp, _i64, _vp]),
    "ldit_fpn_merge_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _i64, _i64, _vp]),
    "ldit_conv3x3_nhwc_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "ldit_conv3x3_nhwc_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp]),
    "ldit_fpn_merge_bwd_f32": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _i64, _i64, _vp]),
    "ldit_pad_nhwc_f32_bf16": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp]),
    "ldit_colsum_scratch_bytes": (_sz, [_i64, _i64]),
    "ldit_colsum_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "ldit_colamax_f32": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "ldit_relu_bwd_bf16": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "ldit_relu_bwd_pad_nhwc_bf16": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "ldit_relu_bwd_bf16_act16": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "ldit_relu_bwd_pad_nhwc_bf16_act16": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    # train step
    "ldit_flat_param_bytes": (_sz, [C.POINTER(LditCfg)]),
    "ldit_flat_param_layout": (C.c_int, [C.POINTER(LditCfg), C.POINTER(_i64), _i32]),
    "ldit_train_saved_bytes": (_sz, [C.POINTER(LditCfg), _i32]),
    "ldit_train_workspace_bytes": (_sz, [C.POINTER(LditCfg), _i32]),
    "ldit_train_mirror_bytes": (_sz, [C.POINTER(LditCfg)]),
    "ldit_pack_train": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _sz, _vp]),
    "ldit_vit_forward_train": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _vp, _i32, C.POINTER(_vp), _vp, _vp, _sz, _vp,
                                         C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ldit_vit_backward": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _vp, _i32, C.POINTER(_vp), _vp, _vp, _sz, _vp, _sz, _vp, _sz,
                                    _i32, _i32, _vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ldit_adamw_step": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _vp, _vp]),
    "ldit_adamw_step_mxfp8": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _vp, _sz, _vp]),
    "ldit_layernorm_mxfp8_train": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _vp]),
    "ldit_attention_mxfp8_train": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp]),
    "ldit_linear_mxfp8_train": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ldit_attention_fwd_lse_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _vp]),
    "ldit_attention_bwd_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                          _i64, _f32, _vp]),
    "ldit_layernorm_bwd_scratch_bytes": (_sz, [_i64, _i64]),
    "ldit_layernorm_bwd_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp, _sz, _vp]),
    "ldit_layernorm_bwd_resid_scratch_bytes": (_sz, [_i64, _i64]),
    "ldit_layernorm_bwd_resid_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp, _sz,
                                               _vp]),
    "ldit_resid_bwd_scratch_bytes": (_sz, [_i64, _i64]),
    "ldit_resid_bwd_bf16": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "ldit_linear_bf16_ex": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                      _i32, _vp]),
    "ldit_reduce_slabs_f32": (C.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "ldit_linear_bf16_tr": (C.c_int, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i32, _vp, _vp]),
    # region proposals
    "ldit_rpn_topk_f32": (C.c_int, [_vp, C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp]),
    "ldit_rpn_topk_chunked_f32": (C.c_int, [_vp, C.POINTER(_i64), _i32, _i32, _i32, _vp, _vp]),
    "ldit_rpn_decode_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _f32, _f32, _f32, _f32, _vp, _vp, _vp]),
    "ldit_nms_workspace_bytes": (_sz, [_i64, _i64]),
    "ldit_nms_batched_f32": (C.c_int, [_vp, _vp, _vp, _i32, _i64, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    # RPN training
    "ldit_rpn_targets_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _f32, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "ldit_rpn_targets_chunked_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _f32, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "ldit_rpn_loss_workspace_bytes": (_sz, [_i64, _i64]),
    "ldit_rpn_loss_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _f32, _vp, _vp, _vp, _vp, _sz, _vp]),
    # box head training
    "ldit_roi_targets_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _f32, _i32, _f32, C.POINTER(_f32), _vp, _vp, _vp,
                                       _vp, _vp, _vp]),
    "ldit_roi_align_levels_bwd_f32": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i64, C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_f32),
                                                C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), _i32, _i64, _i32, _i32, _vp]),
    "ldit_box_loss_workspace_bytes": (_sz, [_i64]),
    "ldit_box_loss_f32": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _i64, _i32, _f32, _vp, _vp, _vp, _sz, _vp]),
    # detector optimizer step
    "ldit_grads_check_multi_f32": (C.c_int, [C.POINTER(LditOptSegment), _i32, _vp, _vp]),
    "ldit_opt_advance": (C.c_int, [_vp, C.c_double, C.c_double, _f32, _f32, _i32, _vp]),
    "ldit_adamw_multi_f32": (C.c_int, [C.POINTER(LditOptSegment), _i32, _vp, C.c_double, C.c_double, _f32, _f32, _f32, _vp]),
    "ldit_grad_norm_partials": (_i64, [C.POINTER(LditOptSegment), _i32]),
    "ldit_grads_check_norm_multi_f32": (C.c_int, [C.POINTER(LditOptSegment), _i32, _vp, _vp, _i64, _vp]),
    "ldit_clip_finish": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "ldit_adamw_groups_multi_f32": (C.c_int, [C.POINTER(LditOptSegment), C.POINTER(LditOptHyper), _i32, _vp, _vp, C.c_double, C.c_double, _f32,
                                              _vp]),
    "ldit_requant_train_mirror": (C.c_int, [C.POINTER(LditCfg), _vp, _vp, _sz, _vp, _vp]),
    "ldit_grads_accumulate_multi_f32": (C.c_int, [C.POINTER(LditAccSegment), _i32, _i32, _vp]),
    "ldit_adamw_ema_groups_multi_f32": (C.c_int, [C.POINTER(LditOptSegment), C.POINTER(LditOptHyper), C.POINTER(_vp), _i32, _vp, _vp, C.c_double,
                                                  C.c_double, _f32, C.c_double, _i32, _vp]),
    "ldit_swap_multi_f32": (C.c_int, [C.POINTER(LditSwapSegment), _i32, _vp]),
    # COCO box evaluation
    "ldit_coco_match": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i64, _vp]),
    "ldit_coco_keys": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp]),
    "ldit_coco_accumulate": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, C.POINTER(C.c_double), C.POINTER(_i32), _vp, _vp, _vp]),
    # box head
    "ldit_roi_align_levels_f32": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_f32), C.POINTER(_i64), C.POINTER(_i64),
                                            C.POINTER(_i64), _i32, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp]),
    "ldit_roi_align_levels_bf16": (C.c_int, [C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_f32), C.POINTER(_i64), C.POINTER(_i64),
                                             C.POINTER(_i64), _i32, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp]),
    "ldit_box_postprocess_f32": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _f32, _f32, C.POINTER(_f32), _f32, _f32, _vp, _vp, _vp, _vp]),
}

_lib = None


class LditError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libldit_hip: error {code}: {message}")
        self.code = code


def load() -> C.CDLL:
    """Load the library (once).  Raises if it is missing - there is no other implementation to fall back to."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `make -C layoutdit_amd/csrc` "
                              f"(or __graft_entry__.build()); layoutdit_amd has no CPU / eager fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        got = lib.ldit_abi_version()
        if got != LDIT_ABI_VERSION:
            raise ImportError(f"libldit_hip ABI {got} != expected {LDIT_ABI_VERSION}")
        _lib = lib
    return _lib


def set_switch(name: str, value) -> None:
    """Set (``value`` a string) or remove (``None``) one of the library's diagnostic ``LDIT_*`` environment switches and make
    the library re-read them: it reads its switches once, not per launch (``ldit_debug_reload_env``, include/ldit.h)."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    load().ldit_debug_reload_env()


def rpn_loss_workspace_bytes(batch: int, n: int) -> int:
    """Scratch bytes ``ldit_rpn_loss_f32`` wants for ``batch`` x ``n`` anchors (host arithmetic, no launch)."""
    return int(load().ldit_rpn_loss_workspace_bytes(batch, n))


def box_loss_workspace_bytes(rows: int) -> int:
    """Scratch bytes ``ldit_box_loss_f32`` wants for ``rows`` sampled rows (host arithmetic, no launch)."""
    return int(load().ldit_box_loss_workspace_bytes(rows))


def nms_workspace_bytes(problems: int, n: int) -> int:
    """Scratch bytes ``ldit_nms_batched_f32`` wants for ``problems`` x ``n`` candidates (host arithmetic, no launch)."""
    return int(load().ldit_nms_workspace_bytes(problems, n))


def grad_norm_partials(segs, S: int) -> int:
    """Partial sums ``ldit_grads_check_norm_multi_f32`` writes for a host array of ``S`` segments (host arithmetic, no launch)."""
    n = int(load().ldit_grad_norm_partials(segs, S))
    if n < 0:
        raise LditError(LDIT_EINVAL, load().ldit_last_error().decode(errors="replace"))
    return n


def check(rc: int) -> None:
    if rc != LDIT_OK:
        raise LditError(rc, load().ldit_last_error().decode(errors="replace"))
