"""ctypes binding of libsampt_hip.so (C ABI: include/sampt_hip.h).

The product path has NO fallback: if the shared library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsampt_hip.so")

c_void_p, c_int, c_size_t, c_float, c_char_p = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_char_p


class SamptError(RuntimeError):
    pass


ERR_CAPACITY = -5     # SAMPT_ERR_CAPACITY: more results than the capacity the caller gave


class VitConfigC(C.Structure):
    _fields_ = [("embed_dim", c_int), ("depth", c_int), ("num_heads", c_int), ("grid", c_int), ("window", c_int),
                ("patch", c_int), ("out_chans", c_int), ("mlp_ratio", c_int), ("img_size", c_int),
                ("global_mask", c_int), ("f16", c_int), ("pixel_mean", c_float * 3), ("pixel_std", c_float * 3)]


class TinyVitConfigC(C.Structure):
    _fields_ = [("img_size", c_int), ("out_chans", c_int), ("mlp_ratio", c_int), ("mbconv_expand_ratio", c_int),
                ("embed_dims", c_int * 4), ("depths", c_int * 4), ("num_heads", c_int * 4), ("window_sizes", c_int * 4),
                ("pixel_mean", c_float * 3), ("pixel_std", c_float * 3)]


# name -> (restype, argtypes); every symbol declared in include/sampt_hip.h
_P = c_void_p
_SIGS = {
    "sampt_version": (c_int, []),
    "sampt_last_error": (c_char_p, []),
    "sampt_pips_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, c_int, c_int, C.POINTER(_P)]),
    "sampt_pips_destroy": (None, [_P]),
    "sampt_pips_fnet_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_pips_fnet_f32": (c_int, [_P, _P, c_int, c_int, c_int, C.POINTER(_P), _P, c_size_t, _P]),
    "sampt_pips_sample_feat_f32": (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P]),
    "sampt_pips2_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, c_int, C.POINTER(_P)]),
    "sampt_pips2_destroy": (None, [_P]),
    "sampt_pips2_fnet_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_pips2_fnet_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, C.POINTER(_P), _P, c_size_t, _P]),
    "sampt_pips2_update_workspace_bytes": (c_int, [_P, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_pips2_update_f32": (c_int, [_P, C.POINTER(_P), c_int, c_int, _P, c_int, c_int, _P, c_int, C.POINTER(_P), c_int, _P,
                                       _P, c_size_t, _P]),
    "sampt_raft_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, C.POINTER(_P)]),
    "sampt_raft_destroy": (None, [_P]),
    "sampt_raft_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_raft_flows_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_raft_chain": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, _P, _P]),
    "sampt_raft_corr_pyramid_workspace_bytes": (c_size_t, [c_int, c_int]),
    "sampt_raft_corr_pyramid": (c_int, [_P, _P, c_int, c_int, C.POINTER(_P), _P, c_size_t, _P]),
    "sampt_raft_lookup": (c_int, [C.POINTER(_P), c_int, c_int, _P, C.c_long, _P, _P]),
    "sampt_raft_upsample": (c_int, [_P, _P, c_float, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "sampt_tapir_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, C.POINTER(_P)]),
    "sampt_tapir_destroy": (None, [_P]),
    "sampt_tapir_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_tapir_track_f32": (c_int, [_P, _P, c_int, _P, c_int, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_tapir_launches": (c_int, [_P]),
    "sampt_tapir_set_max_queries": (c_int, [_P, c_int]),
    "sampt_tapir_backbone_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_tapir_backbone_f32": (c_int, [_P, _P, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_tapir_query_feats_f32": (c_int, [_P, _P, c_int, _P, c_int, _P, _P]),
    "sampt_tapir_heads_f32": (c_int, [_P, c_int, _P, c_int, c_int, _P, c_int, C.POINTER(_P), _P, _P, _P, _P]),
    "sampt_tapir_patch_corr_f32": (c_int, [_P, _P, c_int, c_int, _P, _P, _P, _P, c_int, _P, c_int, _P]),
    "sampt_tapir_temporal_mix_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "sampt_tapir_gemm_f32": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "sampt_conv2d_same_nhwc": (c_int, [c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "sampt_instance_norm_affine_nhwc": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_float, c_int, _P, c_size_t, _P]),
    "sampt_tapnet_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, C.POINTER(_P)]),
    "sampt_tapnet_destroy": (None, [_P]),
    "sampt_tapnet_workspace_bytes": (c_int, [_P, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_tapnet_track_f32": (c_int, [_P, _P, c_int, _P, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_tapnet_launches": (c_int, [_P]),
    "sampt_tapnet_set_stem_chunk": (c_int, [_P, c_int]),
    "sampt_tapnet_backbone_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_tapnet_backbone_f32": (c_int, [_P, _P, c_int, _P, C.POINTER(_P), _P, c_size_t, _P]),
    "sampt_tapnet_bn_shift_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "sampt_tapnet_maxpool_nhwc": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "sampt_tapnet_query_feats_f32": (c_int, [_P, c_int, _P, c_int, _P, _P]),
    "sampt_tapnet_heads_f32": (c_int, [_P, c_int, _P, _P, c_int, C.POINTER(_P), _P, _P, _P]),
    "sampt_sg_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, C.POINTER(_P)]),
    "sampt_sg_destroy": (None, [_P]),
    "sampt_sg_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_size_t), C.POINTER(c_size_t)]),
    "sampt_sg_detect": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_float, c_int, c_int, _P, _P, _P, _P, C.POINTER(c_int), _P, _P,
                                c_size_t, _P]),
    "sampt_sg_match": (c_int, [_P, _P, _P, _P, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, _P, _P, _P,
                               c_size_t, _P]),
    "sampt_sg_nms_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sampt_sg_nms": (c_int, [_P, c_int, c_int, c_int, c_int, c_float, c_int, c_int, _P, _P, _P, C.POINTER(c_int), _P, c_size_t, _P]),
    "sampt_sg_sample_descriptors": (c_int, [_P, c_int, c_int, _P, c_int, _P, _P]),
    "sampt_sg_attention": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "sampt_sg_sinkhorn": (c_int, [_P, c_int, c_int, _P, c_int, _P, _P, _P]),
    "sampt_sg_mutual_match": (c_int, [_P, c_int, c_int, _P, _P, c_float, _P, _P, _P, c_size_t, _P]),
    "sampt_sg_select": (c_int, [_P, c_int, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "sampt_sg_gather": (c_int, [_P, _P, c_int, _P, c_int, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "sampt_cotracker_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, c_int, c_int, C.POINTER(_P)]),
    "sampt_cotracker_destroy": (None, [_P]),
    "sampt_resize_frames_f32": (c_int, [_P, c_int, C.c_long, c_int, c_int, _P, c_int, c_int, _P]),
    "sampt_cotracker_fnet_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_cotracker_fnet_f32": (c_int, [_P, _P, c_int, c_int, c_int, C.POINTER(_P), _P, c_size_t, _P]),
    "sampt_cotracker_track_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_cotracker_track_f32": (c_int, [_P, C.POINTER(_P), c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P, _P, c_int, _P, _P,
                                          _P, c_size_t, _P]),
    "sampt_pips_update_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_pips_update_f32": (c_int, [_P, C.POINTER(_P), c_int, c_int, _P, c_int, _P, _P, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_vit_create": (c_int, [C.POINTER(VitConfigC), C.POINTER(c_char_p), C.POINTER(_P), c_int, c_int, C.POINTER(_P)]),
    "sampt_vit_destroy": (None, [_P]),
    "sampt_vit_encode_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_vit_profile_begin": (c_int, [_P]),
    "sampt_vit_profile_end": (c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(c_int)]),
    "sampt_vit_encode": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_attention_t2i_workspace_bytes": (c_int, [c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_attention_t2i_f32": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, c_size_t, _P]),
    "sampt_vit_live_rows": (c_int, [_P, c_int, c_int, C.POINTER(c_int), C.POINTER(c_size_t)]),
    "sampt_vit_encode_live": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "sampt_tinyvit_create": (c_int, [C.POINTER(TinyVitConfigC), C.POINTER(c_char_p), C.POINTER(_P), c_int, c_int, C.POINTER(_P)]),
    "sampt_tinyvit_destroy": (None, [_P]),
    "sampt_tinyvit_encode_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_tinyvit_encode": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_tinyvit_encode_stages": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, C.POINTER(_P), C.POINTER(c_float), _P, c_size_t, _P]),
    "sampt_tinyvit_preprocess": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_float), C.POINTER(c_float), _P, _P]),
    "sampt_tinyvit_dwconv3x3_nhwc": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "sampt_tinyvit_window_attention_f32": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "sampt_dec_create": (c_int, [C.POINTER(c_char_p), C.POINTER(_P), c_int, c_int, c_int, c_int, c_int, C.POINTER(_P)]),
    "sampt_dec_hq_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_dec_hq_features": (c_int, [_P, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_dec_destroy": (None, [_P]),
    "sampt_dec_workspace_bytes": (c_int, [_P, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_dec_workspace_bytes_k": (c_int, [_P, c_int, c_int, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_sam_decode": (c_int, [_P, _P, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t,
                                 _P]),
    "sampt_sam_decode_multimask": (c_int, [_P, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_sam_decode_points_workspace_bytes": (c_int, [_P, c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_sam_decode_points": (c_int, [_P, c_int, _P, _P, _P, _P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_amg_score_workspace_bytes": (c_size_t, [c_int]),
    "sampt_amg_score": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.c_double, C.c_double, _P, _P, c_size_t, _P]),
    "sampt_amg_binarize": (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.c_double, _P, _P]),
    "sampt_amg_regions_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sampt_amg_regions": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_amg_nms_workspace_bytes": (c_size_t, [c_int]),
    "sampt_amg_nms": (c_int, [_P, _P, c_int, c_float, _P, _P, _P, c_size_t, _P]),
    "sampt_rle_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sampt_rle_count": (c_int, [_P, c_int, c_float, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_rle_emit": (c_int, [c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_rle_string_workspace_bytes": (c_size_t, [C.c_int64]),
    "sampt_rle_string_sizes": (c_int, [_P, _P, c_int, C.c_int64, _P, _P, c_size_t, _P]),
    "sampt_rle_string_emit": (c_int, [_P, _P, c_int, C.c_int64, _P, _P, _P, c_size_t, _P]),
    "sampt_jf_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "sampt_jf_counts": (c_int, [_P, c_int, c_float, _P, _P, _P, c_int, c_float, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P,
                                c_size_t, _P]),
    "sampt_jf_pairs_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "sampt_jf_pairs_counts": (c_int, [_P, c_int, c_float, _P, _P, c_int, _P, c_int, c_float, _P, _P, c_int, _P, _P, c_int, c_int, c_int,
                                      c_int, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_bits_pack": (c_int, [_P, c_int, c_float, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "sampt_rle_decode_workspace_bytes": (c_size_t, [C.c_int64]),
    "sampt_rle_decode_bits": (c_int, [_P, _P, c_int, C.c_int64, c_int, c_int, _P, _P, _P, _P, c_size_t, _P]),
    "sampt_bits_unpack": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "sampt_bits_row_prefix": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "sampt_bits_select": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, _P]),
    "sampt_seq_iou_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "sampt_seq_iou_counts": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "sampt_vis_match": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sampt_viz_band": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "sampt_viz_compose": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P, c_int, c_int, _P, _P]),
    "sampt_patch_filter": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, c_float, _P, c_int, _P, _P, _P]),
    "sampt_sam_track_decode": (c_int, [_P, c_int, _P, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, c_float, c_int, c_int, c_int,
                                       c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_sam_track_decode_graph": (c_int, [_P, c_int, _P, _P, _P, _P, c_int, _P, _P, c_int, c_int, c_int, c_float, c_int, c_int,
                                             c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_dec_graph_stats": (c_int, [_P, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "sampt_dec_set_batch_invariant": (c_int, [_P, c_int]),
    "sampt_gemm_f32_rows": (c_int, [_P, c_int, _P, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "sampt_gemm_f32_route": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int)]),
    "sampt_attn_t2i_plan": (c_int, [c_int, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int)]),
    "sampt_postprocess_masks": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, c_int, _P]),
    "sampt_bbox_workspace_bytes": (c_size_t, [c_int, c_int]),
    "sampt_bbox_from_logits": (c_int, [_P, c_int, c_int, _P, _P, c_size_t, _P]),
    "sampt_resize_logits": (c_int, [_P, c_int, c_int, c_int, _P, c_int, c_int, _P]),
    "sampt_pil_resample_u8": (c_int, [_P, _P, C.c_long, c_int, c_int, c_int, _P, _P, c_int, _P]),
    "sampt_index_masks": (c_int, [_P, c_int, C.c_long, _P, _P]),
    "sampt_vos_index_masks": (c_int, [_P, c_int, c_int, C.c_long, _P, _P, _P, _P]),
    "sampt_vos_index_masks_resized": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, c_int, c_int, _P, _P]),
    "sampt_gemm": (c_int, [c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "sampt_pips_track_workspace_bytes": (c_int, [_P, c_int, C.POINTER(c_size_t)]),
    "sampt_pips_track_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_float, c_int, _P, _P, _P, c_int,
                                     _P, _P, _P, c_size_t, _P, C.POINTER(c_int)]),
    "sampt_vit_set_gemm_workgroups": (c_int, [_P, c_int]),
    "sampt_vit_set_gemm_workgroups_kind": (c_int, [_P, c_int, c_int, c_int, c_int]),
    "sampt_vit_set_attention_head_major": (c_int, [_P, c_int]),
    "sampt_vit_calibrate": (c_int, [_P, _P, c_int]),
    "sampt_gemm_set_stagger": (c_int, [c_int]),
    "sampt_gemm_set_schedule": (c_int, [c_int]),
    "sampt_gemm_set_thin_min_wgs": (c_int, [c_int]),
    "sampt_conv_set_halo": (c_int, [c_int]),
    "sampt_gemm_set_wres": (c_int, [c_int]),
    "sampt_gemm_set_trim": (c_int, [c_int]),
    "sampt_prompt_count": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "sampt_prompt_fill": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, C.c_double, C.c_double, _P, c_int, c_int, _P, _P, _P,
                                  _P, _P]),
    "sampt_mark_outside_frame": (c_int, [_P, _P, C.c_long, c_int, c_int, _P, _P]),
    "sampt_move_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_int, c_int, c_int, c_void_p]),
    "sampt_fill_f32": (c_int, [c_void_p, c_size_t, c_float, c_void_p]),
    "sampt_conv_stem7x7": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
    "sampt_conv3x3_planes_instnorm_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float,
                                                    c_void_p, c_void_p, c_size_t, c_void_p]),
    "sampt_gemm_x3_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "sampt_gemm_x3_rows_epi": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "sampt_sam_mask_dot": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "sampt_pips_set_mixer": (c_int, [c_int, c_int]),
    "sampt_stream_create_cu_range": (c_int, [c_int, c_int, C.POINTER(_P)]),
    "sampt_stream_destroy": (c_int, [_P]),
    "sampt_pips_round_launches": (c_int, [_P]),
    "sampt_pips_mix_mlp_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "sampt_pips_mix_xop_halves": (c_size_t, [c_int]),
    "sampt_pips_mix_pre_f32": (c_int, [_P, c_int, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sampt_pips_mix_mlp_x3": (c_int, [_P, _P, _P, _P, c_int, c_int, _P]),
    "sampt_pips_mix_reduce_f32": (c_int, [_P, c_int, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sampt_gemm_ex": (c_int, [c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, c_int, c_int, _P]),
    "sampt_gemm_f16_p8": (c_int, [c_int, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                  c_int, c_int, _P]),
    "sampt_gemm_f16_p8_plan": (c_int, [c_int, c_int, c_int, c_int, C.POINTER(c_int), C.POINTER(c_int), C.POINTER(c_int)]),
    "sampt_conv2d_nhwc": (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "sampt_instance_norm_nhwc": (c_int, [_P, c_int, c_int, c_int, c_float, c_int, _P, _P, c_size_t, _P]),
    "sampt_instance_norm_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "sampt_layernorm": (c_int, [_P, _P, _P, _P, c_int, c_int, c_float, c_int, c_int, _P]),
    "sampt_resize_bilinear_nhwc": (c_int, [_P, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "sampt_avgpool2x2_nhwc": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "sampt_corr_sample_f32": (c_int, [C.POINTER(_P), c_int, c_int, _P, c_int, c_int, _P, _P, _P, _P]),
    "sampt_pips_corr_sample_ex": (c_int, [C.POINTER(_P), c_int, c_int, _P, c_int, c_int, _P, _P, _P, c_int, c_int, _P, _P]),
    "sampt_pips_build_input_f32": (c_int, [_P, _P, _P, c_int, c_int, _P, c_int, _P]),
    "sampt_pips_init_state_f32": (c_int, [_P, _P, c_float, c_int, c_int, _P, _P, _P, _P]),
    "sampt_pips_apply_update_f32": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "sampt_pips_finalize_f32": (c_int, [_P, _P, _P, _P, c_float, c_int, c_int, _P, _P, _P]),
    "sampt_pips_chain_init": (c_int, [_P, c_int, c_int, _P, _P, _P, _P]),
    "sampt_pips_round_begin": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, c_float, _P]),
    "sampt_pips_round_end": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_float, _P, _P, _P, _P]),
    "sampt_pips2_init_f32": (c_int, [_P, _P, c_int, c_int, _P, c_float, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "sampt_pips2_templates_f32": (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, _P, _P, _P]),
    "sampt_pips2_build_input_f32": (c_int, [_P, _P, c_int, c_int, _P, c_int, _P]),
    "sampt_instnorm1d_relu_f32": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "sampt_add_chanpad_f32": (c_int, [_P, _P, C.c_long, c_int, c_int, c_int, _P]),
    "sampt_pips2_apply_delta_f32": (c_int, [_P, _P, c_float, c_int, c_int, c_int, _P, _P, _P]),
    "sampt_cot_prepare": (c_int, [_P, _P, _P, c_float, c_int, c_int, _P, _P, _P, _P, _P]),
    "sampt_cot_window_init": (c_int, [c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sampt_cot_pos_embed_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "sampt_cot_build_input_f32": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, _P, _P]),
    "sampt_cot_window_store_f32": (c_int, [_P, _P, _P, _P, c_float, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P]),
    "sampt_attention_f32": (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "sampt_cotracker_attention_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "sampt_vit_attention_f16": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "sampt_vit_attention_f16_head_major": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P]),
    "sampt_gemm_f16_head_major": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "sampt_vit_attention_x3": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "sampt_split_rows_x3": (c_int, [_P, _P, c_int, c_int, _P]),
    "sampt_vit_window_attention": (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P]),
    "sampt_kmedoids_rowsums_f64": (c_int, [_P, c_int, _P, _P]),
    "sampt_kmedoids_alternate": (c_int, [_P, c_int, c_int, _P, c_int, _P, _P]),
    "sampt_dbscan_workspace_bytes": (c_size_t, [c_int]),
    "sampt_dbscan_labels": (c_int, [_P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    "sampt_dbscan_largest": (c_int, [_P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "sampt_int_frame_state": (c_int, [_P, _P, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, _P]),
    "sampt_qp_corners_workspace_bytes": (c_int, [c_int, c_int, C.POINTER(c_size_t)]),
    "sampt_qp_erode_u8": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P]),
    "sampt_qp_shi_tomasi": (c_int, [_P, _P, c_int, c_int, c_int, c_float, _P, _P, _P, c_size_t, _P]),
}

_lib = None


def exported_symbols() -> List[str]:
    return list(_SIGS)


def load():
    """Load the HIP library; raises SamptError if it has not been built (`python -c 'import __graft_entry__ as g; g.build()'`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SamptError(f"{LIB_PATH} not found: build it with `make -C sam_pt_amd/csrc` "
                         "(there is no CPU or PyTorch fallback for the SAM-PT hot path)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    if os.environ.get("SAMPT_GEMM_SCHED"):            # A / B switch of the 8-phase GEMM's stage schedule (sampt_gemm_set_schedule)
        lib.sampt_gemm_set_schedule(int(os.environ["SAMPT_GEMM_SCHED"]))
    if os.environ.get("SAMPT_PIPS_MIXER") or os.environ.get("SAMPT_PIPS_MIXER_WGS"):   # csrc/pips_mixer.hip (A / B runs)
        lib.sampt_pips_set_mixer(int(os.environ.get("SAMPT_PIPS_MIXER", "2")), int(os.environ.get("SAMPT_PIPS_MIXER_WGS", "16")))
    if os.environ.get("SAMPT_GEMM_TRIM"):              # A / B switch of the persistent GEMM's workgroup trimming (sampt_gemm_set_trim)
        lib.sampt_gemm_set_trim(int(os.environ["SAMPT_GEMM_TRIM"]))
    if os.environ.get("SAMPT_GEMM_WRES"):              # A / B switch of csrc/gemm_x3_wres.hip (sampt_gemm_set_wres)
        lib.sampt_gemm_set_wres(int(os.environ["SAMPT_GEMM_WRES"]))
    if os.environ.get("SAMPT_CONV_HALO"):              # A / B switch of csrc/conv_halo_x3.hip (sampt_conv_set_halo)
        lib.sampt_conv_set_halo(int(os.environ["SAMPT_CONV_HALO"]))
    if os.environ.get("SAMPT_THIN_MIN_WGS"):          # thin f32 GEMM: tile growth threshold (sampt_gemm_set_thin_min_wgs)
        lib.sampt_gemm_set_thin_min_wgs(int(os.environ["SAMPT_THIN_MIN_WGS"]))
    if os.environ.get("SAMPT_GEMM_STAGGER"):          # experiment knob of the 8-phase GEMM (sampt_gemm_set_stagger)
        lib.sampt_gemm_set_stagger(int(os.environ["SAMPT_GEMM_STAGGER"]))
    _lib = lib
    return lib


def require_hip(device, who: str):
    """The hot path has no CPU / PyTorch fallback: anything but a HIP device is an error."""
    if getattr(device, "type", None) != "cuda":
        raise SamptError(f"{who} runs on the HIP device only (no CPU fallback); got {device}")


def check(rc: int, what: str):
    if rc != 0:
        msg = load().sampt_last_error()
        raise SamptError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """torch's current stream ON `device` (default: the current device — inside ``device_guard`` that is the guarded one)."""
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def cu_range_stream(device, cu_lo: int, cu_hi: int) -> "torch.cuda.Stream":
    """A torch stream on `device` confined to CUs [cu_lo, cu_hi) of every XCD (sampt_stream_create_cu_range).  The HIP stream lives
    as long as the process (a handful per model; the runtime frees them at exit)."""
    h = c_void_p()
    with device_guard(device):
        check(load().sampt_stream_create_cu_range(int(cu_lo), int(cu_hi), C.byref(h)), "sampt_stream_create_cu_range")
    return torch.cuda.ExternalStream(h.value, device=device)


def device_guard(device):
    """The library launches on the HIP *current* device and never calls hipSetDevice itself, and ``stream_ptr()`` is
    torch's current stream of the current device: every public entry point of the package runs inside this guard so that a
    model living on cuda:N works whatever the caller's current device is (``SamHip().to('cuda:1')`` without
    ``set_device``, gloo-initialised multi-GPU processes)."""
    if device is not None and getattr(device, "type", None) == "cuda":
        return torch.cuda.device(device)
    return contextlib.nullcontext()


def on_device(get_device):
    """Decorator form of ``device_guard``: ``get_device(self, *args, **kwargs)`` names the device of the call."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapper(self, *args, **kwargs):
            with device_guard(get_device(self, *args, **kwargs)):
                return fn(self, *args, **kwargs)
        return wrapper
    return deco


def name_table(named: Dict[str, torch.Tensor]):
    """(names array, ptrs array, n) for the *_create functions; keeps the byte strings alive."""
    keys = list(named)
    names = (c_char_p * len(keys))(*[k.encode() for k in keys])
    ptrs = (_P * len(keys))(*[named[k].data_ptr() for k in keys])
    return names, ptrs, len(keys)


def ptr_array(ts: Sequence[torch.Tensor]):
    return (_P * len(ts))(*[t.data_ptr() for t in ts])


# ----------------------------------------------------------------------------------------------------------------------
# what the wrappers above the C ABI share: workspace queries, the chunk plan of a bounded workspace, engine lifetime
# (load / check / require_hip / device_guard / name_table are looked up as module attributes when a helper RUNS, so that a
# test double installed over them is what the helpers see)
# ----------------------------------------------------------------------------------------------------------------------
def workspace_bytes(name: str, *args) -> int:
    """Bytes a ``*_workspace_bytes`` query of the C ABI reports, in either of its two forms: the size is the result, or the
    result is a return code and the size comes back through a trailing ``size_t *`` (appended here, after ``args``)."""
    res, argtypes = _SIGS[name]
    fn = getattr(load(), name)
    if res is c_size_t:
        return int(fn(*args))
    if not argtypes or argtypes[-1] != C.POINTER(c_size_t):
        raise SamptError(f"{name} is not a workspace query")
    n = c_size_t()
    check(fn(*args, C.byref(n)), name)
    return n.value


def workspace(name: str, device, *args, min_bytes: int = 16) -> torch.Tensor:
    """The uint8 scratch tensor on ``device`` that the query ``name(*args)`` asks for (``workspace_bytes``), never smaller than
    ``min_bytes`` so that an empty problem still has a buffer to point at."""
    return torch.empty(max(min_bytes, workspace_bytes(name, *args)), dtype=torch.uint8, device=device)


def chunk_plan(per: int, n: int, given_bytes: Optional[int], cap: int, who: str, h: int, w: int,
               max_chunk: Optional[int] = None) -> Tuple[int, int]:
    """(workspace bytes, items per call) for ``n`` items that need ``per`` scratch bytes each: everything at once up to ``cap``
    bytes unless the caller bounds the workspace, then chunks of as many items as fit (and at most ``max_chunk``).  Less than
    one item's worth still plans one item per call: the native call itself refuses that workspace."""
    if per == 0:
        raise SamptError(f"{who}: h * w must be below 2^31; got {h} x {w}")
    nbytes = max(per, min(n * per, cap)) if given_bytes is None else int(given_bytes)
    chunk = max(1, min(n, nbytes // per))
    if max_chunk is not None:
        chunk = max(1, min(chunk, max_chunk))
    return nbytes, chunk


def create_engine(lib, symbol: str, weights: Dict[str, torch.Tensor], *args, pre=()):
    """One ``sampt_*_create(*pre, names, ptrs, n, *args, &handle)`` over the packed ``weights`` -> the handle."""
    names, ptrs, n = name_table(weights)
    h = c_void_p()
    check(getattr(lib, symbol)(*pre, names, ptrs, n, *args, C.byref(h)), symbol)
    return h


class EngineOwner:
    """Lifetime of the native engines behind one Python object.  A subclass lists ``_engines`` — one (handle attribute, destroy
    symbol) per engine — and names the attribute that records the device; handles, device and ``_lib`` stay plain attributes."""
    _engines: Tuple[Tuple[str, str], ...] = ()
    _engine_device = "_device"
    engines_destroyed = 0              # handles this object has given back to the library so far

    def ensure_engines(self, device, who: str, build):
        """Engines on ``device``: nothing to do when they are there already, else ``build(lib, device)`` packs the weights,
        calls the ``*_create`` functions and returns one handle per entry of ``_engines``.  Engines of another device (or of a
        forgotten one, ``forget_engine_device``) are destroyed first, after that device's work has finished."""
        old = getattr(self, self._engine_device, None)
        live = any(getattr(self, attr, None) is not None for attr, _ in self._engines)
        if live and old == device:
            return
        require_hip(device, who)
        lib = self._lib = load()                  # (before ``build``: a handle of a build that fails half-way can still be destroyed)
        if live:
            old = device if old is None else old
            with device_guard(old):
                if getattr(old, "type", None) == "cuda":
                    torch.cuda.synchronize(old)
                self._destroy_engines(lib)
            self.on_replace()
        for (attr, _), h in zip(self._engines, build(lib, device)):
            setattr(self, attr, h)
        setattr(self, self._engine_device, device)

    def forget_engine_device(self):
        """The next ``ensure_engines`` replaces the engines even on the same device (they are destroyed there, after its work)."""
        setattr(self, self._engine_device, None)

    def on_replace(self):
        """Hook: the old engines are gone — drop whatever was cached for them."""

    def _destroy_engines(self, lib):
        for attr, destroy in self._engines:
            h = getattr(self, attr, None)
            if h is not None:
                getattr(lib, destroy)(h)
                setattr(self, attr, None)
                self.engines_destroyed += 1

    def __del__(self):
        try:
            self._destroy_engines(self._lib)
        except Exception:
            pass
