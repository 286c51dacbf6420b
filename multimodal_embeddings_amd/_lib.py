"""ctypes binding of libmme.so (include/mme.h).  Fails loudly: there is no CPU fallback.

Only this module touches the C ABI; the host mirrors of the reference interface
(embedder.py, cross_compare.py, weighted_region_clustering.py) go through `Engine`.
torch is used for device memory and streams only (data_ptr() into the ABI).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

from .staging import packed_layout
from .weights import (CLIP_ACTS, dinov2_geometry_problem, infer_dinov2_geometry, infer_vit_geometry, siglip_geometry_problem,
                      siglip_text_geometry_problem)

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library is the in-tree libmme.so.  Measurement tools load libmme_diag.so (build.py --diag: the only build
# that reads the experiment switches of DESIGN.md 4.5) by naming it in MME_LIB_PATH AND opting in with
# MME_ALLOW_LIB_OVERRIDE=1 (tools/_diag.py sets both): one stray variable in a user's environment must not be able to
# swap the library -- load_library refuses the override without the opt-in, and says so on stderr when a diagnostic
# build is what got loaded.
DEFAULT_LIB_PATH = os.path.join(_HERE, "libmme.so")
LIB_PATH = os.environ.get("MME_LIB_PATH") or DEFAULT_LIB_PATH
DIAG_LIB_PATH = os.path.join(_HERE, "libmme_diag.so")

NUM_KERNEL_CLASSES = 10
ABI_VERSION = 2  # include/mme.h MME_ABI_VERSION this binding was written against
KERNEL_CLASSES = ("preprocess", "gemm", "layernorm", "attention", "pool", "cosine", "page_reduce", "cluster", "neighbours", "allgather")


class MmeError(RuntimeError):
    pass


class _Layer(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in (
        "ln1_g", "ln1_b", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "o_w", "o_b",
        "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class _Weights(C.Structure):
    _fields_ = [
        ("image_size", C.c_int32), ("patch_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32),
        ("heads", C.c_int32), ("mlp", C.c_int32), ("ln_eps", C.c_float),
        ("cls_token", C.POINTER(C.c_float)), ("pos_emb", C.POINTER(C.c_float)),
        ("patch_w", C.POINTER(C.c_float)), ("patch_b", C.POINTER(C.c_float)),
        ("lnf_g", C.POINTER(C.c_float)), ("lnf_b", C.POINTER(C.c_float)),
        ("layer", C.POINTER(_Layer)),
    ]


class _ClipWeights(C.Structure):  # mme_clip_weights
    _fields_ = [("vit", _Weights), ("pre_g", C.POINTER(C.c_float)), ("pre_b", C.POINTER(C.c_float)), ("proj_w", C.POINTER(C.c_float)),
                ("proj_dim", C.c_int32), ("act", C.c_int32)]


class _ClipTextWeights(C.Structure):  # mme_clip_text_weights
    _fields_ = [(n, C.c_int32) for n in ("hidden", "layers", "heads", "mlp", "vocab", "max_positions", "proj_dim", "act", "eos_token_id")] + [
        ("ln_eps", C.c_float)] + [(n, C.POINTER(C.c_float)) for n in ("token_emb", "pos_emb", "lnf_g", "lnf_b", "proj_w")] + [("layer", C.POINTER(_Layer))]


class _TextApplyArgs(C.Structure):  # mme_text_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("tok", "pos", "ids_host", "x", "qkv", "out", "gamma", "beta", "eos_pos_host", "y", "y_f32")] + [
        ("n", C.c_int32), ("d", C.c_int32), ("heads", C.c_int32), ("vocab", C.c_int32), ("eps", C.c_float)]


class _SiglipTextWeights(C.Structure):  # mme_siglip_text_weights
    _fields_ = [(n, C.c_int32) for n in ("hidden", "layers", "heads", "mlp", "vocab", "max_positions", "projection_size", "pad_token_id", "has_logits")] + [
        (n, C.c_float) for n in ("ln_eps", "logit_scale", "logit_bias")] + [
        (n, C.POINTER(C.c_float)) for n in ("token_emb", "pos_emb", "lnf_g", "lnf_b", "head_w", "head_b")] + [("layer", C.POINTER(_Layer))]


class _SiglipTextApplyArgs(C.Structure):  # mme_siglip_text_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("tok", "pos", "ids_host", "x", "qkv", "out", "gamma", "beta", "y", "y_f32", "acc", "bias", "emb_f32", "emb_bf16",
                                          "cos", "scores")] + [("count", C.c_int64)] + [
        (n, C.c_int32) for n in ("n", "d", "heads", "vocab", "only_block", "p")] + [(n, C.c_float) for n in ("eps", "logit_scale", "logit_bias")]


class _TileLayer(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("ln1_g", "ln1_b", "q_w", "k_w", "v_w", "o_w", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")] + [
        ("gate_attn", C.c_float), ("gate_ffn", C.c_float), ("gated", C.c_int32)]


class _TileWeights(C.Structure):
    _fields_ = [
        ("image_size", C.c_int32), ("patch_size", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32), ("mlp", C.c_int32),
        ("max_tiles", C.c_int32), ("aspect_ratios", C.c_int32), ("layers", C.c_int32), ("global_layers", C.c_int32),
        ("n_intermediate", C.c_int32), ("intermediate", C.c_int32 * 8), ("intermediate_save_point", C.c_int32), ("norm_eps", C.c_float),
        ("pos_gate", C.c_float), ("pre_gate", C.c_float), ("post_gate", C.c_float),
        ("class_embedding", C.POINTER(C.c_float)), ("patch_w", C.POINTER(C.c_float)), ("pos_emb", C.POINTER(C.c_float)),
        ("tile_pos_emb", C.POINTER(C.c_float)), ("pre_emb", C.POINTER(C.c_float)), ("post_emb", C.POINTER(C.c_float)),
        ("ln_pre_g", C.POINTER(C.c_float)), ("ln_pre_b", C.POINTER(C.c_float)), ("ln_post_g", C.POINTER(C.c_float)), ("ln_post_b", C.POINTER(C.c_float)),
        ("layer", C.POINTER(_TileLayer)),
    ]


class _MllamaLMLayer(C.Structure):  # mme_mllama_lm_layer
    _fields_ = [("cross", C.c_int32), ("attn_gate", C.c_float), ("mlp_gate", C.c_float)] + [
        (n, C.POINTER(C.c_float)) for n in ("ln1", "ln2", "q_w", "k_w", "v_w", "o_w", "q_norm", "k_norm", "gate_w", "up_w", "down_w")]


class _MllamaLMWeights(C.Structure):  # mme_mllama_lm_weights
    _fields_ = [(n, C.c_int32) for n in ("hidden", "heads", "kv_heads", "intermediate", "layers", "vocab", "vision_dim", "image_token_id", "hidden_act",
                                         "rope_type", "rope_original_max")] + [
        (n, C.c_float) for n in ("rms_eps", "rope_theta", "rope_factor", "rope_low_freq_factor", "rope_high_freq_factor")] + [
        (n, C.POINTER(C.c_float)) for n in ("embed_tokens", "norm", "proj_w", "proj_b")] + [("layer", C.POINTER(_MllamaLMLayer))]


class _MllamaApplyArgs(C.Structure):  # mme_mllama_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("tok", "ids_host", "len_host", "xmask_host", "x", "y", "kv", "w", "cos", "sin", "rowzero", "emb_f32", "emb_bf16")] + [
        ("rows", C.c_int64), ("ld", C.c_int64)] + [(n, C.c_int32) for n in ("n", "S", "d", "heads", "kv_heads", "col0", "vocab", "tiles", "tokens")] + [
        ("eps", C.c_float)]


class _GemmApplyArgs(C.Structure):  # mme_gemm_apply_args
    _fields_ = [
        ("epilogue", C.c_int32), ("variant", C.c_int32), ("reverse_m", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int64), ("res", C.c_void_p),
        ("pos", C.c_void_p), ("pos_rows", C.c_int64), ("outf", C.c_void_p), ("ldf", C.c_int64), ("ln_stats", C.c_void_p),
        ("colsum", C.c_void_p), ("ln_part", C.c_void_p), ("ln_part_rows", C.c_int64), ("ln_part_floats", C.c_int64),
    ]


class _RowopApplyArgs(C.Structure):  # mme_rowop_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("x", "y", "gamma", "beta", "stats", "part", "cls", "pos", "emb_f32", "emb_bf16")] + [
        (n, C.c_int64) for n in ("rows", "row0", "row1", "stride", "part_rows", "part_floats")] + [
        ("d", C.c_int32), ("B", C.c_int32), ("tok", C.c_int32), ("eps", C.c_float)]


class _PoolApplyArgs(C.Structure):  # mme_pool_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("x", "gamma", "beta", "grids", "emb_f32", "emb_bf16")] + [
        (n, C.c_int32) for n in ("B", "tokens", "g", "first", "d")] + [("eps", C.c_float)]


class _SelectApplyArgs(C.Structure):  # mme_select_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("qsim", "group", "idx_out", "sim_out", "run_if", "cand_val", "cand_idx", "len", "A", "W", "thr", "cand_count",
                                          "overflow")] + [("ld", C.c_int64)] + [
        (n, C.c_int32) for n in ("N", "nrows", "row0", "fetch", "top_n", "keep_self", "cap", "M", "K", "thr_stride")] + [
        ("min_sim", C.c_float), ("max_sim", C.c_float)]


class _ClipApplyArgs(C.Structure):  # mme_clip_apply_args
    _fields_ = [("gemm", C.POINTER(_GemmApplyArgs))] + [(n, C.c_void_p) for n in ("x", "gamma", "beta", "stats", "y", "xf", "y_f32", "y_bf16")] + [
        ("rows", C.c_int64), ("d", C.c_int32), ("B", C.c_int32), ("tok", C.c_int32), ("p", C.c_int32), ("eps", C.c_float),
        ("ran_256", C.POINTER(C.c_int32))]


class _Vit32ApplyArgs(C.Structure):  # mme_vit32_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("src", "dst", "acc", "bias", "pos", "cls", "x", "qkv", "out", "gamma", "beta", "y", "emb_f32", "emb_bf16")] + [
        (n, C.c_int32) for n in ("n", "d", "heads", "only_block", "tok")] + [("eps", C.c_float)]


class _SiglipWeights(C.Structure):  # mme_siglip_weights
    _fields_ = [("vit", _Weights), ("probe", C.POINTER(C.c_float)), ("head", _Layer)]


class _Dinov2Scale(C.Structure):  # mme_dinov2_scale
    _fields_ = [("lambda1", C.POINTER(C.c_float)), ("lambda2", C.POINTER(C.c_float))]


class _Dinov2Weights(C.Structure):  # mme_dinov2_weights
    _fields_ = [("vit", _Weights), ("scale", C.POINTER(_Dinov2Scale))]


class _Dinov2ApplyArgs(C.Structure):  # mme_dinov2_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("src", "dst", "acc", "bias", "pos", "cls", "x", "qkv", "out", "gamma", "beta", "emb_f32", "emb_bf16", "w", "factor",
                                          "prepared")] + [("rows", C.c_int64), ("cols", C.c_int64)] + [
        (n, C.c_int32) for n in ("n", "d", "heads", "only_block", "tok", "dtype")] + [("eps", C.c_float)]


class _SiglipApplyArgs(C.Structure):  # mme_siglip_apply_args
    _fields_ = [("gemm", C.POINTER(_GemmApplyArgs)), ("ran_256", C.POINTER(C.c_int32))] + [
        (n, C.c_void_p) for n in ("acc", "bias", "pos", "x", "kv", "q", "out", "emb_f32", "emb_bf16")] + [(n, C.c_int32) for n in ("n", "d", "heads")]


class _TileRowopApplyArgs(C.Structure):  # mme_tile_rowop_apply_args
    _fields_ = [(n, C.c_void_p) for n in ("pv", "patches", "pemb", "cls", "pre", "pos", "tilepos", "gamma", "beta", "post", "aid", "x", "inter", "hidden",
                                          "emb_f32", "emb_bf16")] + [
        (n, C.c_int64) for n in ("npatch", "rows", "out_rows", "inter_stride")] + [
        ("n", C.c_int32), ("ni", C.c_int32), ("aspect_rows", C.c_int32), ("eps", C.c_float)]


class _WeightPrepApplyArgs(C.Structure):  # mme_weight_prep_apply_args
    _fields_ = [
        ("dtype", C.c_int32), ("scaled", C.c_int32), ("out_bf16", C.c_int32), ("scale", C.c_float), ("src", C.c_void_p), ("dst", C.c_void_p),
        ("count", C.c_int64), ("rows", C.c_int32), ("cols_padded", C.c_int32), ("cols", C.c_int32), ("nsrc", C.c_int32),
        ("w", C.c_void_p * 3), ("b", C.c_void_p * 3), ("src_rows", C.c_int64 * 3), ("src_scale", C.c_float * 3), ("src_scaled", C.c_int32 * 3),
        ("gamma", C.c_void_p), ("beta", C.c_void_p), ("wf", C.c_void_p), ("cs", C.c_void_p), ("bf", C.c_void_p),
    ]


class _DupState(C.Structure):  # mme_dup_state
    _fields_ = [
        ("parent", C.c_void_p), ("degree", C.c_void_p), ("best", C.c_void_p), ("page_pairs", C.c_void_p), ("edges", C.c_void_p),
        ("edge_sim", C.c_void_p), ("counters", C.c_void_p), ("edge_cap", C.c_int64), ("P", C.c_int32),
    ]


class _DensityState(C.Structure):  # mme_density_state
    _fields_ = [(f, C.c_void_p) for f in ("count", "parent", "border", "counters")]


_HIERARCHY_FIELDS = ("core", "comp", "row_key", "parent", "comp_weight", "comp_edge", "edges", "weights", "counters")


class _HierarchyState(C.Structure):  # mme_hierarchy_state
    _fields_ = [(f, C.c_void_p) for f in _HIERARCHY_FIELDS]


class _KmeansState(C.Structure):  # mme_kmeans_state
    _fields_ = [(f, C.c_void_p) for f in ("centroids", "sums", "counts", "labels", "sim", "info", "objective")]


class _KmeansApplyArgs(C.Structure):  # mme_kmeans_apply_args
    _fields_ = [
        ("qsim", C.c_void_p), ("ld", C.c_int64), ("emb", C.c_void_p), ("centroids", C.c_void_p), ("N", C.c_int32), ("d", C.c_int32),
        ("k", C.c_int32), ("chunk_rows", C.c_int32), ("labels", C.c_void_p), ("sim", C.c_void_p), ("moved", C.c_void_p),
        ("run_if", C.c_void_p), ("sums", C.c_void_p), ("counts", C.c_void_p),
    ]


class _ResizeSpec(C.Structure):  # mme_resize_spec
    _fields_ = [(f, C.c_int32) for f in ("mode", "height", "width", "resample")]


class _K1Rule(C.Structure):  # mme_k1_rule
    _fields_ = [("kind", C.c_int32), ("spec", _ResizeSpec), ("tile", C.c_int32), ("max_tiles", C.c_int32)]


K1_RECORD_INT32 = ("new_h", "new_w", "top", "left", "r0", "nr", "th", "tw", "h_pass", "v_pass", "gh", "kv", "h_class", "band_rows", "n_bands", "h_lds", "v_lds",
                   "refused")
K1_RECORD_INT64 = ("tab_off", "tab_bytes", "tmp_off", "tmp_bytes")
# mme_k1_record as a numpy record: 18 int32 then 4 int64 (72 bytes in: the int64 fields are naturally aligned)
K1_RECORD = np.dtype([(f, np.int32) for f in K1_RECORD_INT32] + [(f, np.int64) for f in K1_RECORD_INT64], align=True)
K1_REFUSALS = {0: None, 1: "size", 2: "tile_taps", 3: "h_lds", 4: "v_taps"}  # MME_K1_REFUSED_*


class _SilhouetteOut(C.Structure):  # mme_silhouette_out
    _fields_ = [(f, C.c_void_p) for f in ("sample", "cluster", "score", "info", "sums", "counts")]


EXPORTS = {
    "mme_abi_version": (C.c_int, []),
    "mme_is_diag_build": (C.c_int, []),
    "mme_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "mme_destroy": (None, [C.c_void_p]),
    "mme_last_error": (C.c_char_p, [C.c_void_p]),
    "mme_load_vit": (C.c_int, [C.c_void_p, C.POINTER(_Weights)]),
    "mme_vit_geometry": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_load_vit_as": (C.c_int, [C.c_void_p, C.POINTER(_Weights), C.c_int, C.c_void_p]),
    "mme_load_clip": (C.c_int, [C.c_void_p, C.POINTER(_ClipWeights)]),
    "mme_load_clip_as": (C.c_int, [C.c_void_p, C.POINTER(_ClipWeights), C.c_int, C.c_void_p]),
    "mme_encoder_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_clip_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_ClipApplyArgs), C.c_void_p]),
    "mme_vit32_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_Vit32ApplyArgs), C.c_void_p]),
    "mme_load_dinov2": (C.c_int, [C.c_void_p, C.POINTER(_Dinov2Weights)]),
    "mme_load_dinov2_as": (C.c_int, [C.c_void_p, C.POINTER(_Dinov2Weights), C.c_int, C.c_void_p]),
    "mme_dinov2_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_Dinov2ApplyArgs), C.c_void_p]),
    "mme_load_siglip": (C.c_int, [C.c_void_p, C.POINTER(_SiglipWeights)]),
    "mme_load_siglip_as": (C.c_int, [C.c_void_p, C.POINTER(_SiglipWeights), C.c_int, C.c_void_p]),
    "mme_siglip_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_SiglipApplyArgs), C.c_void_p]),
    "mme_load_clip_text": (C.c_int, [C.c_void_p, C.POINTER(_ClipTextWeights)]),
    "mme_load_clip_text_as": (C.c_int, [C.c_void_p, C.POINTER(_ClipTextWeights), C.c_int, C.c_void_p]),
    "mme_text_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_text_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_text_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_TextApplyArgs), C.c_void_p]),
    "mme_load_siglip_text": (C.c_int, [C.c_void_p, C.POINTER(_SiglipTextWeights)]),
    "mme_load_siglip_text_as": (C.c_int, [C.c_void_p, C.POINTER(_SiglipTextWeights), C.c_int, C.c_void_p]),
    "mme_text_geometry": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_siglip_scores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "mme_siglip_text_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_SiglipTextApplyArgs), C.c_void_p]),
    "mme_weights_fingerprint": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "mme_weights_read": (C.c_int64, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "mme_weight_prep_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_WeightPrepApplyArgs), C.c_void_p]),
    "mme_set_normalisation": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mme_normalisation_form": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "mme_set_resize_rule": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_resize_rule": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_set_resize_spec": (C.c_int, [C.c_void_p, C.POINTER(_ResizeSpec)]),
    "mme_get_resize_spec": (C.c_int, [C.c_void_p, C.POINTER(_ResizeSpec)]),
    "mme_set_chunk": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_set_gemm_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_set_ln_fusion": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_set_attention_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_attention_redone": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_attention_redone_n": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "mme_attention_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                      C.POINTER(C.c_int32), C.c_void_p]),
    "mme_set_forward_pruning": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_set_tile_order": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_preprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "mme_vit_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_vit_tokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_embed_tokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mme_set_pooling": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_pooling": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_pool_grid": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "mme_pool_grids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mme_k1_plan": (C.c_int, [C.POINTER(_K1Rule), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "mme_vit_forward_grids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_pool_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_PoolApplyArgs), C.c_void_p]),
    "mme_normalise_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mme_cosine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mme_cosine_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mme_page_similarity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "mme_page_similarity_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int, C.c_int, C.c_double, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "mme_cluster_pages": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_preprocess_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "mme_crop_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_lanczos_tables": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "mme_lanczos_workspace": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "mme_lanczos_resize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                     C.c_void_p]),
    "mme_nms_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_neighbours": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_set_neighbour_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_duplicates_init": (C.c_int, [C.c_void_p, C.POINTER(_DupState), C.c_int, C.c_void_p]),
    "mme_duplicates_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                      C.POINTER(_DupState), C.c_void_p]),
    "mme_duplicates_merge": (C.c_int, [C.c_void_p, C.POINTER(_DupState), C.POINTER(_DupState), C.c_int, C.c_void_p]),
    "mme_duplicates_finish": (C.c_int, [C.c_void_p, C.POINTER(_DupState), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_density_init": (C.c_int, [C.c_void_p, C.POINTER(_DensityState), C.c_int, C.c_void_p]),
    "mme_density_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.POINTER(_DensityState), C.c_void_p]),
    "mme_density_link": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(_DensityState),
                                   C.c_void_p]),
    "mme_density_finish": (C.c_int, [C.c_void_p, C.POINTER(_DensityState), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "mme_hierarchy_init": (C.c_int, [C.c_void_p, C.POINTER(_HierarchyState), C.c_int, C.c_void_p]),
    "mme_hierarchy_core": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_HierarchyState), C.c_void_p]),
    "mme_hierarchy_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(_HierarchyState), C.c_void_p]),
    "mme_hierarchy_merge": (C.c_int, [C.c_void_p, C.POINTER(_HierarchyState), C.c_int, C.c_void_p]),
    "mme_kmeans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(_KmeansState), C.c_void_p]),
    "mme_kmeans_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_KmeansApplyArgs), C.c_void_p]),
    "mme_silhouette": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(_SilhouetteOut), C.c_void_p]),
    "mme_silhouette_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "mme_moments_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_gemm_bench": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "mme_gemm_stamps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mme_gemm_apply": (C.c_int, [C.c_void_p, C.POINTER(_GemmApplyArgs), C.POINTER(C.c_int32), C.c_void_p]),
    "mme_rowop_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_RowopApplyArgs), C.c_void_p]),
    "mme_select_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_SelectApplyArgs), C.c_void_p]),
    "mme_load_tile_vit": (C.c_int, [C.c_void_p, C.POINTER(_TileWeights)]),
    "mme_load_tile_vit_as": (C.c_int, [C.c_void_p, C.POINTER(_TileWeights), C.c_int, C.c_void_p]),
    "mme_tile_vit_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mme_tile_rowop_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_TileRowopApplyArgs), C.c_void_p]),
    "mme_load_mllama_lm": (C.c_int, [C.c_void_p, C.POINTER(_MllamaLMWeights)]),
    "mme_load_mllama_lm_as": (C.c_int, [C.c_void_p, C.POINTER(_MllamaLMWeights), C.c_int, C.c_void_p]),
    "mme_mllama_lm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "mme_mllama_lm_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "mme_mllama_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "mme_mllama_apply": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_MllamaApplyArgs), C.c_void_p]),
    "mme_comm_unique_id": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mme_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "mme_comm_destroy": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mme_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "mme_attention_stamps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "mme_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "mme_profile_reset": (C.c_int, [C.c_void_p]),
    "mme_profile_read_sync": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}

RESIZE_SPEC_RULE = 2  # MME_RESIZE_SPEC: a rule with parameters, so not one of Engine.RESIZE_RULES' names
RESIZE_MODES = {"shortest_edge": 0, "exact": 1}  # MME_RESIZE_MODE_*
RESIZE_MODES_BY_NUMBER = {v: k for k, v in RESIZE_MODES.items()}


@dataclasses.dataclass(frozen=True)
class ResizeSpec:
    """mme_resize_spec: how a crop becomes 224 x 224 pixels the way a checkpoint's image processor makes them.  The whole crop
    is resized with Pillow's `resample` (2 BILINEAR, 3 BICUBIC) -- mode "exact": to height x width, the aspect not kept; mode
    "shortest_edge": the short edge to `height`, the long edge to int(height * long / short), `width` 0 -- and the 224 x 224
    centre window of the result is taken.  `ResizeSpec.of("shortest_edge", 256, 3)` is DINOv2's, `.of("exact", 224, 3)` SigLIP's,
    `.of("exact", 224, 2)` ViT's."""
    mode: str
    height: int
    width: int
    resample: int

    @classmethod
    def of(cls, mode, size, resample):
        if mode == "exact":
            h, w = (size, size) if isinstance(size, int) else tuple(size)
            return cls("exact", h, w, resample)
        return cls(mode, size, 0, resample)

    @property
    def mode_number(self):
        if self.mode not in RESIZE_MODES and not isinstance(self.mode, int):
            raise MmeError(f"ResizeSpec mode = {self.mode!r}; supported {sorted(RESIZE_MODES)}")
        return RESIZE_MODES.get(self.mode, self.mode)


_lib = None


def load_library(path: str | None = None):
    """dlopen libmme.so and type every export of include/mme.h (no GPU needed for this)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if path is None and os.path.abspath(p) != os.path.abspath(DEFAULT_LIB_PATH) and os.environ.get("MME_ALLOW_LIB_OVERRIDE") != "1":
        raise MmeError(f"MME_LIB_PATH={p} names another library than the in-tree libmme.so; that is a measurement-tool switch "
                       "(tools/_diag.py) and needs MME_ALLOW_LIB_OVERRIDE=1 beside it.  Unset MME_LIB_PATH to run the product library.")
    # torch ships its own libamdhip64; libmme.so must bind to THAT runtime (one HIP runtime per
    # process), so torch is always loaded first.  Loading libmme.so first makes the second
    # runtime report "no ROCm-capable device".
    import torch  # noqa: F401

    if not os.path.exists(p):
        raise MmeError(
            f"{p} is missing: build it with `python -m multimodal_embeddings_amd.build` "
            "(hipcc, gfx950).  There is no CPU fallback for the embed/compare path."
        )
    lib = C.CDLL(p)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.mme_abi_version() != ABI_VERSION:
        raise MmeError(f"libmme ABI version {lib.mme_abi_version()} != {ABI_VERSION} (include/mme.h MME_ABI_VERSION): rebuild the library "
                       "(python -m multimodal_embeddings_amd.build --force) or update the binding")
    if lib.mme_is_diag_build():
        import sys

        print(f"libmme: DIAGNOSTIC build loaded ({p}): it reads the MME_* experiment switches from the environment, some of which "
              "produce wrong results on purpose; never use it for production embeddings", file=sys.stderr, flush=True)
    if path is None:
        _lib = lib
    return lib


def _fp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


LANCZOS_MAX_IN, LANCZOS_MAX_OUT, LANCZOS_MAX_RATIO = 32768, 8000, 16  # what mme_lanczos_resize accepts per axis (include/mme.h)


def lanczos_geometry_ok(h: int, w: int, new_h: int, new_w: int) -> bool:
    """Whether mme_lanczos_resize accepts h x w -> new_h x new_w."""
    return all(1 <= i <= LANCZOS_MAX_IN and 1 <= o <= LANCZOS_MAX_OUT and i <= LANCZOS_MAX_RATIO * o for i, o in ((h, new_h), (w, new_w)))


def check_lanczos_geometry(h: int, w: int, new_h: int, new_w: int):
    """Raises MmeError naming the field, its value and the supported range, as the library does."""
    for (iname, i), (oname, o) in ((("h", h), ("new_h", new_h)), (("w", w), ("new_w", new_w))):
        if not 1 <= i <= LANCZOS_MAX_IN:
            raise MmeError(f"lanczos_resize: {iname} = {i}; supported 1..{LANCZOS_MAX_IN}")
        if not 1 <= o <= LANCZOS_MAX_OUT:
            raise MmeError(f"lanczos_resize: {oname} = {o}; supported 1..{LANCZOS_MAX_OUT}")
        if i > LANCZOS_MAX_RATIO * o:
            raise MmeError(f"lanczos_resize: {iname} / {oname} = {i} / {o}; supported: a ratio of at most {LANCZOS_MAX_RATIO}")


def lanczos_workspace(h: int, w: int, new_h: int, new_w: int) -> int:
    """Bytes of device scratch mme_lanczos_resize needs (mme_lanczos_workspace; no GPU needed)."""
    lib = load_library()
    n = C.c_size_t(0)
    if lib.mme_lanczos_workspace(int(h), int(w), int(new_h), int(new_w), C.byref(n)) != 0:
        raise MmeError(f"mme_lanczos_workspace failed: {lib.mme_last_error(None).decode()}")
    return int(n.value)


def lanczos_tables(in_size: int, out_size: int):
    """(bounds int32[out, 2] {xmin, n}, coeffs int32[out, ksize]) of one axis: Pillow's own fixed-point LANCZOS tables
    (mme_lanczos_tables; a host function, no GPU needed)."""
    lib = load_library()
    ks = C.c_int(0)
    if lib.mme_lanczos_tables(int(in_size), int(out_size), None, None, C.byref(ks)) != 0:
        raise MmeError(f"mme_lanczos_tables failed: {lib.mme_last_error(None).decode()}")
    bounds = np.zeros((int(out_size), 2), dtype=np.int32)
    coeffs = np.zeros((int(out_size), ks.value), dtype=np.int32)
    if lib.mme_lanczos_tables(int(in_size), int(out_size), bounds.ctypes.data, coeffs.ctypes.data, C.byref(ks)) != 0:
        raise MmeError(f"mme_lanczos_tables failed: {lib.mme_last_error(None).decode()}")
    return bounds, coeffs


# ---- the per-encoder pieces of a weight struct; encoders.ENCODER_TABLE names them, Engine._weights_struct runs them -----------------
def _fill_layers(layers, names, arr, scales=None):
    """The tensor pointers of every layer: names(i) maps the fields of layer i (_Layer's; "lambda1" / "lambda2" are
    _Dinov2Scale's, in scales[i]) to its tensor names."""
    for i, L in enumerate(layers):
        for fld, name in names(i).items():
            setattr(scales[i] if fld.startswith("lambda") else L, fld, arr(name))


def _refuse(bad, fields):
    """Raises for a weights.*_geometry_problem in one of `fields`, those the C struct does not carry: the library could not refuse it."""
    if bad and bad[0] in fields:
        raise MmeError(f"{bad[0]} = {bad[1]!r}; supported: {bad[2]}")


def _clip_act(geom) -> int:
    if geom.hidden_act not in CLIP_ACTS:
        raise MmeError(f"hidden_act = {geom.hidden_act!r}; supported: {', '.join(CLIP_ACTS)}")
    return CLIP_ACTS.index(geom.hidden_act)


def _vit_scalars(W, geom):
    V = getattr(W, "vit", W)  # the image towers' structs begin with an mme_vit_weights
    V.image_size, V.patch_size, V.hidden, V.layers, V.heads, V.mlp = (geom.image_size, geom.patch_size, geom.hidden_size, geom.num_layers,
                                                                      geom.num_heads, geom.intermediate_size)
    V.ln_eps = float(geom.layer_norm_eps)


def _clip_scalars(W, geom):
    _vit_scalars(W, geom)
    W.proj_dim, W.act = int(geom.projection_dim or 0), _clip_act(geom)


def _siglip_scalars(W, geom):
    _refuse(siglip_geometry_problem(geom), ("hidden_act", "vision_use_head"))
    _vit_scalars(W, geom)


def _siglip_head(W, geom, arr):
    """The pooling head, as one more _Layer without a first LayerNorm: in_proj_weight [3 D, D] and in_proj_bias [3 D] are
    split q | k | v by element offset."""
    h, D, H = "vision_model.head.", geom.hidden_size, W.head
    H.ln1_g = H.ln1_b = None
    H.q_w, H.k_w, H.v_w = (arr(h + "attention.in_proj_weight", i * D * D) for i in range(3))
    H.q_b, H.k_b, H.v_b = (arr(h + "attention.in_proj_bias", i * D) for i in range(3))
    H.o_w, H.o_b = arr(h + "attention.out_proj.weight"), arr(h + "attention.out_proj.bias")
    H.ln2_g, H.ln2_b = arr(h + "layernorm.weight"), arr(h + "layernorm.bias")
    H.fc1_w, H.fc1_b = arr(h + "mlp.fc1.weight"), arr(h + "mlp.fc1.bias")
    H.fc2_w, H.fc2_b = arr(h + "mlp.fc2.weight"), arr(h + "mlp.fc2.bias")


def _dinov2_scalars(W, geom):
    _refuse(dinov2_geometry_problem(geom), ("hidden_act", "use_swiglu_ffn", "num_register_tokens", "position_grid"))
    _vit_scalars(W, geom)
    W.vit.image_size = 224  # whatever the position table was made for


def _dinov2_host_geometry(w: dict, geom):
    """`geom` (None: all of it) with the position grid the tensors have."""
    try:
        found = infer_dinov2_geometry(w)
    except ValueError as e:
        raise MmeError(f"load_dinov2: {e}") from e
    return found if geom is None else dataclasses.replace(geom, position_grid=found.position_grid)


def _dinov2_special(get, extra):
    """pos: the f32 [257, D] position table -- a checkpoint object's own (`extra`), else the dict's table interpolated to
    16 x 16 here, once, as the model does on every forward.  -> (special arguments of the builder, what must stay alive)."""
    import torch

    from .checkpoint import DINOV2_POSITIONS, interpolate_dinov2_positions

    table = extra["position_table"] if extra is not None else interpolate_dinov2_positions(
        torch.from_numpy(np.ascontiguousarray(get(DINOV2_POSITIONS), dtype=np.float32)))
    return {"pos": C.cast(C.c_void_p(table.data_ptr()), C.POINTER(C.c_float))}, table


def _mllama_lm_special(get, extra):
    """The gates of the cross layers travel as numbers: gate(name) reads the checkpoint's (or the dict's) one-element tensor."""
    def gate(name):
        t = get(name)
        return float(t.float().reshape(-1)[0]) if hasattr(t, "float") else float(np.asarray(t).reshape(-1)[0])

    return {"gate": gate}, None


def _clip_text_scalars(W, geom):
    W.hidden, W.layers, W.heads, W.mlp, W.vocab, W.max_positions = (geom.hidden_size, geom.num_layers, geom.num_heads, geom.intermediate_size,
                                                                   geom.vocab_size, geom.max_position_embeddings)
    W.proj_dim, W.act, W.eos_token_id, W.ln_eps = int(geom.projection_dim or 0), _clip_act(geom), int(geom.eos_token_id), float(geom.layer_norm_eps)


def _siglip_text_scalars(W, geom, logits=None):
    """`logits`: (logit_scale, logit_bias) of a whole SiglipModel, or None."""
    _refuse(siglip_text_geometry_problem(geom), ("hidden_act",))  # the struct has no field for it: the library runs tanh-GELU
    W.hidden, W.layers, W.heads, W.mlp, W.vocab, W.max_positions = (geom.hidden_size, geom.num_layers, geom.num_heads, geom.intermediate_size,
                                                                   geom.vocab_size, geom.max_position_embeddings)
    W.projection_size, W.pad_token_id, W.ln_eps = int(geom.projection_size), int(geom.pad_token_id), float(geom.layer_norm_eps)
    W.has_logits, W.logit_scale, W.logit_bias = int(logits is not None), float(logits[0]) if logits else 0.0, float(logits[1]) if logits else 0.0


def _siglip_logits(get):
    """(logit_scale, logit_bias) as floats from get(name) -> a one-value array / tensor or None; None when both are absent."""
    vals = [get(k) for k in ("logit_scale", "logit_bias")]
    if vals[0] is None and vals[1] is None:
        return None
    if vals[0] is None or vals[1] is None:
        raise MmeError("load_siglip_text: logit_scale and logit_bias come together (a whole SiglipModel) or not at all")
    return tuple(float(np.asarray(v.float() if hasattr(v, "float") and not isinstance(v, np.ndarray) else v, dtype=np.float32).reshape(-1)[0]) for v in vals)


def _siglip_text_special(get, extra):
    return {"logits": _siglip_logits(get)}, None


class KmeansResult:
    """What Engine.kmeans returns, CUDA tensors: labels int32 [N], sim float32 [N], centroids bfloat16 [k, d], counts int32 [k],
    sums float64 [k, d], info int64 [4] (iterations, rows moved by the last one, converged, empty clusters), objective
    float64 [1] (the sum of sim)."""

    __slots__ = ("labels", "sim", "centroids", "counts", "sums", "info", "objective")

    def __init__(self, **kw):
        for f in self.__slots__:
            setattr(self, f, kw[f])


class SilhouetteResult:
    """What Engine.silhouette returns, CUDA tensors: score float64 [1] (NaN with fewer than two clusters with members), cluster
    float64 [k] (each cluster's mean, NaN for an empty one), info int64 [2] (rows counted, clusters with members), sums float64
    [k, d] and counts int32 [k] (as K15's update leaves them), samples float64 [N] or None."""

    __slots__ = ("score", "cluster", "info", "sums", "counts", "samples")

    def __init__(self, **kw):
        for f in self.__slots__:
            setattr(self, f, kw[f])


class Engine:
    """One mme_ctx bound to one GPU.  Methods take torch CUDA tensors / numpy control arrays."""

    def __init__(self, device: int = 0):
        import torch

        self.lib = load_library()
        if not torch.cuda.is_available():
            raise MmeError("no GPU visible to torch; the embed/compare path is HIP only (no CPU fallback)")
        self.torch = torch
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.mme_create(self.device, C.byref(h))
        if rc != 0:
            raise MmeError(f"mme_create({device}) failed ({rc}): {self.lib.mme_last_error(None).decode()}")
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.lib.mme_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise MmeError(f"{what} failed ({rc}): {self.lib.mme_last_error(self.h).decode()}")

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ---- weights ---------------------------------------------------------------------------------
    @staticmethod
    def _weights_struct(kind, geom, arr, pos=None, **special):
        """The weight struct of encoder `kind` (a key of encoders.ENCODER_TABLE) at `geom` (+ its layer array, with DINOv2's
        scale array in a pair, which the caller keeps alive).  Tensor pointers come from arr(name, first_element = 0) over the
        names of the record's tensor_specs; a tensor this geometry does not have (CLIP without a projection) stays null.  `pos`
        (DINOv2): the pointer of the f32 [257, D] position table; `logits` (SigLIP text): see _siglip_text_scalars; `gate` (the
        tile tower, which keeps its own builder): scalar gates from gate(name)."""
        from .encoders import ENCODER_TABLE

        rec = ENCODER_TABLE[kind]
        if rec.block is None:  # the two Mllama towers keep their own builders
            return (Engine._mllama_lm_struct if kind == "mllama_text" else Engine._tile_struct)(geom, arr, **special)
        W = rec.struct()
        rec.scalars(W, geom, **special)
        layers = (_Layer * max(0, int(geom.num_layers)))()
        scales = (_Dinov2Scale * len(layers))() if hasattr(W, "scale") else None
        _fill_layers(layers, rec.layer_names, arr, scales)
        V = getattr(W, "vit", W)  # mme_vit_weights: the struct itself, or the one an image tower's struct begins with
        present = {s[0] for s in rec.tensor_specs(dataclasses.replace(geom, num_layers=0))}  # the names outside the layers that this geometry has
        for fld, name in rec.top.items():
            ptr = pos if fld == "pos_emb" and pos is not None else arr(name) if name in present else None
            setattr(W if hasattr(W, fld) else V, fld, ptr)
        if rec.fill:
            rec.fill(W, geom, arr)
        V.layer = layers
        if scales is None:
            return W, layers
        W.scale = scales
        return W, (layers, scales)

    def _load(self, kind, w: dict, geom=None):
        """A dict of f32 arrays under the names of the record's tensor_specs -> this context (the text range of it for a text
        tower), prepared by the host.  `geom` defaults to what the tensor shapes say; every tensor's element count is checked
        against it here, the geometry itself against the supported set by the library."""
        from .encoders import ENCODER_TABLE

        rec = ENCODER_TABLE[kind]
        if rec.host_geometry:
            geom = rec.host_geometry(w, geom)
        elif geom is None:
            geom = rec.infer_geometry(w)
        for name, shape, _ in rec.tensor_specs(geom) if not rec.library_refuses_depth or 0 < geom.num_layers <= 64 else ():
            if name not in w:
                raise MmeError(f"{rec.loader}: tensor {name!r} is missing")
            if int(np.prod(np.shape(w[name]))) != int(np.prod(shape)):
                raise MmeError(f"{rec.loader}: tensor {name!r} has shape {tuple(np.shape(w[name]))}, expected {tuple(shape)}")
        keep = {}

        def arr(name, first=0):
            if name not in keep:
                keep[name] = np.ascontiguousarray(w[name], dtype=np.float32).reshape(-1)
            return _fp(keep[name][first:])

        special, held = rec.special(w.get, None) if rec.special else ({}, None)
        W, arrays = self._weights_struct(kind, geom, arr, **special)
        self._check(getattr(self.lib, rec.symbol)(self.h, C.byref(W)), rec.symbol)

    @staticmethod
    def _ckpt_ptr(ckpt, name, first=0):
        t = ckpt.tensors[name]
        if not t.is_contiguous() or t.device.type != "cpu":
            raise MmeError(f"checkpoint tensor {name!r} must be a contiguous host tensor")
        return C.cast(C.c_void_p(t.data_ptr() + first * t.element_size()), C.POINTER(C.c_float))  # elements of ckpt.dtype behind the struct's float*

    def _load_checkpoint(self, kind, ckpt):
        """`checkpoint.read_checkpoint(dir, kind)` -> this context at the checkpoint's geometry: the raw f32 / bf16 / f16 bytes go
        to the device and are converted, scaled and LayerNorm-folded there, bit-identically to `_load` on the same values."""
        from .encoders import ENCODER_TABLE

        rec = ENCODER_TABLE[kind]
        if getattr(ENCODER_TABLE.get(ckpt.encoder), "symbol", None) != rec.symbol:  # "vit_b16" and "vit" share one loader
            raise MmeError(f"{rec.loader}_checkpoint: the checkpoint was read for encoder {ckpt.encoder!r}")
        special, held = rec.special(ckpt.tensors.get, ckpt.extra) if rec.special else ({}, None)
        W, arrays = self._weights_struct(kind, ckpt.geometry, lambda name, first=0: self._ckpt_ptr(ckpt, name, first), **special)
        self._check(getattr(self.lib, rec.symbol + "_as")(self.h, C.byref(W), int(ckpt.dtype_id), self._stream()), rec.symbol + "_as")

    def load_vit(self, w: dict, eps: float | None = None, geom=None):
        """Canonical-name dict of f32 arrays (weights.vit_tensor_specs) -> this context, replacing what it held.  The
        geometry is `geom` (a weights.ViTGeometry) or, by default, read off the tensor shapes (heads of 64).  `eps` overrides
        the geometry's layer_norm_eps."""
        if eps is not None:
            geom = dataclasses.replace(infer_vit_geometry(w) if geom is None else geom, layer_norm_eps=float(eps))
        self._load("vit", w, geom)

    def load_vit_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "vit_b16" | "vit")` -> this context.  Replaces what the context held."""
        self._load_checkpoint("vit", ckpt)

    def vit_geometry(self):
        """The weights.ViTGeometry this context runs (mme_vit_geometry): that of its last load, ViT-B/16 before any.
        layer_norm_eps is not reported by the library and keeps the dataclass default."""
        from .weights import ViTGeometry

        g = (C.c_int32 * 6)()
        self._check(self.lib.mme_vit_geometry(self.h, g), "mme_vit_geometry")
        return ViTGeometry(image_size=g[0], patch_size=g[1], hidden_size=g[2], num_layers=g[3], num_heads=g[4], intermediate_size=g[5])

    def encoder_info(self) -> dict:
        """What the last load brought (mme_encoder_info): {"kind": "vit" | "clip" | "siglip" | "dinov2", "embed_dim", "hidden_act", "projection_dim"}."""
        o = (C.c_int32 * 4)()
        self._check(self.lib.mme_encoder_info(self.h, o), "mme_encoder_info")
        acts = CLIP_ACTS + ("gelu_pytorch_tanh",)  # the library's act codes: 0, 1 (mme_clip_weights.act), 2 (SigLIP)
        return {"kind": ("vit", "clip", "siglip", "dinov2")[o[0]], "embed_dim": int(o[1]), "hidden_act": acts[o[2]], "projection_dim": int(o[3]) or None}

    @property
    def embed_dim(self) -> int:
        """Width of the rows `vit_forward` / `embed` return: the hidden size (twice that under pooling "cls+mean"), or a CLIP tower's projection_dim."""
        return self.encoder_info()["embed_dim"]

    # ---- the other image towers: each load replaces what the context held ----------------------------------------------------
    def load_clip(self, w: dict, geom=None):
        """`weights.clip_tensor_specs` dict of f32 arrays (the state dict of transformers' CLIPVisionModelWithProjection, or
        of CLIPVisionModel: no visual_projection).  `geom`: a weights.CLIPGeometry; by default read off the tensor shapes, with
        QuickGELU and eps 1e-5 (clip-vit-base-patch16's)."""
        self._load("clip", w, geom)

    def load_clip_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "clip")`, prepared on the device bit-identically to `load_clip` on the same values."""
        self._load_checkpoint("clip", ckpt)

    def load_siglip(self, w: dict, geom=None):
        """`weights.siglip_tensor_specs` dict of f32 arrays (the vision state dict of transformers' SiglipModel).  `geom`: a
        weights.SiglipGeometry; by default read off the tensor shapes, eps 1e-6."""
        self._load("siglip", w, geom)

    def load_siglip_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "siglip")`, prepared on the device bit-identically to `load_siglip` on the same values."""
        self._load_checkpoint("siglip", ckpt)

    def load_dinov2(self, w: dict, geom=None):
        """`weights.dinov2_tensor_specs` dict of f32 arrays (the state dict of transformers' Dinov2Model).  `geom`: a
        weights.Dinov2Geometry; by default read off the tensor shapes, eps 1e-6.  The position table (257 rows, or 1 + g * g of a
        g x g grid) is interpolated to 16 x 16 here, once, as the model does on every forward."""
        self._load("dinov2", w, geom)

    def load_dinov2_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "dinov2")`, prepared on the device bit-identically to `load_dinov2` on the same values.
        The position table is the checkpoint object's interpolated f32 table under every dtype."""
        self._load_checkpoint("dinov2", ckpt)

    DINOV2_OPS = {"retile": 0, "embed_rows": 1, "attention": 2, "pool_ln_l2": 3, "rowscale": 4, "mul": 5}

    def dinov2_apply(self, op, *, src=None, dst=None, acc=None, bias=None, pos=None, cls=None, x=None, qkv=None, out=None, gamma=None, beta=None,
                     emb_f32=None, emb_bf16=None, w=None, factor=None, prepared=None, rows: int = 0, cols: int = 0, n: int = 0, d: int = 768,
                     heads: int = 12, only_block: int = -1, tok: int = 0, dtype: int = 0, eps: float = 1e-6):
        """ONE launch of a kernel a DINOv2 tower adds (ViT/14 @224: 256 patches, 257 tokens), on the caller's CUDA tensors
        (mme_dinov2_apply; synchronous, works on a bare context).  op: a name of DINOV2_OPS or its code; `n` = crops; which
        tensors each op reads is in include/mme.h.  The library validates."""
        a = _Dinov2ApplyArgs()
        a.src, a.dst, a.acc, a.bias, a.pos, a.cls, a.x = (self._ptr(t) for t in (src, dst, acc, bias, pos, cls, x))
        a.qkv, a.out, a.gamma, a.beta, a.emb_f32, a.emb_bf16 = (self._ptr(t) for t in (qkv, out, gamma, beta, emb_f32, emb_bf16))
        a.w, a.factor, a.prepared = (self._ptr(t) for t in (w, factor, prepared))
        a.rows, a.cols = int(rows), int(cols)
        a.n, a.d, a.heads, a.only_block, a.tok, a.dtype, a.eps = int(n), int(d), int(heads), int(only_block), int(tok), int(dtype), float(eps)
        self._check(self.lib.mme_dinov2_apply(self.h, int(self.DINOV2_OPS.get(op, op)), C.byref(a), self._stream()), "mme_dinov2_apply")

    # ---- CLIP text tower (mme_load_clip_text*): lives beside the image tower of the same context ----------------------------
    def load_clip_text(self, w: dict, geom=None):
        """`weights.clip_text_tensor_specs` dict of f32 arrays (the state dict of transformers' CLIPTextModelWithProjection, or
        of CLIPTextModel: no text_projection) -> the text tower of this context, replacing an earlier text tower and nothing
        else.  `geom`: a weights.CLIPTextGeometry; by default read off the tensor shapes (weights.infer_clip_text_geometry)."""
        self._load("clip_text", w, geom)

    def load_clip_text_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "clip_text")` -> the text tower of this context, prepared on the device
        bit-identically to `load_clip_text` on the same values."""
        self._load_checkpoint("clip_text", ckpt)

    def text_info(self) -> dict:
        """The text tower of this context (mme_text_info); every number 0 and hidden_act None before a text load."""
        o = (C.c_int32 * 9)()
        self._check(self.lib.mme_text_info(self.h, o), "mme_text_info")
        acts = tuple(CLIP_ACTS) + ("gelu_pytorch_tanh",)  # EncoderPass::act; 2 under a SigLIP text tower, whose last word is pad_token_id
        return {"loaded": int(o[0]), "hidden_size": int(o[1]), "num_layers": int(o[2]), "num_heads": int(o[3]), "intermediate_size": int(o[4]),
                "vocab_size": int(o[5]), "projection_dim": int(o[6]) or None, "hidden_act": acts[o[7]] if o[0] else None,
                "eos_token_id": int(o[8])}

    TEXT_KINDS = (None, "clip", "siglip")

    def text_geometry(self) -> dict:
        """What `text_forward` takes and gives under the loaded text tower (mme_text_geometry): kind None | "clip" | "siglip",
        tokens per sequence (77 | 64; 0 before a text load), projection width (None: none), pad id."""
        o = (C.c_int32 * 4)()
        self._check(self.lib.mme_text_geometry(self.h, o), "mme_text_geometry")
        return {"kind": self.TEXT_KINDS[o[0]], "tokens": int(o[1]), "projection": int(o[2]) or None, "pad_token_id": int(o[3])}

    @property
    def text_embed_dim(self) -> int:
        """Width of the rows `text_forward` returns: the text tower's projection_dim, or its hidden size; 0 before a text load."""
        i = self.text_info()
        return int(i["projection_dim"] or i["hidden_size"])

    def text_forward(self, ids, want_f32: bool = True, want_bf16: bool = True):
        """int token ids [n, 77] (host; [n, 64] under a SigLIP text tower) -> (f32 [n, text_embed_dim] | None, bf16 | None) CUDA
        tensors of unit rows (mme_text_forward).  The library checks every id and finds each sequence's EOS position (CLIP) or
        pools position 63 (SigLIP); n = 0 gives empty tensors."""
        t = self.torch
        a = np.asarray(ids)
        T = self.text_geometry()["tokens"] or 77
        if a.ndim != 2 or a.shape[1] != T or a.dtype.kind not in "iu":
            raise MmeError(f"text_forward: ids must be an integer array [n, {T}], got {a.dtype} {tuple(a.shape)}")
        if a.size and (a.min() < -2**31 or a.max() >= 2**31):
            raise MmeError("text_forward: an id does not fit 32 bits")
        a = np.ascontiguousarray(a, dtype=np.int32)
        n, d = a.shape[0], self.text_embed_dim
        dev = t.device("cuda", self.device)
        e32 = t.empty((n, d), dtype=t.float32, device=dev) if want_f32 else None
        e16 = t.empty((n, d), dtype=t.bfloat16, device=dev) if want_bf16 else None
        self._check(self.lib.mme_text_forward(self.h, a.ctypes.data, n, e32.data_ptr() if want_f32 and n else None,
                                              e16.data_ptr() if want_bf16 and n else None, self._stream()), "mme_text_forward")
        return e32, e16

    TEXT_OPS = {"token_rows": 0, "attention_causal": 1, "eos_pool_ln": 2}

    def text_apply(self, op, *, tok=None, pos=None, ids=None, x=None, qkv=None, out=None, gamma=None, beta=None, eos_pos=None, y=None, y_f32=None,
                   n: int = 0, d: int = 512, heads: int = 8, vocab: int = 0, eps: float = 1e-5):
        """ONE launch of a kernel the text tower adds, on the caller's CUDA tensors (mme_text_apply; synchronous).  op: a name of
        TEXT_OPS or its code; `ids` [n, 77] and `eos_pos` [n] are host integer arrays.  The library validates."""
        a = _TextApplyArgs()
        keep = []

        def host(v):
            if v is None:
                return None
            h = np.ascontiguousarray(np.asarray(v), dtype=np.int32)
            keep.append(h)
            return h.ctypes.data

        a.tok, a.pos, a.x, a.qkv, a.out, a.gamma, a.beta, a.y, a.y_f32 = (self._ptr(t) for t in (tok, pos, x, qkv, out, gamma, beta, y, y_f32))
        a.ids_host, a.eos_pos_host = host(ids), host(eos_pos)
        a.n, a.d, a.heads, a.vocab, a.eps = int(n), int(d), int(heads), int(vocab), float(eps)
        self._check(self.lib.mme_text_apply(self.h, int(self.TEXT_OPS.get(op, op)), C.byref(a), self._stream()), "mme_text_apply")

    # ---- SigLIP text tower (mme_load_siglip_text*): takes the text range of the context, beside whatever image tower it holds ----
    def load_siglip_text(self, w: dict, geom=None):
        """`weights.siglip_text_tensor_specs` dict of f32 arrays (the text half of transformers' SiglipModel state dict; with
        `logit_scale` / `logit_bias` beside the tensors, `siglip_scores` works) -> the text tower of this context, replacing an
        earlier text tower of either kind and nothing else.  `geom`: a weights.SiglipTextGeometry; by default read off the shapes."""
        self._load("siglip_text", w, geom)

    def load_siglip_text_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "siglip_text")` -> the text tower of this context, prepared on the device
        bit-identically to `load_siglip_text` on the same values."""
        self._load_checkpoint("siglip_text", ckpt)

    def siglip_scores(self, cos, out=None):
        """f32 CUDA cosine block [m, N] (`cosine`) -> sigmoid(exp(logit_scale) cos + logit_bias), f32 [m, N] (mme_siglip_scores):
        SiglipModel's probabilities.  `out` may be `cos` (in place).  MmeError unless the loaded text tower is SigLIP's with its two scalars."""
        t = self.torch
        if cos.dtype != t.float32 or cos.dim() != 2 or not cos.is_contiguous():
            raise MmeError(f"siglip_scores: cos must be a contiguous f32 [m, N] tensor, got {cos.dtype} {tuple(cos.shape)}")
        if out is None:
            out = t.empty_like(cos)
        if out.dtype != t.float32 or tuple(out.shape) != tuple(cos.shape) or not out.is_contiguous():
            raise MmeError("siglip_scores: out must match cos")
        self._check(self.lib.mme_siglip_scores(self.h, cos.data_ptr() if cos.numel() else None, int(cos.shape[0]), int(cos.shape[1]),
                                               out.data_ptr() if cos.numel() else None, self._stream()), "mme_siglip_scores")
        return out

    SIGLIP_TEXT_OPS = {"token_rows": 0, "attention": 1, "last_pool_ln": 2, "bias_l2": 3, "scores": 4}

    def siglip_text_apply(self, op, *, tok=None, pos=None, ids=None, x=None, qkv=None, out=None, gamma=None, beta=None, y=None, y_f32=None, acc=None,
                          bias=None, emb_f32=None, emb_bf16=None, cos=None, scores=None, count=None, n: int = 0, d: int = 512, heads: int = 8,
                          vocab: int = 0, only_block: int = -1, p: int = 64, eps: float = 1e-6, logit_scale: float = 0.0, logit_bias: float = 0.0):
        """ONE launch of a kernel the SigLIP text tower adds, on the caller's CUDA tensors (mme_siglip_text_apply; synchronous,
        works on a bare context).  op: a name of SIGLIP_TEXT_OPS or its code; `ids` [n, 64] is a host integer array; `count`
        defaults to cos.numel().  The library validates."""
        a = _SiglipTextApplyArgs()
        h = None
        if ids is not None:
            h = np.ascontiguousarray(np.asarray(ids), dtype=np.int32)
            a.ids_host = h.ctypes.data
        (a.tok, a.pos, a.x, a.qkv, a.out, a.gamma, a.beta, a.y, a.y_f32, a.acc, a.bias, a.emb_f32, a.emb_bf16, a.cos, a.scores) = (
            self._ptr(t) for t in (tok, pos, x, qkv, out, gamma, beta, y, y_f32, acc, bias, emb_f32, emb_bf16, cos, scores))
        a.count = int(cos.numel() if count is None and cos is not None else (count or 0))
        a.n, a.d, a.heads, a.vocab, a.only_block, a.p = int(n), int(d), int(heads), int(vocab), int(only_block), int(p)
        a.eps, a.logit_scale, a.logit_bias = float(eps), float(logit_scale), float(logit_bias)
        self._check(self.lib.mme_siglip_text_apply(self.h, int(self.SIGLIP_TEXT_OPS.get(op, op)), C.byref(a), self._stream()), "mme_siglip_text_apply")

    @staticmethod
    def _tile_struct(geom, arr, gate):
        """mme_tile_vit_weights (+ its layer array, which the caller keeps alive) for `geom`: tensor pointers from arr(name),
        the scalar gates from gate(name)."""
        L = geom.num_layers + geom.num_global_layers
        layers = (_TileLayer * L)()
        for i in range(L):
            gated = i >= geom.num_layers
            p = f"global_transformer.layers.{i - geom.num_layers}." if gated else f"transformer.layers.{i}."
            X = layers[i]
            X.ln1_g, X.ln1_b = arr(p + "input_layernorm.weight"), arr(p + "input_layernorm.bias")
            X.q_w, X.k_w, X.v_w, X.o_w = (arr(p + f"self_attn.{n}_proj.weight") for n in "qkvo")
            X.ln2_g, X.ln2_b = arr(p + "post_attention_layernorm.weight"), arr(p + "post_attention_layernorm.bias")
            X.fc1_w, X.fc1_b, X.fc2_w, X.fc2_b = arr(p + "mlp.fc1.weight"), arr(p + "mlp.fc1.bias"), arr(p + "mlp.fc2.weight"), arr(p + "mlp.fc2.bias")
            X.gated = int(gated)
            X.gate_attn = gate(p + "gate_attn") if gated else 0.0
            X.gate_ffn = gate(p + "gate_ffn") if gated else 0.0
        W = _TileWeights()
        W.image_size, W.patch_size, W.hidden, W.heads, W.mlp = geom.image_size, geom.patch_size, geom.hidden_size, geom.num_heads, geom.intermediate_size
        W.max_tiles, W.aspect_ratios, W.layers, W.global_layers = geom.max_num_tiles, geom.max_aspect_ratio_id + 1, geom.num_layers, geom.num_global_layers
        W.n_intermediate = len(geom.intermediate_layers)
        for k, v in enumerate(geom.intermediate_layers):
            W.intermediate[k] = int(v)
        W.intermediate_save_point = {"after": 0, "before": 1}[geom.intermediate_save_point]
        W.norm_eps = float(geom.norm_eps)
        W.pos_gate = gate("gated_positional_embedding.gate")
        W.pre_gate = gate("pre_tile_positional_embedding.gate")
        W.post_gate = gate("post_tile_positional_embedding.gate")
        W.class_embedding, W.patch_w = arr("class_embedding"), arr("patch_embedding.weight")
        W.pos_emb, W.tile_pos_emb = arr("gated_positional_embedding.embedding"), arr("gated_positional_embedding.tile_embedding.weight")
        W.pre_emb, W.post_emb = arr("pre_tile_positional_embedding.embedding.weight"), arr("post_tile_positional_embedding.embedding.weight")
        W.ln_pre_g, W.ln_pre_b = arr("layernorm_pre.weight"), arr("layernorm_pre.bias")
        W.ln_post_g, W.ln_post_b = arr("layernorm_post.weight"), arr("layernorm_post.bias")
        W.layer = layers
        return W, layers

    def load_tile_vit(self, w: dict, geom=None):
        """Hugging Face `MllamaVisionModel` state dict (f32 arrays) -> the tile-ViT encoder of this context."""
        from .weights import TILE_VIT

        geom = geom or TILE_VIT
        keep = []

        def arr(name):
            a = np.ascontiguousarray(w[name], dtype=np.float32)
            keep.append(a)
            return _fp(a)

        W, layers = self._tile_struct(geom, arr, lambda name: float(w[name][0]))
        self._check(self.lib.mme_load_tile_vit(self.h, C.byref(W)), "mme_load_tile_vit")
        self.tile_features = geom.output_dim

    # ---- weights from a checkpoint, in the file's own dtype, prepared on the device (mme_load_*_as) ------------
    def load_tile_vit_checkpoint(self, ckpt, geometry=None):
        """`checkpoint.read_checkpoint(dir, "mllama_tiles")` -> the tile-ViT encoder of this context, prepared on the device.
        `geometry` overrides the checkpoint's (the save point of the intermediate states is not in the file)."""
        if ckpt.encoder != "mllama_tiles":
            raise MmeError(f"load_tile_vit_checkpoint: the checkpoint was read for encoder {ckpt.encoder!r}")
        geom = geometry or ckpt.geometry
        arr = lambda name: self._ckpt_ptr(ckpt, name)  # noqa: E731
        gate = lambda name: float(ckpt.tensors[name].float().reshape(-1)[0])  # noqa: E731
        W, layers = self._tile_struct(geom, arr, gate)
        self._check(self.lib.mme_load_tile_vit_as(self.h, C.byref(W), int(ckpt.dtype_id), self._stream()), "mme_load_tile_vit_as")
        self.tile_features = geom.output_dim

    # ---- Mllama language tower (mme_load_mllama_lm*): lives beside the tile tower of the same context ----------------------
    @staticmethod
    def _mllama_lm_struct(geom, arr, gate=None):
        """mme_mllama_lm_weights (+ its layer array, which the caller keeps alive) for a weights.MllamaLMGeometry: tensor
        pointers from arr(name), the scalar gates from gate(name) -- by default the first f32 behind arr(name) --; names as
        weights.mllama_lm_tensor_specs."""
        from .weights import MLLAMA_ROPE_TYPES

        if gate is None:
            def gate(name):
                p = arr(name)
                return float(p[0]) if p else 0.0

        n_layers = max(0, int(geom.num_layers))
        cross = set(geom.cross_layers)
        layers = (_MllamaLMLayer * n_layers)()
        for i in range(n_layers):
            p = f"language_model.layers.{i}."
            a = p + ("cross_attn." if i in cross else "self_attn.")
            X = layers[i]
            X.cross = int(i in cross)
            X.ln1, X.ln2 = arr(p + "input_layernorm.weight"), arr(p + "post_attention_layernorm.weight")
            X.q_w, X.k_w, X.v_w, X.o_w = (arr(a + f"{n}_proj.weight") for n in "qkvo")
            if i in cross:
                X.q_norm, X.k_norm = arr(a + "q_norm.weight"), arr(a + "k_norm.weight")
                X.attn_gate, X.mlp_gate = gate(p + "cross_attn_attn_gate"), gate(p + "cross_attn_mlp_gate")
            X.gate_w, X.up_w, X.down_w = (arr(p + f"mlp.{n}_proj.weight") for n in ("gate", "up", "down"))
        W = _MllamaLMWeights()
        W.hidden, W.heads, W.kv_heads, W.intermediate, W.layers = geom.hidden_size, geom.num_heads, geom.num_kv_heads, geom.intermediate_size, geom.num_layers
        W.vocab, W.vision_dim, W.image_token_id = geom.vocab_size, geom.vision_output_dim, geom.image_token_id
        W.hidden_act = 0 if geom.hidden_act == "silu" else -1
        W.rope_type = MLLAMA_ROPE_TYPES.index(geom.rope_type) if geom.rope_type in MLLAMA_ROPE_TYPES else -1
        W.rope_original_max = int(geom.rope_original_max)
        W.rms_eps, W.rope_theta, W.rope_factor = float(geom.rms_norm_eps), float(geom.rope_theta), float(geom.rope_factor)
        W.rope_low_freq_factor, W.rope_high_freq_factor = float(geom.rope_low_freq_factor), float(geom.rope_high_freq_factor)
        W.embed_tokens, W.norm = arr("language_model.embed_tokens.weight"), arr("language_model.norm.weight")
        W.proj_w, W.proj_b = arr("multi_modal_projector.weight"), arr("multi_modal_projector.bias")
        W.layer = layers
        return W, layers

    def load_mllama_lm(self, w: dict, geom=None):
        """`weights.mllama_lm_tensor_specs` dict of f32 arrays (the language model and projector of transformers'
        MllamaForConditionalGeneration, names without `model.`) -> the language tower of this context; the context's other
        towers stay.  `geom`: a weights.MllamaLMGeometry; by default read off the tensor shapes."""
        from .weights import infer_mllama_lm_geometry, mllama_lm_tensor_specs

        geom = geom or infer_mllama_lm_geometry(w)
        if 0 < geom.num_layers <= 64:
            for name, shape, _, _ in mllama_lm_tensor_specs(geom):
                if name not in w:
                    raise MmeError(f"load_mllama_lm: tensor {name!r} is missing")
                if int(np.prod(np.shape(w[name]))) != int(np.prod(shape)):
                    raise MmeError(f"load_mllama_lm: tensor {name!r} has shape {tuple(np.shape(w[name]))}, expected {tuple(shape)}")
        keep = []

        def arr(name):
            a = np.ascontiguousarray(w[name], dtype=np.float32).reshape(-1)
            keep.append(a)
            return _fp(a)

        W, layers = self._mllama_lm_struct(geom, arr, lambda name: float(np.asarray(w[name]).reshape(-1)[0]))
        self._check(self.lib.mme_load_mllama_lm(self.h, C.byref(W)), "mme_load_mllama_lm")

    def load_mllama_lm_tensors(self, tensors: dict, geom, dtype_id: int):
        """Contiguous host torch tensors of ONE dtype (MME_DT_* code `dtype_id`) under the canonical names -> the language tower,
        prepared on the device bit-identically to `load_mllama_lm` on the same values (mme_load_mllama_lm_as)."""
        def arr(name):
            t = tensors[name]
            if not t.is_contiguous() or t.device.type != "cpu":
                raise MmeError(f"checkpoint tensor {name!r} must be a contiguous host tensor")
            return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float))

        W, layers = self._mllama_lm_struct(geom, arr, lambda name: float(tensors[name].float().reshape(-1)[0]))
        self._check(self.lib.mme_load_mllama_lm_as(self.h, C.byref(W), int(dtype_id), self._stream()), "mme_load_mllama_lm_as")

    def load_mllama_lm_checkpoint(self, ckpt):
        """`checkpoint.read_checkpoint(dir, "mllama_text")` -> the language tower of this context, prepared on the device
        bit-identically to `load_mllama_lm` on the same values."""
        self._load_checkpoint("mllama_text", ckpt)

    def mllama_lm_info(self) -> dict:
        """The loaded language tower's geometry as the library holds it (mme_mllama_lm_info); `loaded` False before a load."""
        out = (C.c_int32 * 12)()
        self._check(self.lib.mme_mllama_lm_info(self.h, out), "mme_mllama_lm_info")
        keys = ("loaded", "hidden_size", "num_heads", "num_kv_heads", "intermediate_size", "num_layers", "num_cross_layers", "vocab_size",
                "vision_output_dim", "image_token_id", "rope_type", "first_buffer")
        d = dict(zip(keys, (int(v) for v in out)))
        d["loaded"] = bool(d["loaded"])
        return d

    @staticmethod
    def _mllama_sequences(ids, lengths, xmask):
        ids = np.ascontiguousarray(np.asarray(ids), dtype=np.int32)
        if ids.ndim != 2:
            raise MmeError("the ids must be int32 [n, S]")
        n, S = ids.shape
        lens = np.full(n, S, dtype=np.int32) if lengths is None else np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int32)
        if lens.shape[0] != n:
            raise MmeError(f"{lens.shape[0]} lengths for {n} sequences")
        xm = None
        if xmask is not None:
            xm = np.ascontiguousarray(np.asarray(xmask), dtype=np.uint8)
            if xm.shape != (n, S):
                raise MmeError(f"xmask must be uint8 [n, S] = {(n, S)}, got {xm.shape}")
        return ids, lens, xm, n, S

    def mllama_lm_forward(self, ids, lengths=None, vision=None, num_tiles=None, xmask=None, want_f32: bool = True, want_bf16: bool = True):
        """ids int32 [n, S] (+ attended lengths [n], right padding; default S) -> (emb f32 [n, hidden] | None, emb bf16 | None).
        vision: bf16 CUDA [n, tiles, tokens, vision_dim], the vision model's last_hidden_state, or None for the text-only path;
        num_tiles [n] and / or xmask uint8 [n, S] (attended tiles as bits) as mme_mllama_lm_forward reads them."""
        t = self.torch
        ids, lens, xm, n, S = self._mllama_sequences(ids, lengths, xmask)
        D = self.mllama_lm_info()["hidden_size"]
        dev = t.device("cuda", self.device)
        tiles = tokens = 0
        nt = None
        if vision is not None:
            if vision.dtype != t.bfloat16 or vision.dim() != 4 or vision.shape[0] != n or not vision.is_cuda:
                raise MmeError("mllama_lm_forward: vision must be a bf16 CUDA tensor [n, tiles, tokens, vision_dim]")
            vision = vision.contiguous()
            tiles, tokens = int(vision.shape[1]), int(vision.shape[2])
            if num_tiles is not None:
                nt = np.ascontiguousarray(np.asarray(num_tiles).reshape(-1), dtype=np.int32)
        e32 = t.empty((n, D), dtype=t.float32, device=dev) if want_f32 else None
        e16 = t.empty((n, D), dtype=t.bfloat16, device=dev) if want_bf16 else None
        self._check(self.lib.mme_mllama_lm_forward(self.h, ids.ctypes.data, lens.ctypes.data, n, S, self._ptr(vision), tiles, tokens,
                                                   nt.ctypes.data if nt is not None else None, xm.ctypes.data if xm is not None else None,
                                                   self._ptr(e32), self._ptr(e16), self._stream()), "mme_mllama_lm_forward")
        return e32, e16

    def mllama_embed(self, pixel_values, aspect_ratio_ids, num_tiles, ids, lengths=None, xmask=None, want_f32: bool = True, want_bf16: bool = True):
        """pixel_values f32 CUDA [n, 4, 3, 560, 560] (+ ids / tile counts, as `preprocess_tiles` returns them) and the prompt ids
        int32 [n, S] -> the tile tower, the projector and the language tower -> (emb f32 [n, hidden] | None, emb bf16 | None)."""
        t = self.torch
        pv = pixel_values.contiguous()
        if pv.dtype != t.float32 or tuple(pv.shape[1:]) != (4, 3, 560, 560):
            raise MmeError("mllama_embed: pixel_values must be f32 [n, 4, 3, 560, 560]")
        ids, lens, xm, n, S = self._mllama_sequences(ids, lengths, xmask)
        if pv.shape[0] != n:
            raise MmeError(f"mllama_embed: {pv.shape[0]} images for {n} sequences")
        aid = np.ascontiguousarray(np.asarray(aspect_ratio_ids).reshape(-1), dtype=np.int32)
        nt = np.ascontiguousarray(np.asarray(num_tiles).reshape(-1), dtype=np.int32)
        D = self.mllama_lm_info()["hidden_size"]
        e32 = t.empty((n, D), dtype=t.float32, device=pv.device) if want_f32 else None
        e16 = t.empty((n, D), dtype=t.bfloat16, device=pv.device) if want_bf16 else None
        self._check(self.lib.mme_mllama_embed(self.h, pv.data_ptr(), aid.ctypes.data, nt.ctypes.data, n, ids.ctypes.data, lens.ctypes.data, S,
                                              xm.ctypes.data if xm is not None else None, self._ptr(e32), self._ptr(e16), self._stream()), "mme_mllama_embed")
        return e32, e16

    MLLAMA_OPS = {"gather": 0, "rmsnorm": 1, "headnorm": 2, "rope": 3, "silu_mul": 4, "pool": 5, "self_attn": 6, "cross_attn": 7}

    def mllama_apply(self, op, *, tok=None, ids=None, lengths=None, xmask=None, x=None, y=None, kv=None, w=None, cos=None, sin=None, rowzero=None,
                     emb_f32=None, emb_bf16=None, rows: int = 0, ld: int = 0, n: int = 0, S: int = 0, d: int = 0, heads: int = 0, kv_heads: int = 0,
                     col0: int = 0, vocab: int = 0, tiles: int = 0, tokens: int = 0, eps: float = 1e-5):
        """ONE launch of a kernel of the language tower on the caller's CUDA tensors (mme_mllama_apply; synchronous).  op: a name
        of MLLAMA_OPS or its code; ids / lengths (int32) and xmask (uint8) are host arrays.  The library validates."""
        a = _MllamaApplyArgs()
        keep = []
        for fld, v, dt in (("ids_host", ids, np.int32), ("len_host", lengths, np.int32), ("xmask_host", xmask, np.uint8)):
            if v is not None:
                h = np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=dt)
                keep.append(h)
                setattr(a, fld, h.ctypes.data)
        a.tok, a.x, a.y, a.kv, a.w, a.cos, a.sin, a.rowzero, a.emb_f32, a.emb_bf16 = (
            self._ptr(t) for t in (tok, x, y, kv, w, cos, sin, rowzero, emb_f32, emb_bf16))
        a.rows, a.ld = int(rows), int(ld)
        a.n, a.S, a.d, a.heads, a.kv_heads, a.col0, a.vocab, a.tiles, a.tokens = (int(v) for v in (n, S, d, heads, kv_heads, col0, vocab, tiles, tokens))
        a.eps = float(eps)
        self._check(self.lib.mme_mllama_apply(self.h, int(self.MLLAMA_OPS.get(op, op)), C.byref(a), self._stream()), "mme_mllama_apply")

    def weights_fingerprint(self) -> tuple:
        """One 64-bit checksum per prepared weight buffer of this context, in creation order (mme_weights_fingerprint):
        equal tuples = the same prepared weights, without running a forward."""
        n = self.lib.mme_weights_fingerprint(self.h, 0, None)
        self._check(min(n, 0), "mme_weights_fingerprint")
        out = (C.c_uint64 * max(n, 1))()
        rc = self.lib.mme_weights_fingerprint(self.h, n, out)
        self._check(min(rc, 0), "mme_weights_fingerprint")
        return tuple(int(out[i]) for i in range(n))

    def weights_read(self, index: int) -> np.ndarray:
        """The bytes of prepared weight buffer `index` (creation order, named in include/mme.h) as a uint8 array
        (mme_weights_read; synchronises the device)."""
        n = int(self.lib.mme_weights_read(self.h, int(index), 0, None))
        self._check(min(n, 0), "mme_weights_read")
        out = np.empty(n, dtype=np.uint8)
        rc = int(self.lib.mme_weights_read(self.h, int(index), n, out.ctypes.data))
        self._check(min(rc, 0), "mme_weights_read")
        return out

    WEIGHT_PREP_OPS = {"convert": 0, "pad": 1, "fold": 2}

    def weight_prep_apply(self, op, *, dtype: int = 0, src=None, dst=None, count: int = 0, scale: float = 1.0, scaled: bool = False,
                          out_bf16: bool = False, rows: int = 0, cols: int = 0, cols_padded: int = 0, w=(), b=(), src_rows=(), src_scale=(),
                          src_scaled=(), nsrc=None, gamma=None, beta=None, wf=None, cs=None, bf=None):
        """ONE launch of a weight-preparation kernel on the caller's CUDA tensors (mme_weight_prep_apply; synchronous).  op: a
        name of WEIGHT_PREP_OPS or its code; dtype an MME_DT_* code (0 f32, 1 bf16, 2 f16) of every source; w / b / src_rows /
        src_scale / src_scaled are per-source sequences of the fold (b[i] may be None).  The library validates."""
        a = _WeightPrepApplyArgs()
        a.dtype, a.scaled, a.out_bf16, a.scale = int(dtype), int(bool(scaled)), int(bool(out_bf16)), float(scale)
        a.src, a.dst, a.count = self._ptr(src), self._ptr(dst), int(count)
        a.rows, a.cols, a.cols_padded = int(rows), int(cols), int(cols_padded)
        a.nsrc = int(len(w) if nsrc is None else nsrc)
        for i in range(min(len(w), 3)):
            a.w[i] = self._ptr(w[i])
            a.b[i] = self._ptr(b[i]) if i < len(b) else None
            a.src_rows[i] = int(src_rows[i]) if i < len(src_rows) else 0
            a.src_scale[i] = float(src_scale[i]) if i < len(src_scale) else 1.0
            a.src_scaled[i] = int(bool(src_scaled[i])) if i < len(src_scaled) else 0
        a.gamma, a.beta, a.wf, a.cs, a.bf = (self._ptr(t) for t in (gamma, beta, wf, cs, bf))
        self._check(self.lib.mme_weight_prep_apply(self.h, int(self.WEIGHT_PREP_OPS.get(op, op)), C.byref(a), self._stream()), "mme_weight_prep_apply")

    def tile_vit_forward(self, pixel_values, aspect_ratio_ids, num_tiles, want_hidden=False, want_f32=True, want_bf16=True):
        """pixel_values f32 CUDA [n, 4, 3, 560, 560] (+ ids / tile counts, as `preprocess_tiles` returns them) ->
        (hidden f32 [n, 4, 1601, F] | None, emb f32 [n, F] | None, emb bf16 [n, F] | None)."""
        t = self.torch
        pv = pixel_values.contiguous()
        n, F = pv.shape[0], self.tile_features
        if pv.dtype != t.float32 or tuple(pv.shape[1:]) != (4, 3, 560, 560):
            raise MmeError("tile_vit_forward: pixel_values must be f32 [n, 4, 3, 560, 560]")
        ids = np.ascontiguousarray(np.asarray(aspect_ratio_ids).reshape(-1), dtype=np.int32)
        nt = np.ascontiguousarray(np.asarray(num_tiles).reshape(-1), dtype=np.int32)
        hidden = t.empty((n, 4, 1601, F), dtype=t.float32, device=pv.device) if want_hidden else None
        e32 = t.empty((n, F), dtype=t.float32, device=pv.device) if want_f32 else None
        e16 = t.empty((n, F), dtype=t.bfloat16, device=pv.device) if want_bf16 else None
        self._check(self.lib.mme_tile_vit_forward(self.h, pv.data_ptr(), ids.ctypes.data, nt.ctypes.data, n,
                                                  hidden.data_ptr() if want_hidden else None, e32.data_ptr() if want_f32 else None,
                                                  e16.data_ptr() if want_bf16 else None, self._stream()), "mme_tile_vit_forward")
        return hidden, e32, e16

    def set_normalisation(self, mean, std):
        m = (C.c_float * 3)(*mean)
        s = (C.c_float * 3)(*std)
        self._check(self.lib.mme_set_normalisation(self.h, m, s), "mme_set_normalisation")

    def normalisation_form(self):
        """(exact, a float32[3], b float32[3]) of the current constants (mme_normalisation_form): exact = True when the patch
        emitter of a resized batch computes bf16(fma(u, a[ch], b[ch])), False when it reads the table (a, b then mean nothing)."""
        exact = C.c_int32(-1)
        a, b = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
        self._check(self.lib.mme_normalisation_form(self.h, C.byref(exact), _fp(a), _fp(b)), "mme_normalisation_form")
        return bool(exact.value), a, b

    RESIZE_RULES = {"fit_pad": 0, "clip": 1}  # MME_RESIZE_* (include/mme.h)

    def set_resize_rule(self, rule):
        """How `preprocess` / `embed` make 224 x 224 pixels (mme_set_resize_rule): "fit_pad" (the default: fit, BILINEAR, zero
        pad) or "clip" (CLIPImageProcessor's shortest-edge BICUBIC resize + centre crop).  An int goes to the library as it is."""
        if isinstance(rule, str):
            if rule not in self.RESIZE_RULES:
                raise MmeError(f"resize rule {rule!r}: supported {sorted(self.RESIZE_RULES)}")
            rule = self.RESIZE_RULES[rule]
        self._check(self.lib.mme_set_resize_rule(self.h, int(rule)), "mme_set_resize_rule")

    @property
    def resize_rule(self) -> str:
        """"fit_pad", "clip", or "spec" while a `ResizeSpec` is the rule (`resize_spec`)."""
        v = C.c_int32(-1)
        self._check(self.lib.mme_resize_rule(self.h, C.byref(v)), "mme_resize_rule")
        return {RESIZE_SPEC_RULE: "spec", **{n: k for k, n in self.RESIZE_RULES.items()}}[v.value]

    def set_resize_spec(self, mode, size=None, resample=None):
        """Make a spec the rule of `preprocess` / `embed` (mme_set_resize_spec): resize the whole crop with Pillow's filter
        `resample` (2 BILINEAR, 3 BICUBIC) to `size`, then take the 224 x 224 centre window.  `mode` "shortest_edge" with
        `size` the edge, or "exact" with `size` = (height, width) or one int for both.  A `ResizeSpec` may be passed alone.
        The library refuses what it does not run (edges outside 224..512, other filters) and the rule then stays as it was."""
        spec = mode if isinstance(mode, ResizeSpec) else ResizeSpec.of(mode, size, resample)
        try:
            raw = _ResizeSpec(int(spec.mode_number), int(spec.height), int(spec.width), int(spec.resample))
        except (TypeError, ValueError) as e:
            raise MmeError(f"{spec!r}: mode, size and resample must be integers ({e})") from None
        self._check(self.lib.mme_set_resize_spec(self.h, C.byref(raw)), "mme_set_resize_spec")

    @property
    def resize_spec(self):
        """The `ResizeSpec` that is the current rule, or None under "fit_pad" and "clip"."""
        v = C.c_int32(-1)
        self._check(self.lib.mme_resize_rule(self.h, C.byref(v)), "mme_resize_rule")
        if v.value != RESIZE_SPEC_RULE:
            return None
        raw = _ResizeSpec()
        self._check(self.lib.mme_get_resize_spec(self.h, C.byref(raw)), "mme_get_resize_spec")
        return ResizeSpec(RESIZE_MODES_BY_NUMBER.get(raw.mode, raw.mode), raw.height, raw.width, raw.resample)

    def set_gemm_variant(self, variant: int):
        self._check(self.lib.mme_set_gemm_variant(self.h, int(variant)), "mme_set_gemm_variant")

    def set_ln_fusion(self, mode):
        """0 / False: LayerNorm kernel; 1: folded + statistics pass over x; 2 / True: folded + partial sums from the producing GEMM."""
        m = 2 if mode is True else int(mode)
        self._check(self.lib.mme_set_ln_fusion(self.h, m), "mme_set_ln_fusion")

    def set_attention_mode(self, mode):
        """1 / "fast" (default): guarded fast softmax; 0 / "exact": row maximum first (see mme.h)."""
        m = {"exact": 0, "fast": 1, "fast_forced_redo": 2}.get(mode, mode)
        self._check(self.lib.mme_set_attention_mode(self.h, int(m)), "mme_set_attention_mode")

    def set_tile_order(self, mode: int):
        """0 upwards, 1 zig-zag between consecutive kernels (default), 2 attention downwards only; bit-identical results."""
        self._check(self.lib.mme_set_tile_order(self.h, int(mode)), "mme_set_tile_order")

    def set_forward_pruning(self, on: bool):
        """Skip what nothing reads in the LAST layer (only the pooled token's row is computed after its attention):
        bit-identical embeddings, 6 % less work; off by default (see mme.h)."""
        self._check(self.lib.mme_set_forward_pruning(self.h, int(bool(on))), "mme_set_forward_pruning")

    POOLINGS = {"token": 0, "mean": 1, "cls+mean": 2}  # MME_POOL_*

    def set_pooling(self, mode):
        """"token" / 0 (default: the row `pool_token` names), "mean" / 1 (the mean of the final-LayerNorm patch rows the crop
        covers, L2-normalised) or "cls+mean" / 2 ([class row | mean], one L2 norm, embed_dim = 2 * hidden); the mean modes need
        a vit or dinov2 tower loaded, and every load goes back to "token" (mme_set_pooling, include/mme.h)."""
        self._check(self.lib.mme_set_pooling(self.h, int(self.POOLINGS.get(mode, mode))), "mme_set_pooling")

    @property
    def pooling(self) -> str:
        m = C.c_int32(-1)
        self._check(self.lib.mme_pooling(self.h, C.byref(m)), "mme_pooling")
        return {v: k for k, v in self.POOLINGS.items()}[m.value]

    @staticmethod
    def pool_grid(h: int, w: int, patch: int = 16):
        """(R, C): the patches an h x w crop covers under the fit-and-pad rule (mme_pool_grid; a host function, no GPU needed)."""
        lib = load_library()
        rc = (C.c_int32 * 2)()
        if lib.mme_pool_grid(int(h), int(w), int(patch), rc) != 0:
            raise MmeError(f"mme_pool_grid failed: {lib.mme_last_error(None).decode()}")
        return int(rc[0]), int(rc[1])

    @staticmethod
    def k1_plan(rule, hw, *, tile: int = 560, max_tiles: int = 4, bands: bool = False):
        """(records, totals): what K1 plans on the host for crops of sizes hw [n, 2] (h, w) under `rule` -- "fit_pad", "clip", a
        `ResizeSpec`, or "tiles" with (tile, max_tiles) (mme_k1_plan; a host function, no GPU needed).  records: a numpy record
        array of K1_RECORD, one per crop; totals: int64 [4] = table bytes, scratch bytes, bands, largest kv.  bands=True: a third
        value, int32 [bands, 4] = (crop, first source row, rows, class) of every band of the horizontal pass in launch order."""
        lib = load_library()
        raw = _K1Rule()
        if rule == "fit_pad":
            raw.kind = 0
        elif rule == "tiles":
            raw.kind, raw.tile, raw.max_tiles = 2, int(tile), int(max_tiles)
        else:
            spec = ResizeSpec("shortest_edge", 224, 0, 3) if rule == "clip" else rule
            if not isinstance(spec, ResizeSpec):
                raise MmeError(f"k1_plan rule = {rule!r}; supported 'fit_pad', 'clip', 'tiles' and a ResizeSpec")
            raw.kind, raw.spec = 1, _ResizeSpec(int(spec.mode_number), int(spec.height), int(spec.width), int(spec.resample))
        hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
        out = np.zeros(len(hw), dtype=K1_RECORD)
        totals = np.zeros(4, dtype=np.int64)
        if lib.mme_k1_plan(C.byref(raw), hw.ctypes.data, len(hw), out.ctypes.data, totals.ctypes.data, None, 0) != 0:
            raise MmeError(f"mme_k1_plan failed: {lib.mme_last_error(None).decode()}")
        if not bands:
            return out, totals
        listed = np.zeros((int(totals[2]), 4), dtype=np.int32)
        if lib.mme_k1_plan(C.byref(raw), hw.ctypes.data, len(hw), out.ctypes.data, totals.ctypes.data, listed.ctypes.data, len(listed)) != 0:
            raise MmeError(f"mme_k1_plan failed: {lib.mme_last_error(None).decode()}")
        return out, totals, listed

    def pool_grids(self, hw) -> np.ndarray:
        """int32 [n, 2]: the covered grids the pixel path of this context uses for crops of sizes hw [n, 2] (mme_pool_grids)."""
        hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
        out = np.zeros_like(hw)
        self._check(self.lib.mme_pool_grids(self.h, hw.ctypes.data, len(hw), out.ctypes.data), "mme_pool_grids")
        return out

    POOL_OPS = {"mean": 0, "cls+mean": 1}

    def pool_apply(self, op, *, x=None, gamma=None, beta=None, grids=None, emb_f32=None, emb_bf16=None, B: int = 0, tokens: int = 197, g: int = 14,
                   first: int = 1, d: int = 768, eps: float = 1e-12):
        """ONE launch of the mean-pooling kernel on the caller's CUDA tensors (mme_pool_apply; synchronous).  `grids`: an int32
        CUDA tensor [B, 2] (R, C) or None for whole grids; the library cannot read device memory, so the entries are checked
        here (1..g each, else MmeError and nothing is launched).  Everything else the library validates."""
        if grids is not None and grids.numel() and (int(grids.min()) < 1 or int(grids.max()) > int(g)):
            bad = self.torch.nonzero((grids < 1) | (grids > int(g)))[0].tolist()
            raise MmeError(f"pool_apply: grids[{bad[0]}][{bad[1]}] = {int(grids[bad[0], bad[1]])}; supported 1..{int(g)}")
        a = _PoolApplyArgs()
        a.x, a.gamma, a.beta, a.grids, a.emb_f32, a.emb_bf16 = (self._ptr(t) for t in (x, gamma, beta, grids, emb_f32, emb_bf16))
        a.B, a.tokens, a.g, a.first, a.d, a.eps = int(B), int(tokens), int(g), int(first), int(d), float(eps)
        self._check(self.lib.mme_pool_apply(self.h, int(self.POOL_OPS.get(op, op)), C.byref(a), self._stream()), "mme_pool_apply")

    def attention_redone(self, count: int = 12):
        """Layers of the LAST encoder pass whose attention launch raised the fast form's guard (list of `count` ints:
        `vit_geometry().num_layers` for the ViT forward -- 12 for ViT-B/16 --, the tower's layer count after `tile_vit_forward`)."""
        flags = (C.c_int32 * int(count))()
        self._check(self.lib.mme_attention_redone_n(self.h, int(count), flags), "mme_attention_redone_n")
        return list(flags)

    # (tokens, heads, head dim) of the attention kinds mme_attention_apply takes; kind 0 runs at the context's geometry
    _ATTN_KINDS = {0: (197, None, 64), 1: (6432, 16, 80)}

    def attention(self, qkv, kind: int, ntiles=None, only_block: int = -1, reverse: bool = False, out=None):
        """ONE attention launch under the current attention mode (mme_attention_apply; synchronous).  qkv bf16 CUDA
        [n * T, 3 * H * dh] = Q | K | V with Q pre-scaled by dh^-0.5 log2(e); kind 0 = the ViT of this context (T 197, H x 64
        with H = 6, 12 or 16 as loaded; 12 before any load), kind 1 =
        tile-ViT (T 6432, 16 x 80, `ntiles` = tiles per image, 1..4).  -> (out bf16 [n * T, H * dh], redone: bool)."""
        t = self.torch
        if kind not in self._ATTN_KINDS:
            raise MmeError(f"attention: kind {kind} (0 = ViT/16, 1 = tile-ViT)")
        T, H, dh = self._ATTN_KINDS[kind]
        if H is None:
            H = self.vit_geometry().num_heads
            if self.encoder_info()["kind"] == "siglip":  # no class token: the kernel's 196-token instantiation
                T = 196
        if qkv.dtype != t.bfloat16 or not qkv.is_contiguous() or qkv.dim() != 2 or qkv.shape[1] != 3 * H * dh or qkv.shape[0] % T:
            raise MmeError(f"attention: qkv must be a contiguous bf16 [n * {T}, {3 * H * dh}] tensor")
        n = qkv.shape[0] // T
        if out is None:
            out = t.empty((n * T, H * dh), dtype=t.bfloat16, device=qkv.device)
        if out.dtype != t.bfloat16 or not out.is_contiguous() or tuple(out.shape) != (n * T, H * dh):
            raise MmeError(f"attention: out must be a contiguous bf16 [{n * T}, {H * dh}] tensor")
        nt = None
        if ntiles is not None:
            nt = np.ascontiguousarray(np.asarray(ntiles).reshape(-1), dtype=np.int32)
            if nt.shape[0] != n:
                raise MmeError(f"attention: {nt.shape[0]} tile counts for {n} images")
        redone = C.c_int32(0)
        self._check(self.lib.mme_attention_apply(self.h, int(kind), qkv.data_ptr(), n, None if nt is None else nt.ctypes.data, int(only_block),
                                                 int(bool(reverse)), out.data_ptr(), C.byref(redone), self._stream()), "mme_attention_apply")
        return out, bool(redone.value)

    @staticmethod
    def _ptr(t):
        return None if t is None else int(t.data_ptr())

    def _gemm_args(self, A, W, M, N, K, variant, reverse_m, bias, out, ldo, ln_stats, colsum):
        """The operands every GEMM hook takes (gemm_apply, and the GEMM ops of clip_apply / siglip_apply) as mme_gemm_apply_args:
        M, N, K default to the operands' shapes, ldo to N."""
        g = _GemmApplyArgs()
        g.variant, g.reverse_m = int(variant), int(reverse_m)
        g.M = int(A.shape[0] if M is None else M)
        g.N = int(W.shape[0] if N is None else N)
        g.K = int(A.shape[1] if K is None else K)
        g.A, g.W, g.bias, g.out, g.ln_stats, g.colsum = (self._ptr(t) for t in (A, W, bias, out, ln_stats, colsum))
        g.ldo = int(g.N if ldo is None else ldo)
        return g

    def gemm_apply(self, epilogue: int, A, W, *, M=None, N=None, K=None, variant: int = 0, reverse_m: int = 0, bias=None, out=None, ldo=None,
                   res=None, pos=None, outf=None, ldf=None, ln_stats=None, colsum=None, ln_part=None, ln_part_rows: int = 0) -> bool:
        """ONE GEMM launch with one epilogue on the caller's CUDA tensors (mme_gemm_apply; synchronous): A bf16 [M, K],
        W bf16 [N, K]; the other tensors as include/mme.h describes them, `out` / `res` / `outf` possibly views into larger
        buffers with row pitch `ldo` / `ldf` (default N).  M, N, K default to the operands' shapes.  -> True when the
        256 x 256 kernel ran.  Nothing is checked here: the library validates every argument and raises MmeError."""
        a = self._gemm_args(A, W, M, N, K, variant, reverse_m, bias, out, ldo, ln_stats, colsum)
        a.epilogue = int(epilogue)
        a.res, a.pos, a.outf, a.ln_part = (self._ptr(t) for t in (res, pos, outf, ln_part))
        a.ldf = int(a.N if ldf is None else ldf)
        a.pos_rows = 0 if pos is None else int(pos.shape[0])
        a.ln_part_rows = int(ln_part_rows)
        a.ln_part_floats = 0 if ln_part is None else int(ln_part.numel())
        ran = C.c_int32(-1)
        self._check(self.lib.mme_gemm_apply(self.h, C.byref(a), C.byref(ran), self._stream()), "mme_gemm_apply")
        return bool(ran.value)

    ROWOPS = {"layernorm": 0, "ln_stats": 1, "ln_stats_canonical": 2, "ln_finish": 3, "cls_rows": 4, "pool_ln_l2": 5}

    def rowop_apply(self, op, *, x=None, y=None, gamma=None, beta=None, stats=None, part=None, cls=None, pos=None, emb_f32=None, emb_bf16=None,
                    rows: int = 0, row0: int = 0, row1: int = 0, stride: int = 1, part_rows: int = 0, d: int = 768, B: int = 0, tok: int = 0,
                    eps: float = 1e-12):
        """ONE launch of a row kernel of the forward on the caller's CUDA tensors (mme_rowop_apply; synchronous).  op: a name
        of ROWOPS or its code; which tensors and sizes each op reads is in include/mme.h.  The library validates."""
        a = _RowopApplyArgs()
        a.x, a.y, a.gamma, a.beta, a.stats = (self._ptr(t) for t in (x, y, gamma, beta, stats))
        a.part, a.cls, a.pos, a.emb_f32, a.emb_bf16 = (self._ptr(t) for t in (part, cls, pos, emb_f32, emb_bf16))
        a.rows, a.row0, a.row1, a.stride, a.part_rows = int(rows), int(row0), int(row1), int(stride), int(part_rows)
        a.part_floats = 0 if part is None else int(part.numel())
        a.d, a.B, a.tok, a.eps = int(d), int(B), int(tok), float(eps)
        self._check(self.lib.mme_rowop_apply(self.h, int(self.ROWOPS.get(op, op)), C.byref(a), self._stream()), "mme_rowop_apply")

    SELECT_OPS = {"topk_rows": 0, "topk_candidates": 1, "gemm_topk": 2}

    def select_apply(self, op, *, qsim=None, ld=None, N=None, nrows=None, row0: int = 0, group=None, fetch: int = 1, top_n: int = 1,
                     keep_self: int = 0, min_sim: float = float("-inf"), max_sim: float = float("inf"), idx_out=None, sim_out=None, run_if=None,
                     cand_val=None, cand_idx=None, len=None, cap: int = 0, A=None, W=None, M=None, K=None, thr=None, thr_stride: int = 1,
                     cand_count=None, overflow=None):
        """ONE launch of a step of K12 on the caller's CUDA tensors (mme_select_apply; synchronous, works on a bare context).
        op: a name of SELECT_OPS or its code; which tensors and sizes each op reads is in include/mme.h.  `ld` defaults to
        qsim's row pitch, `nrows` to idx_out's rows, M / K to A's shape and N (op 2) to W's rows.  The library validates."""
        a = _SelectApplyArgs()
        a.qsim, a.group, a.idx_out, a.sim_out, a.run_if = (self._ptr(t) for t in (qsim, group, idx_out, sim_out, run_if))
        a.cand_val, a.cand_idx, a.len, a.A, a.W = (self._ptr(t) for t in (cand_val, cand_idx, len, A, W))
        a.thr, a.cand_count, a.overflow = (self._ptr(t) for t in (thr, cand_count, overflow))
        a.ld = int((qsim.shape[-1] if qsim is not None else 0) if ld is None else ld)
        a.N = int((W.shape[0] if W is not None else 0) if N is None else N)
        a.nrows = int((idx_out.shape[0] if idx_out is not None else 0) if nrows is None else nrows)
        a.row0, a.fetch, a.top_n, a.keep_self, a.cap = int(row0), int(fetch), int(top_n), int(keep_self), int(cap)
        a.M = int((A.shape[0] if A is not None else 0) if M is None else M)
        a.K = int((A.shape[1] if A is not None else 0) if K is None else K)
        a.thr_stride, a.min_sim, a.max_sim = int(thr_stride), float(min_sim), float(max_sim)
        self._check(self.lib.mme_select_apply(self.h, int(self.SELECT_OPS.get(op, op)), C.byref(a), self._stream()), "mme_select_apply")

    CLIP_OPS = {"gemm_qgelu": 0, "gemm_ln_qgelu": 1, "pre_ln": 2, "pool_ln": 3, "l2": 4}

    def clip_apply(self, op, *, A=None, W=None, M=None, N=None, K=None, variant: int = 0, reverse_m: int = 0, bias=None, out=None, ldo=None,
                   ln_stats=None, colsum=None, x=None, gamma=None, beta=None, stats=None, y=None, xf=None, y_f32=None, y_bf16=None,
                   rows: int = 0, d: int = 768, B: int = 0, tok: int = 0, p: int = 0, eps: float = 1e-5):
        """ONE launch of a kernel the CLIP tower adds, on the caller's CUDA tensors (mme_clip_apply; synchronous).  op: a name
        of CLIP_OPS or its code.  The GEMM ops take A bf16 [M, K], W bf16 [N, K], bias, out (+ ln_stats, colsum) as
        `gemm_apply`; the row ops the tensors include/mme.h lists.  The library validates.  -> for the GEMM ops, True when the
        256 x 256 kernel ran; None for the row ops."""
        code = int(self.CLIP_OPS.get(op, op))
        a = _ClipApplyArgs()
        g = None
        if A is not None or W is not None:
            g = self._gemm_args(A, W, M, N, K, variant, reverse_m, bias, out, ldo, ln_stats, colsum)
            a.gemm = C.pointer(g)
        a.x, a.gamma, a.beta, a.stats, a.y, a.xf, a.y_f32, a.y_bf16 = (self._ptr(t) for t in (x, gamma, beta, stats, y, xf, y_f32, y_bf16))
        a.rows, a.d, a.B, a.tok, a.p, a.eps = int(rows), int(d), int(B), int(tok), int(p), float(eps)
        ran = C.c_int32(-1)
        a.ran_256 = C.pointer(ran)
        self._check(self.lib.mme_clip_apply(self.h, code, C.byref(a), self._stream()), "mme_clip_apply")
        return bool(ran.value) if g is not None else None

    SIGLIP_OPS = {"gemm_tgelu": 0, "gemm_ln_tgelu": 1, "embed_rows": 2, "map_pool": 3, "l2_bf16": 4}

    def siglip_apply(self, op, *, A=None, W=None, M=None, N=None, K=None, variant: int = 0, reverse_m: int = 0, bias=None, out=None, ldo=None,
                     ln_stats=None, colsum=None, acc=None, pos=None, x=None, kv=None, q=None, emb_f32=None, emb_bf16=None, n: int = 0, d: int = 768,
                     heads: int = 12):
        """ONE launch of a kernel a SigLIP tower adds, on the caller's CUDA tensors (mme_siglip_apply; synchronous, works on a
        bare context).  op: a name of SIGLIP_OPS or its code.  The GEMM ops take A bf16 [M, K], W bf16 [N, K], bias, out
        (+ ln_stats, colsum) as `gemm_apply`; the others the tensors include/mme.h lists (`bias` and `out` serve both).  The
        library validates.  -> for the GEMM ops, True when the 256 x 256 kernel ran; None otherwise."""
        code = int(self.SIGLIP_OPS.get(op, op))
        a = _SiglipApplyArgs()
        g = None
        if A is not None or W is not None:
            g = self._gemm_args(A, W, M, N, K, variant, reverse_m, bias, out, ldo, ln_stats, colsum)
            a.gemm = C.pointer(g)
        a.acc, a.bias, a.pos, a.x, a.kv, a.q, a.out, a.emb_f32, a.emb_bf16 = (self._ptr(t) for t in (acc, bias, pos, x, kv, q, out, emb_f32, emb_bf16))
        a.n, a.d, a.heads = int(n), int(d), int(heads)
        ran = C.c_int32(-1)
        a.ran_256 = C.pointer(ran)
        self._check(self.lib.mme_siglip_apply(self.h, code, C.byref(a), self._stream()), "mme_siglip_apply")
        return bool(ran.value) if g is not None else None

    VIT32_OPS = {"retile": 0, "embed_rows": 1, "attention": 2, "pool_ln": 3, "pool_ln_l2": 4}

    def vit32_apply(self, op, *, src=None, dst=None, acc=None, bias=None, pos=None, cls=None, x=None, qkv=None, out=None, gamma=None, beta=None,
                    y=None, emb_f32=None, emb_bf16=None, n: int = 0, d: int = 768, heads: int = 12, only_block: int = -1, tok: int = 0,
                    eps: float = 1e-5):
        """ONE launch of a kernel a patch-32 tower adds (ViT/32 @224: 49 patches, 50 tokens), on the caller's CUDA tensors
        (mme_vit32_apply; synchronous, works on a bare context).  op: a name of VIT32_OPS or its code; `n` = crops; which
        tensors each op reads is in include/mme.h.  The library validates."""
        a = _Vit32ApplyArgs()
        a.src, a.dst, a.acc, a.bias, a.pos, a.cls, a.x = (self._ptr(t) for t in (src, dst, acc, bias, pos, cls, x))
        a.qkv, a.out, a.gamma, a.beta, a.y, a.emb_f32, a.emb_bf16 = (self._ptr(t) for t in (qkv, out, gamma, beta, y, emb_f32, emb_bf16))
        a.n, a.d, a.heads, a.only_block, a.tok, a.eps = int(n), int(d), int(heads), int(only_block), int(tok), float(eps)
        self._check(self.lib.mme_vit32_apply(self.h, int(self.VIT32_OPS.get(op, op)), C.byref(a), self._stream()), "mme_vit32_apply")

    TILE_ROWOPS = {"patchify": 0, "assemble": 1, "ln_post": 2, "output": 3, "pool": 4}

    def tile_rowop_apply(self, op, *, pv=None, patches=None, pemb=None, cls=None, pre=None, pos=None, tilepos=None, gamma=None, beta=None, post=None,
                         aid=None, x=None, inter=None, hidden=None, emb_f32=None, emb_bf16=None, npatch: int = 0, rows: int = 0, out_rows: int = 0,
                         inter_stride: int = 0, n: int = 0, ni: int = 0, aspect_rows: int = 9, eps: float = 1e-5):
        """ONE launch of a row kernel of the tile-ViT forward on the caller's CUDA tensors (mme_tile_rowop_apply; synchronous).
        op: a name of TILE_ROWOPS or its code; which tensors and sizes each op reads is in include/mme.h (`aid` is a CUDA
        int32 tensor).  The library validates."""
        a = _TileRowopApplyArgs()
        a.pv, a.patches, a.pemb, a.cls, a.pre, a.pos, a.tilepos, a.gamma = (self._ptr(t) for t in (pv, patches, pemb, cls, pre, pos, tilepos, gamma))
        a.beta, a.post, a.aid, a.x, a.inter, a.hidden, a.emb_f32, a.emb_bf16 = (self._ptr(t) for t in (beta, post, aid, x, inter, hidden, emb_f32, emb_bf16))
        a.npatch, a.rows, a.out_rows, a.inter_stride = int(npatch), int(rows), int(out_rows), int(inter_stride)
        a.n, a.ni, a.aspect_rows, a.eps = int(n), int(ni), int(aspect_rows), float(eps)
        self._check(self.lib.mme_tile_rowop_apply(self.h, int(self.TILE_ROWOPS.get(op, op)), C.byref(a), self._stream()), "mme_tile_rowop_apply")

    def set_chunk(self, crops: int):
        self._check(self.lib.mme_set_chunk(self.h, int(crops)), "mme_set_chunk")

    # ---- hot path ----------------------------------------------------------------------------------
    def _crop_tables(self, offs, hw):
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        hw = np.ascontiguousarray(hw, dtype=np.int32).reshape(-1, 2)
        if len(offs) != len(hw):
            raise ValueError("offs and hw disagree")
        return offs, hw

    def crop_boxes(self, page, boxes, out=None, base: int = 0):
        """page: uint8 CUDA tensor [H, W, 3]; boxes: int array [n, 4] (x0, y0, x1, y1), already int()-truncated.

        Returns (pix uint8 CUDA tensor, offs int64[n], hw int32[n, 2]) ready for `preprocess` / `embed`.  With `out` (a
        uint8 CUDA buffer) the crops are packed into it from byte `base` (a multiple of 16) on and `offs` are offsets
        into `out`: the boxes of several pages fill ONE packed buffer (RegionProcessor.process_regions)."""
        t = self.torch
        if page.dtype != t.uint8 or page.dim() != 3 or page.shape[2] != 3 or not page.is_contiguous():
            raise MmeError("crop_boxes: page must be a contiguous uint8 [H, W, 3] tensor")
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        n = len(b)
        b64 = b.astype(np.int64)  # corners are any int32: the difference of two needs 33 bits
        hw64 = np.stack([b64[:, 3] - b64[:, 1], b64[:, 2] - b64[:, 0]], axis=1)
        if n and (hw64.min() <= 0 or hw64.max() > 8000):
            i = int(np.flatnonzero(((hw64 <= 0) | (hw64 > 8000)).any(axis=1))[0])
            raise MmeError(f"crop_boxes: box {i} is {hw64[i, 1]}x{hw64[i, 0]} (w x h); every box must be 1..8000 pixels wide and high after int() truncation")
        hw = np.ascontiguousarray(hw64.astype(np.int32)) if n else np.zeros((0, 2), np.int32)
        offs, _, total = packed_layout(hw)  # `total` counts the 16 bytes behind the last crop
        if out is not None:
            if out.dtype != t.uint8 or not out.is_contiguous() or out.device != page.device or base % 16 or base < 0 or base + total > out.numel():
                raise MmeError("crop_boxes: `out` must be a contiguous uint8 buffer on the page's device with room for the crops (+16 B) from a 16-byte aligned `base`")
            pix, offs = out, offs + int(base)
        else:
            pix = t.empty(total, dtype=t.uint8, device=page.device)
        self._check(self.lib.mme_crop_boxes(self.h, page.data_ptr(), int(page.shape[0]), int(page.shape[1]), b.ctypes.data, n,
                                            pix.data_ptr(), offs.ctypes.data, self._stream()), "mme_crop_boxes")
        return pix, offs, hw

    def lanczos_resize(self, src, new_h: int, new_w: int, out=None, *, pitch=None, work=None):
        """`Image.fromarray(src).resize((new_w, new_h), Image.LANCZOS)` on the device, bit for bit (mme_lanczos_resize: the
        8000-pixel cap of embedder.py:110-114).  src: a uint8 CUDA tensor [h, w, 3] whose pixels are 3 bytes apart and whose
        rows are `pitch` bytes apart (default: the tensor's own row stride, so a box sliced out of a page `page[y0:y1, x0:x1]`
        is a valid source).  out: a uint8 CUDA buffer of new_h * new_w * 3 elements (any address), made when None.
        work: caller-owned uint8 CUDA scratch of at least `lanczos_workspace(...)` bytes, made when None.
        -> out as [new_h, new_w, 3].  Asynchronous on the current stream apart from the upload of the tables."""
        t = self.torch
        if not isinstance(src, t.Tensor) or src.dtype != t.uint8 or src.dim() != 3 or src.shape[2] != 3 or not src.is_cuda:
            raise MmeError("lanczos_resize: src must be a uint8 CUDA tensor [h, w, 3]")
        h, w = int(src.shape[0]), int(src.shape[1])
        if h < 1 or w < 1 or src.stride(2) != 1 or src.stride(1) != 3:
            raise MmeError("lanczos_resize: src must hold at least one pixel, its pixels 3 bytes apart")
        pitch = int(src.stride(0) if pitch is None else pitch)
        new_h, new_w = int(new_h), int(new_w)
        check_lanczos_geometry(h, w, new_h, new_w)
        if pitch < 3 * w:
            raise MmeError(f"lanczos_resize: pitch = {pitch}; at least 3 * w = {3 * w} is required")
        need = lanczos_workspace(h, w, new_h, new_w)
        if work is None:
            work = t.empty(need, dtype=t.uint8, device=src.device)
        elif work.dtype != t.uint8 or not work.is_contiguous() or work.device != src.device or work.numel() < need:
            raise MmeError(f"lanczos_resize: `work` must be a contiguous uint8 buffer of at least {need} bytes on the source's device")
        if out is None:
            out = t.empty((new_h, new_w, 3), dtype=t.uint8, device=src.device)
        elif out.dtype != t.uint8 or not out.is_contiguous() or out.device != src.device or out.numel() != new_h * new_w * 3:
            raise MmeError(f"lanczos_resize: `out` must be a contiguous uint8 buffer of {new_h} * {new_w} * 3 elements on the source's device")
        self._check(self.lib.mme_lanczos_resize(self.h, src.data_ptr(), pitch, h, w, out.data_ptr(), new_h, new_w, work.data_ptr(), int(work.numel()),
                                                self._stream()), "mme_lanczos_resize")
        return out.view(new_h, new_w, 3)

    def nms_boxes(self, boxes, scores, classes, page_offs, iou_threshold=0.5):
        """K13 (3_combine_grids.py:80-137) over many pages: host arrays in, list of kept page-local index arrays out
        (the reference's output order)."""
        boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 4))
        scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
        classes = np.ascontiguousarray(classes, dtype=np.int32).reshape(-1)
        page_offs = np.ascontiguousarray(page_offs, dtype=np.int32).reshape(-1)
        pages = len(page_offs) - 1
        n = len(scores)
        if pages < 0 or len(boxes) != n or len(classes) != n or (pages >= 0 and int(page_offs[-1]) != n):
            raise MmeError("nms_boxes: boxes / scores / classes / page_offs disagree")
        keep = np.full(n, -1, dtype=np.int32)
        count = np.zeros(max(pages, 0), dtype=np.int32)
        self._check(self.lib.mme_nms_boxes(self.h, boxes.ctypes.data, scores.ctypes.data, classes.ctypes.data, page_offs.ctypes.data,
                                           pages, float(iou_threshold), keep.ctypes.data, count.ctypes.data, self._stream()), "mme_nms_boxes")
        return [keep[page_offs[p] : page_offs[p] + count[p]].copy() for p in range(pages)]

    def preprocess(self, pix, offs, hw):
        """pix: uint8 CUDA tensor (concatenated HWC crops, >=16 spare bytes at the end).  -> bf16 patches of the loaded
        geometry: [n * 196, 768] at patch 16, [n * 49, 3072] at patch 32 (the same bytes per crop), [n * 256, 640] at patch 14
        (588 values of a patch, zero columns behind)."""
        t = self.torch
        offs, hw = self._crop_tables(offs, hw)
        n = len(offs)
        g = self.vit_geometry()
        patches = t.empty((n * g.num_patches, (g.patch_dim + 63) // 64 * 64), dtype=t.bfloat16, device=pix.device)
        self._check(self.lib.mme_preprocess(self.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, n, patches.data_ptr(), self._stream()), "mme_preprocess")
        return patches

    def preprocess_tiles(self, pix, offs, hw, tile=560, max_tiles=4, out=None):
        """Mllama multi-tile preprocessing of packed crops -> (pixel_values f32 CUDA [n, max_tiles, 3, tile, tile],
        aspect_ratio_ids int64[n], aspect_ratio_mask int64[n, max_tiles], num_tiles list[int]).  `out`, if given, is the
        contiguous f32 tensor of that shape on pix's device that receives the pixel values (and is returned).  A crop
        whose height shrinks by a factor above 79 (a vertical window of more than 160 taps) is refused (include/mme.h)."""
        t = self.torch
        offs, hw = self._crop_tables(offs, hw)
        n = len(offs)
        if out is None:
            out = t.empty((n, max_tiles, 3, tile, tile), dtype=t.float32, device=pix.device)
        elif out.dtype != t.float32 or not out.is_contiguous() or out.device != pix.device or tuple(out.shape) != (n, max_tiles, 3, tile, tile):
            raise MmeError(f"preprocess_tiles: `out` must be a contiguous float32 tensor [{n}, {max_tiles}, 3, {tile}, {tile}] on the crops' device")
        ids = np.zeros(n, dtype=np.int32)
        nt = np.zeros(n, dtype=np.int32)
        self._check(self.lib.mme_preprocess_tiles(self.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, n, int(tile), int(max_tiles),
                                                  out.data_ptr(), ids.ctypes.data, nt.ctypes.data, self._stream()), "mme_preprocess_tiles")
        mask = (np.arange(max_tiles)[None, :] < nt[:, None]).astype(np.int64)
        return out, ids.astype(np.int64), mask, nt.tolist()

    def vit_forward(self, patches, pool_token: int = 0, want_f32: bool = True, want_bf16: bool = True, grids=None):
        """`grids`: under pooling "mean" / "cls+mean", a host int32 array [n, 2] of covered grids (R, C) (mme_vit_forward_grids;
        pool_token is not used); without it the mean modes pool whole grids."""
        t = self.torch
        g = self.vit_geometry()
        n, d = patches.shape[0] // g.num_patches, self.embed_dim
        e32 = t.empty((n, d), dtype=t.float32, device=patches.device) if want_f32 else None
        e16 = t.empty((n, d), dtype=t.bfloat16, device=patches.device) if want_bf16 else None
        if grids is not None:
            grids = np.ascontiguousarray(grids, dtype=np.int32).reshape(-1, 2)
            if len(grids) != n:
                raise ValueError(f"grids holds {len(grids)} rows for {n} crops")
            self._check(self.lib.mme_vit_forward_grids(self.h, patches.data_ptr(), n, grids.ctypes.data, e32.data_ptr() if want_f32 else None,
                                                       e16.data_ptr() if want_bf16 else None, self._stream()), "mme_vit_forward_grids")
            return e32, e16
        self._check(self.lib.mme_vit_forward(self.h, patches.data_ptr(), n, int(pool_token), e32.data_ptr() if want_f32 else None,
                                             e16.data_ptr() if want_bf16 else None, self._stream()), "mme_vit_forward")
        return e32, e16

    def embed(self, pix, offs, hw, pool_token: int = 0, out_f32=None, out_bf16=None, want_f32: bool = True, want_bf16: bool = True):
        t = self.torch
        offs, hw = self._crop_tables(offs, hw)
        n = len(offs)
        e32 = out_f32 if out_f32 is not None else (t.empty((n, self.embed_dim), dtype=t.float32, device=pix.device) if want_f32 else None)
        e16 = out_bf16 if out_bf16 is not None else (t.empty((n, self.embed_dim), dtype=t.bfloat16, device=pix.device) if want_bf16 else None)
        self._check(self.lib.mme_embed(self.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, n, int(pool_token),
                                       e32.data_ptr() if e32 is not None else None, e16.data_ptr() if e16 is not None else None,
                                       self._stream()), "mme_embed")
        return e32, e16

    def _token_window(self, tok0, ntok):
        """The default window is the patch tokens: from 1 where the tower has a class token (ViT, CLIP, DINOv2), from 0 for SigLIP."""
        g = self.vit_geometry()
        first = 0 if self.encoder_info()["kind"] == "siglip" else 1
        tok0 = first if tok0 is None else int(tok0)
        ntok = g.num_patches + first - tok0 if ntok is None else int(ntok)
        return tok0, ntok, g

    def _token_out(self, out, n, ntok, hidden, device):
        t = self.torch
        if out is None:
            return t.empty((n, max(ntok, 0), hidden), dtype=t.bfloat16, device=device)
        if out.dtype != t.bfloat16 or not out.is_contiguous() or out.device != device or tuple(out.shape) != (n, ntok, hidden):
            raise MmeError(f"token rows: `out` must be a contiguous bfloat16 tensor [{n}, {ntok}, {hidden}] on the input's device")
        return out

    def vit_tokens(self, patches, pool_token: int = 0, tok0=None, ntok=None, out=None, want_f32: bool = True, want_bf16: bool = True):
        """vit_forward that also returns the final-LayerNorm, L2-normalised token rows tok0 .. tok0 + ntok - 1 of every crop
        (mme_vit_tokens; default: the patch tokens) -> (tokens bf16 [n, ntok, hidden], emb_f32, emb_bf16)."""
        t = self.torch
        tok0, ntok, g = self._token_window(tok0, ntok)
        n, d = patches.shape[0] // g.num_patches, self.embed_dim
        tokens = self._token_out(out, n, ntok, g.hidden_size, patches.device)
        e32 = t.empty((n, d), dtype=t.float32, device=patches.device) if want_f32 else None
        e16 = t.empty((n, d), dtype=t.bfloat16, device=patches.device) if want_bf16 else None
        self._check(self.lib.mme_vit_tokens(self.h, patches.data_ptr(), n, int(pool_token), tok0, ntok, tokens.data_ptr(),
                                            e32.data_ptr() if want_f32 else None, e16.data_ptr() if want_bf16 else None, self._stream()), "mme_vit_tokens")
        return tokens, e32, e16

    def embed_tokens(self, pix, offs, hw, pool_token: int = 0, tok0=None, ntok=None, out=None, out_f32=None, out_bf16=None, want_f32: bool = True,
                     want_bf16: bool = True):
        """embed that also returns the token rows (mme_embed_tokens), as vit_tokens."""
        t = self.torch
        offs, hw = self._crop_tables(offs, hw)
        n = len(offs)
        tok0, ntok, g = self._token_window(tok0, ntok)
        tokens = self._token_out(out, n, ntok, g.hidden_size, pix.device)
        e32 = out_f32 if out_f32 is not None else (t.empty((n, self.embed_dim), dtype=t.float32, device=pix.device) if want_f32 else None)
        e16 = out_bf16 if out_bf16 is not None else (t.empty((n, self.embed_dim), dtype=t.bfloat16, device=pix.device) if want_bf16 else None)
        self._check(self.lib.mme_embed_tokens(self.h, pix.data_ptr(), offs.ctypes.data, hw.ctypes.data, n, int(pool_token), tok0, ntok,
                                              tokens.data_ptr(), e32.data_ptr() if e32 is not None else None,
                                              e16.data_ptr() if e16 is not None else None, self._stream()), "mme_embed_tokens")
        return tokens, e32, e16

    def normalise_rows(self, x):
        """f32 CUDA tensor [n,d] -> L2-normalised bf16 [n,d]."""
        t = self.torch
        x = x.contiguous()
        y = t.empty(x.shape, dtype=t.bfloat16, device=x.device)
        self._check(self.lib.mme_normalise_rows(self.h, x.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), self._stream()), "mme_normalise_rows")
        return y

    def cosine(self, a, b=None, out=None):
        """a [m,d], b [n,d] bf16 CUDA tensors of L2-normalised rows -> f32 [m,n]."""
        t = self.torch
        b = a if b is None else b
        m, d = a.shape
        n = b.shape[0]
        if out is None:
            out = t.empty((m, n), dtype=t.float32, device=a.device)
        assert a.dtype == t.bfloat16 and b.dtype == t.bfloat16 and a.is_contiguous() and b.is_contiguous()
        self._check(self.lib.mme_cosine(self.h, a.data_ptr(), m, b.data_ptr(), n, d, out.data_ptr(), out.stride(0), self._stream()), "mme_cosine")
        return out

    def cosine_bf16(self, a, b=None, out=None):
        """as `cosine`, S rounded to bf16 (mme_cosine_bf16): half the bytes; bit-equal to `cosine(...).to(bfloat16)`."""
        t = self.torch
        b = a if b is None else b
        m, d = a.shape
        n = b.shape[0]
        if out is None:
            out = t.empty((m, (n + 7) // 8 * 8), dtype=t.bfloat16, device=a.device)[:, :n]
        assert a.dtype == t.bfloat16 and b.dtype == t.bfloat16 and a.is_contiguous() and b.is_contiguous() and out.dtype == t.bfloat16
        self._check(self.lib.mme_cosine_bf16(self.h, a.data_ptr(), m, b.data_ptr(), n, d, out.data_ptr(), out.stride(0), self._stream()), "mme_cosine_bf16")
        return out

    def page_similarity(self, emb, area_pct, valid, page_offs, skip=None, *, max_query=10, top_k=10, max_dist=0.9, metric=0, normalise=True,
                        pair_range=None):
        """pair_range=(lo, hi): only those upper-triangle pair ranks, raw and zero elsewhere (one rank's shard)."""
        t = self.torch
        N, d = emb.shape
        page_offs = np.ascontiguousarray(page_offs, dtype=np.int32)
        P = len(page_offs) - 1
        S = t.empty((P, P), dtype=t.float64, device=emb.device)
        if pair_range is not None:
            self._check(self.lib.mme_page_similarity_pairs(self.h, emb.data_ptr(), N, d, area_pct.data_ptr(), valid.data_ptr(), page_offs.ctypes.data,
                                                           P, skip.data_ptr() if skip is not None else None, int(max_query), int(top_k),
                                                           float(max_dist), int(metric), int(pair_range[0]), int(pair_range[1]), S.data_ptr(),
                                                           self._stream()), "mme_page_similarity_pairs")
            return S
        self._check(self.lib.mme_page_similarity(self.h, emb.data_ptr(), N, d, area_pct.data_ptr(), valid.data_ptr(), page_offs.ctypes.data, P,
                                                 skip.data_ptr() if skip is not None else None, int(max_query), int(top_k), float(max_dist),
                                                 int(metric), int(bool(normalise)), S.data_ptr(), self._stream()), "mme_page_similarity")
        return S

    def cluster_pages(self, S, n_clusters=None, mode="reference_fallback"):
        """S: numpy f64 [P,P] (unit diagonal) or CUDA f64 tensor -> (labels int list, k, [(k, silhouette)...])."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        Sd = S if isinstance(S, t.Tensor) else t.from_numpy(np.ascontiguousarray(S, dtype=np.float64)).to(dev)
        Sd = Sd.contiguous()
        P = Sd.shape[0]
        if P < 2:
            raise MmeError("cluster_pages needs at least 2 pages")
        labels = t.empty(P, dtype=t.int32, device=dev)
        k = t.empty(1, dtype=t.int32, device=dev)
        scores = t.empty(16, dtype=t.float64, device=dev)
        m = {"reference_fallback": 0, "precomputed": 1}[mode]
        self._check(self.lib.mme_cluster_pages(self.h, Sd.data_ptr(), P, int(n_clusters or 0), m, labels.data_ptr(), k.data_ptr(),
                                               scores.data_ptr(), self._stream()), "mme_cluster_pages")
        sc = scores.cpu().numpy()
        return labels.cpu().numpy().tolist(), int(k.item()), [(i, float(sc[i])) for i in range(2, 16) if sc[i] == sc[i]]

    def set_neighbour_mode(self, mode):
        """0 / "auto", 1 / "block", 2 / "fused" (see mme.h)."""
        m = {"auto": 0, "block": 1, "fused": 2}.get(mode, mode)
        self._check(self.lib.mme_set_neighbour_mode(self.h, int(m)), "mme_set_neighbour_mode")

    def neighbours(self, emb_bf16, group=None, *, row0=0, nrows=None, fetch=30, top_n=10, keep_self=False,
                   min_sim=-float("inf"), max_sim=float("inf")):
        """Ranked neighbour lists of rows [row0, row0+nrows) of the normalised bf16 rows emb_bf16[N, d].

        group: optional int32[N] (CUDA tensor or array); rows with the query's group id are dropped.
        Returns (idx int32[nrows, top_n] padded with -1, sim float32[nrows, top_n]) CUDA tensors."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != dev:
            raise MmeError("neighbours: emb must be a 2-D bfloat16 tensor on this engine's device")
        N, d = e.shape
        nrows = N - row0 if nrows is None else int(nrows)
        g = None
        if group is not None:
            g = group if isinstance(group, t.Tensor) else t.from_numpy(np.ascontiguousarray(group, dtype=np.int32))
            g = g.to(device=dev, dtype=t.int32).contiguous()
            if g.numel() != N:
                raise MmeError("neighbours: group must have one id per row")
        idx = t.empty((max(nrows, 0), top_n), dtype=t.int32, device=dev)
        sim = t.empty((max(nrows, 0), top_n), dtype=t.float32, device=dev)
        self._check(self.lib.mme_neighbours(self.h, e.data_ptr(), N, d, g.data_ptr() if g is not None else None, int(row0), nrows,
                                            int(fetch), int(top_n), int(bool(keep_self)), float(min_sim), float(max_sim),
                                            idx.data_ptr(), sim.data_ptr(), self._stream()), "mme_neighbours")
        return idx, sim

    # ---- K14 near-duplicate groups (mme.h, mme_duplicates_*) ----
    def _dup_struct(self, state):
        st = _DupState()
        for f in ("parent", "degree", "best", "page_pairs", "edges", "edge_sim", "counters"):
            setattr(st, f, self._ptr(state.get(f)))
        st.edge_cap, st.P = int(state.get("edge_cap", 0)), int(state.get("pages", 0))
        return st

    def _i32_rows(self, v, N, what, who="duplicates"):
        """optional int32 [N] control vector (CUDA tensor or array) on this engine's device"""
        if v is None:
            return None
        t = self.torch
        g = v if isinstance(v, t.Tensor) else t.from_numpy(np.ascontiguousarray(v, dtype=np.int32))
        g = g.to(device=t.device(f"cuda:{self.device}"), dtype=t.int32).contiguous()
        if g.numel() != N:
            raise MmeError(f"{who}: {what} must have one id per row")
        return g

    def duplicates_init(self, N, pages=0, edge_cap=0):
        """A fresh state for N rows: a dict of CUDA tensors `parent`, `degree` int32 [N], `best` int64 [N] (packed keys),
        `counters` int64 [2] (edges found, edges written), `page_pairs` int32 [pages, pages] when pages > 0, `edges`
        int32 [edge_cap, 2] and `edge_sim` float32 [edge_cap] when edge_cap > 0; plus `N`, `pages`, `edge_cap`."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        N, pages, edge_cap = int(N), int(pages), int(edge_cap)
        state = {"N": N, "pages": pages, "edge_cap": edge_cap,
                 "parent": t.empty(max(N, 1), dtype=t.int32, device=dev), "degree": t.empty(max(N, 1), dtype=t.int32, device=dev),
                 "best": t.empty(max(N, 1), dtype=t.int64, device=dev), "counters": t.empty(2, dtype=t.int64, device=dev)}
        if pages > 0:
            state["page_pairs"] = t.empty((pages, pages), dtype=t.int32, device=dev)
        if edge_cap > 0:
            state["edges"] = t.zeros((edge_cap, 2), dtype=t.int32, device=dev)
            state["edge_sim"] = t.zeros(edge_cap, dtype=t.float32, device=dev)
        self._check(self.lib.mme_duplicates_init(self.h, C.byref(self._dup_struct(state)), N, self._stream()), "mme_duplicates_init")
        return state

    def duplicates_scan(self, state, emb_bf16, group=None, page_of=None, *, min_sim, row0=0, nrows=None):
        """Adds the edges (i, j), row0 <= i < row0 + nrows, i < j < N, to `state`.  Scans over disjoint row ranges that
        cover [0, N) are one whole run, in any order."""
        t = self.torch
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != t.device(f"cuda:{self.device}"):
            raise MmeError("duplicates: emb must be a 2-D bfloat16 tensor on this engine's device")
        N, d = e.shape
        if N != state["N"]:
            raise MmeError(f"duplicates: the state was made for {state['N']} rows, emb has {N}")
        nrows = N - row0 if nrows is None else int(nrows)
        g, p = self._i32_rows(group, N, "group"), self._i32_rows(page_of, N, "page_of")
        self._check(self.lib.mme_duplicates_scan(self.h, e.data_ptr(), N, d, self._ptr(g), self._ptr(p), float(min_sim), int(row0), nrows,
                                                 C.byref(self._dup_struct(state)), self._stream()), "mme_duplicates_scan")

    def duplicates_merge(self, dst, src):
        """dst <- dst and src (two states over the same rows, e.g. row shards of two GPUs).  Edge lists are not merged."""
        if dst["N"] != src["N"]:
            raise MmeError(f"duplicates: merge of states for {dst['N']} and {src['N']} rows")
        self._check(self.lib.mme_duplicates_merge(self.h, C.byref(self._dup_struct(dst)), C.byref(self._dup_struct(src)), dst["N"], self._stream()),
                    "mme_duplicates_merge")

    def duplicates_finish(self, state):
        """The outputs by name, CUDA tensors: labels, degree, best_idx int32 [N], best_sim float32 [N], summary int64 [4]
        (edges, groups of >= 2 rows, rows in such groups, rows of the largest group), counters int64 [2], and page_pairs /
        edges / edge_sim where the state has them (edges[:counters[1]] are valid).  The state's own tensors are returned,
        not copies."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        N = state["N"]
        out = {"labels": t.empty(N, dtype=t.int32, device=dev), "best_idx": t.empty(N, dtype=t.int32, device=dev),
               "best_sim": t.empty(N, dtype=t.float32, device=dev), "summary": t.empty(4, dtype=t.int64, device=dev)}
        self._check(self.lib.mme_duplicates_finish(self.h, C.byref(self._dup_struct(state)), N, self._ptr(out["labels"]) if N else None,
                                                   self._ptr(out["best_idx"]) if N else None, self._ptr(out["best_sim"]) if N else None,
                                                   out["summary"].data_ptr(), self._stream()), "mme_duplicates_finish")
        out["degree"] = state["degree"][:N]
        out["counters"] = state["counters"]
        for k in ("page_pairs", "edges", "edge_sim"):
            if k in state:
                out[k] = state[k]
        return out

    def duplicates(self, emb, group=None, page_of=None, pages=0, *, min_sim, rows=None, edge_cap=0):
        """Near-duplicate groups of the L2-normalised bf16 rows emb[N, d] in one call: init, scan of `rows` = (row0, nrows)
        (default: all rows), finish.  See duplicates_finish for what comes back."""
        state = self.duplicates_init(emb.shape[0], pages=pages, edge_cap=edge_cap)
        row0, nrows = (0, None) if rows is None else rows
        self.duplicates_scan(state, emb, group, page_of, min_sim=min_sim, row0=row0, nrows=nrows)
        return self.duplicates_finish(state)

    # ---- K18 density clusters (mme.h, mme_density_*) ----
    def _density_struct(self, state):
        st = _DensityState()
        for f in ("count", "parent", "border", "counters"):
            setattr(st, f, self._ptr(state.get(f)))
        return st

    def density_init(self, N):
        """A fresh state for N rows: a dict of CUDA tensors `count`, `parent` int32 [N], `border` int64 [N] (packed keys),
        `counters` int64 [2] (neighbour pairs the count calls found, pairs the link calls saw); plus `N`."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        N = int(N)
        state = {"N": N, "count": t.empty(max(N, 1), dtype=t.int32, device=dev), "parent": t.empty(max(N, 1), dtype=t.int32, device=dev),
                 "border": t.empty(max(N, 1), dtype=t.int64, device=dev), "counters": t.empty(2, dtype=t.int64, device=dev)}
        self._check(self.lib.mme_density_init(self.h, C.byref(self._density_struct(state)), N, self._stream()), "mme_density_init")
        return state

    def _density_table(self, state, emb_bf16, group):
        t = self.torch
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != t.device(f"cuda:{self.device}"):
            raise MmeError("density: emb must be a 2-D bfloat16 tensor on this engine's device")
        if e.shape[0] != state["N"]:
            raise MmeError(f"density: the state was made for {state['N']} rows, emb has {e.shape[0]}")
        g = self._i32_rows(group, e.shape[0], "group", who="density")
        return e, g

    def density_count(self, state, emb_bf16, group=None, *, min_sim, row0=0, nrows=None):
        """Counts the neighbour pairs (i, j), row0 <= i < row0 + nrows, i < j < N, into `state`.  Calls over disjoint row
        ranges that cover [0, N) are one count, in any order."""
        e, g = self._density_table(state, emb_bf16, group)
        N, d = e.shape
        nrows = N - row0 if nrows is None else int(nrows)
        self._check(self.lib.mme_density_count(self.h, e.data_ptr(), N, d, self._ptr(g), float(min_sim), int(row0), nrows,
                                               C.byref(self._density_struct(state)), self._stream()), "mme_density_count")

    def density_link(self, state, emb_bf16, group=None, *, min_sim, min_samples, row0=0, nrows=None):
        """Links the same pairs: unions of two core rows, border offers of one.  Call it only after the count calls have
        covered every row (on the same stream), with the same emb, group and min_sim."""
        e, g = self._density_table(state, emb_bf16, group)
        N, d = e.shape
        nrows = N - row0 if nrows is None else int(nrows)
        self._check(self.lib.mme_density_link(self.h, e.data_ptr(), N, d, self._ptr(g), float(min_sim), int(min_samples), int(row0), nrows,
                                              C.byref(self._density_struct(state)), self._stream()), "mme_density_link")

    def density_finish(self, state, *, min_samples):
        """The outputs by name, CUDA tensors: labels (the cluster's smallest core row, -1 for noise), kind (2 core, 1 border,
        0 noise), count, border_idx int32 [N], border_sim float32 [N], summary int64 [6] (neighbour pairs, clusters, core,
        border, noise rows, rows of the largest cluster) and counters int64 [2].  count and counters are the state's own."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        N = state["N"]
        out = {"labels": t.empty(N, dtype=t.int32, device=dev), "kind": t.empty(N, dtype=t.int32, device=dev),
               "border_idx": t.empty(N, dtype=t.int32, device=dev), "border_sim": t.empty(N, dtype=t.float32, device=dev),
               "summary": t.empty(6, dtype=t.int64, device=dev)}
        ptr = lambda k: self._ptr(out[k]) if N else None  # noqa: E731
        self._check(self.lib.mme_density_finish(self.h, C.byref(self._density_struct(state)), N, int(min_samples), ptr("labels"), ptr("kind"),
                                                ptr("border_idx"), ptr("border_sim"), out["summary"].data_ptr(), self._stream()), "mme_density_finish")
        out["count"] = state["count"][:N]
        out["counters"] = state["counters"]
        return out

    def density_clusters(self, emb, min_sim, min_samples, group=None):
        """DBSCAN of the L2-normalised bf16 rows emb[N, d] in one call: init, count, link, finish, all enqueued on the current
        stream.  See density_finish for what comes back."""
        state = self.density_init(emb.shape[0])
        self.density_count(state, emb, group, min_sim=min_sim)
        self.density_link(state, emb, group, min_sim=min_sim, min_samples=min_samples)
        return self.density_finish(state, min_samples=min_samples)

    # ---- K19 cluster hierarchy (mme.h, mme_hierarchy_*) ----
    def _hierarchy_struct(self, state):
        st = _HierarchyState()
        for f in _HIERARCHY_FIELDS:
            setattr(st, f, self._ptr(state.get(f)))
        return st

    def hierarchy_init(self, N):
        """A fresh state for N rows: a dict of CUDA tensors `core` float32 and `comp` int32 [N rounded up to 4], `row_key`,
        `comp_edge` int64 [N] (packed keys), `parent`, `comp_weight` int32 [N], `edges` int32 [N - 1, 2], `weights` float32
        [N - 1], `counters` int64 [3] (edges emitted, rounds run, components left); plus `N`."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        N = int(N)
        n1, n4 = max(N, 1), max((N + 3) & ~3, 4)
        state = {"N": N, "core": t.empty(n4, dtype=t.float32, device=dev), "comp": t.empty(n4, dtype=t.int32, device=dev),
                 "row_key": t.empty(n1, dtype=t.int64, device=dev), "parent": t.empty(n1, dtype=t.int32, device=dev),
                 "comp_weight": t.empty(n1, dtype=t.int32, device=dev), "comp_edge": t.empty(n1, dtype=t.int64, device=dev),
                 "edges": t.zeros((max(N - 1, 1), 2), dtype=t.int32, device=dev), "weights": t.zeros(max(N - 1, 1), dtype=t.float32, device=dev),
                 "counters": t.empty(3, dtype=t.int64, device=dev)}
        self._check(self.lib.mme_hierarchy_init(self.h, C.byref(self._hierarchy_struct(state)), N, self._stream()), "mme_hierarchy_init")
        return state

    def _hierarchy_table(self, state, emb_bf16, group):
        t = self.torch
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != t.device(f"cuda:{self.device}"):
            raise MmeError("hierarchy: emb must be a 2-D bfloat16 tensor on this engine's device")
        if e.shape[0] != state["N"]:
            raise MmeError(f"hierarchy: the state was made for {state['N']} rows, emb has {e.shape[0]}")
        return e, self._i32_rows(group, e.shape[0], "group", who="hierarchy")

    def hierarchy_core(self, state, emb_bf16, group=None, *, min_samples, row0=0, nrows=None):
        """core[i], row0 <= i < row0 + nrows: the (min_samples - 1)-th largest admissible cosine of the row.  Calls over row
        ranges that cover [0, N) fill `core`, in any order; all of them come before the first hierarchy_scan."""
        e, g = self._hierarchy_table(state, emb_bf16, group)
        N, d = e.shape
        nrows = N - row0 if nrows is None else int(nrows)
        self._check(self.lib.mme_hierarchy_core(self.h, e.data_ptr(), N, d, self._ptr(g), int(min_samples), int(row0), nrows,
                                                C.byref(self._hierarchy_struct(state)), self._stream()), "mme_hierarchy_core")

    def hierarchy_scan(self, state, emb_bf16, group=None, *, row0=0, nrows=None):
        """One round's scan of the rows row0 <= i < row0 + nrows against every row.  Calls over disjoint row ranges that cover
        [0, N) are one round's scan, in any order; then hierarchy_merge ends the round."""
        e, g = self._hierarchy_table(state, emb_bf16, group)
        N, d = e.shape
        nrows = N - row0 if nrows is None else int(nrows)
        self._check(self.lib.mme_hierarchy_scan(self.h, e.data_ptr(), N, d, self._ptr(g), int(row0), nrows,
                                                C.byref(self._hierarchy_struct(state)), self._stream()), "mme_hierarchy_scan")

    def hierarchy_merge(self, state):
        """Ends a round: emits every component's maximal edge, unites, renews `comp`, updates `counters`.  Enqueues only."""
        self._check(self.lib.mme_hierarchy_merge(self.h, C.byref(self._hierarchy_struct(state)), state["N"], self._stream()), "mme_hierarchy_merge")

    def hierarchy_rounds(self, state, scan):
        """The round loop: `scan()` enqueues one round's scans, then the merge; repeated until the forest is whole or a round
        emits no edge.  The number of rounds depends on the data, so the edge counter (8 bytes) is read back once per round:
        the one synchronisation per round.  -> (edges emitted, rounds run)."""
        N = state["N"]
        edges, rounds = 0, 0
        while edges < N - 1 and rounds <= max(N - 1, 1).bit_length():  # at most ceil(log2 N) rounds emit edges
            scan()
            self.hierarchy_merge(state)
            rounds += 1
            now = int(state["counters"][0].item())
            if now == edges:
                break
            edges = now
        return edges, rounds

    def hierarchy_sorted(self, state, n_edges):
        """(edges int32 [E, 2], weights float32 [E]) of the state, as copies sorted by the order of the tree: weight descending
        (on the order-preserving image of the f32), then lo, then hi ascending."""
        t = self.torch
        e, w = state["edges"][:n_edges], state["weights"][:n_edges]
        if n_edges == 0:
            return e.clone(), w.clone()
        pair = (e[:, 0].to(t.int64) << 32) | e[:, 1].to(t.int64)
        order = t.sort(pair, stable=True)[1]
        u = w.view(t.int32).to(t.int64) & 0xFFFFFFFF
        image = t.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
        order = order[t.sort(image[order], descending=True, stable=True)[1]]
        return e[order].contiguous(), w[order].contiguous()

    def hierarchy(self, emb, min_samples, group=None):
        """The mutual-reachability spanning forest of the L2-normalised bf16 rows emb[N, d] in one call: init, core, then rounds
        of scan and merge on the current stream (hierarchy_rounds: one 8-byte read-back per round).  -> dict of CUDA tensors
        `edges` int32 [E, 2] (lo, hi) and `weights` float32 [E], sorted by weight descending, then lo, then hi; `core` float32
        [N]; and the ints `rounds` and `components` (E = N - components)."""
        state = self.hierarchy_init(emb.shape[0])
        self.hierarchy_core(state, emb, group, min_samples=min_samples)
        n_edges, rounds = self.hierarchy_rounds(state, lambda: self.hierarchy_scan(state, emb, group))
        edges, weights = self.hierarchy_sorted(state, n_edges)
        return {"edges": edges, "weights": weights, "core": state["core"][:state["N"]], "rounds": rounds, "components": state["N"] - n_edges}

    # ---- K15 spherical k-means (mme.h, mme_kmeans*) ----
    def kmeans(self, emb_bf16, k, init_rows=None, centroids=None, max_iter=100):
        """Spherical k-means of the L2-normalised bf16 rows emb_bf16[N, d] into k clusters (mme_kmeans; enqueues and returns).
        The start is `init_rows` (k distinct rows of emb) or `centroids` (bf16 [k, d], copied), exactly one of them.
        max_iter = 0 assigns the rows to the given centroids.  -> KmeansResult of CUDA tensors; counts and sums are those
        of the last update (zero with max_iter = 0).  The library validates N, d, k, max_iter and the rows."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != dev:
            raise MmeError("kmeans: emb must be a 2-D bfloat16 tensor on this engine's device")
        if (init_rows is None) == (centroids is None):
            raise MmeError("kmeans: give exactly one of init_rows and centroids")
        N, d = e.shape
        k = int(k)
        rows = None
        if init_rows is not None:
            rows = np.ascontiguousarray(np.asarray(init_rows).reshape(-1), dtype=np.int32)
            if rows.size != k:
                raise MmeError(f"kmeans: init_rows has {rows.size} rows, k = {k}")
            cen = t.zeros((max(k, 1), d), dtype=t.bfloat16, device=dev)
        else:
            if centroids.dtype != t.bfloat16 or centroids.dim() != 2 or tuple(centroids.shape) != (k, d):
                raise MmeError(f"kmeans: centroids must be a bfloat16 tensor [k = {k}, d = {d}], got {centroids.dtype} {tuple(centroids.shape)}")
            cen = centroids.to(dev).contiguous().clone()
        res = KmeansResult(labels=t.empty(max(N, 1), dtype=t.int32, device=dev)[:N], sim=t.empty(max(N, 1), dtype=t.float32, device=dev)[:N],
                           centroids=cen[:k], counts=t.zeros(max(k, 1), dtype=t.int32, device=dev)[:k],
                           sums=t.zeros((max(k, 1), d), dtype=t.float64, device=dev)[:k], info=t.zeros(4, dtype=t.int64, device=dev),
                           objective=t.zeros(1, dtype=t.float64, device=dev))
        st = _KmeansState()
        for f in ("centroids", "sums", "counts", "labels", "sim", "info", "objective"):
            setattr(st, f, int(getattr(res, f).data_ptr()))
        self._check(self.lib.mme_kmeans(self.h, e.data_ptr(), N, d, k, None if rows is None else rows.ctypes.data, int(max_iter), C.byref(st),
                                        self._stream()), "mme_kmeans")
        return res

    KMEANS_OPS = {"argmax": 0, "assign": 1, "update": 2}

    def kmeans_apply(self, op, *, qsim=None, ld=None, emb=None, centroids=None, N=None, d=None, k=None, chunk_rows: int = 0, labels=None, sim=None,
                     moved=None, run_if=None, sums=None, counts=None):
        """ONE step of K15 on the caller's CUDA tensors (mme_kmeans_apply; synchronous, works on a bare context).  op: a name
        of KMEANS_OPS or its code; which tensors each op reads and writes is in include/mme.h.  `ld` defaults to qsim's row
        pitch, N to the rows of qsim / emb, d to emb's width and k to the rows of centroids.  The library validates."""
        a = _KmeansApplyArgs()
        a.qsim, a.emb, a.centroids, a.labels, a.sim = (self._ptr(x) for x in (qsim, emb, centroids, labels, sim))
        a.moved, a.run_if, a.sums, a.counts = (self._ptr(x) for x in (moved, run_if, sums, counts))
        a.ld = int((qsim.stride(0) if qsim is not None else 0) if ld is None else ld)
        src = qsim if qsim is not None else emb
        a.N = int((src.shape[0] if src is not None else 0) if N is None else N)
        a.d = int((emb.shape[1] if emb is not None else 0) if d is None else d)
        a.k = int((centroids.shape[0] if centroids is not None else 0) if k is None else k)
        a.chunk_rows = int(chunk_rows)
        self._check(self.lib.mme_kmeans_apply(self.h, int(self.KMEANS_OPS.get(op, op)), C.byref(a), self._stream()), "mme_kmeans_apply")

    # ---- K16 silhouette of a partition (mme.h, mme_silhouette) ----
    def silhouette(self, emb_bf16, labels, k, samples=False):
        """The silhouette of the partition `labels` (int32 [N]; a label outside 0..k-1 belongs to no cluster) of the bf16 rows
        emb_bf16[N, d] under the distance 1 - x_i . x_j (mme_silhouette; enqueues and returns).  -> SilhouetteResult of CUDA
        tensors, `samples` only when asked for.  The library validates N, d and k."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != dev:
            raise MmeError("silhouette: emb must be a 2-D bfloat16 tensor on this engine's device")
        N, d = e.shape
        k = int(k)
        if not hasattr(labels, "dtype") or labels.dtype != t.int32 or labels.dim() != 1 or labels.shape[0] != N or labels.device != dev:
            raise MmeError(f"silhouette: labels must be an int32 tensor [N = {N}] on this engine's device")
        lab = labels.contiguous()
        kk = max(k, 1)
        res = SilhouetteResult(score=t.zeros(1, dtype=t.float64, device=dev), cluster=t.zeros(kk, dtype=t.float64, device=dev)[:k],
                               info=t.zeros(2, dtype=t.int64, device=dev), sums=t.zeros((kk, d), dtype=t.float64, device=dev)[:k],
                               counts=t.zeros(kk, dtype=t.int32, device=dev)[:k],
                               samples=t.zeros(max(N, 1), dtype=t.float64, device=dev)[:N] if samples else None)
        out = _SilhouetteOut()
        for f, v in (("sample", res.samples), ("cluster", res.cluster), ("score", res.score), ("info", res.info), ("sums", res.sums), ("counts", res.counts)):
            setattr(out, f, None if v is None else int(v.data_ptr()))
        self._check(self.lib.mme_silhouette(self.h, e.data_ptr(), N, d, lab.data_ptr(), k, C.byref(out), self._stream()), "mme_silhouette")
        return res

    def silhouette_rows(self, emb_bf16, labels, sums, counts, sample):
        """The rows kernel of K16 alone on the caller's CUDA tensors (mme_silhouette_rows; enqueues): sample float64 [N] from
        sums float64 [k, d] and counts int32 [k].  The library validates."""
        N, d = emb_bf16.shape
        self._check(self.lib.mme_silhouette_rows(self.h, self._ptr(emb_bf16), int(N), int(d), self._ptr(labels), int(counts.shape[0]), self._ptr(sums),
                                                 self._ptr(counts), self._ptr(sample), self._stream()), "mme_silhouette_rows")

    # ---- K17 moments and projection of the vector table (mme.h, mme_moments / mme_project) ----
    MOMENTS_BLOCK = 1024  # MME_MOMENTS_BLOCK

    def moments(self, emb_bf16, group_blocks=None):
        """(sum float64 [d], gram float64 [d, d]) of the bf16 rows emb_bf16[N, d], CUDA tensors, in the fixed order of mme.h
        (mme_moments; enqueues and returns).  `group_blocks` (diagnostic, mme_moments_apply; synchronous): that many row
        blocks per workspace group.  The library validates N and d."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != dev:
            raise MmeError("moments: emb must be a 2-D bfloat16 tensor on this engine's device")
        N, d = e.shape
        s = t.empty(max(d, 1), dtype=t.float64, device=dev)[:d]
        g = t.empty((max(d, 1), max(d, 1)), dtype=t.float64, device=dev)[:d, :d]
        if group_blocks is None:
            self._check(self.lib.mme_moments(self.h, e.data_ptr(), N, d, s.data_ptr(), g.data_ptr(), self._stream()), "mme_moments")
        else:
            self._check(self.lib.mme_moments_apply(self.h, e.data_ptr(), N, d, int(group_blocks), s.data_ptr(), g.data_ptr(), self._stream()),
                        "mme_moments_apply")
        return s, g

    def _f32_table(self, x, what):
        """A float32 CUDA tensor of a mean / component table: a tensor on the device as it is (float32 required), anything else
        (numpy, lists; float64 is rounded once) uploaded on the current stream."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        if t.is_tensor(x) and x.device == dev:
            if x.dtype != t.float32:
                raise MmeError(f"project: {what} on the device must be float32, got {x.dtype}")
            return x.contiguous()
        host = t.from_numpy(np.ascontiguousarray(np.asarray(x.cpu() if t.is_tensor(x) else x, dtype=np.float64).astype(np.float32)))
        return host.to(dev)

    def project(self, emb_bf16, mean, components, *, normalise=True, f32=False, out_f32=None):
        """The rows emb_bf16[N, d] centred by `mean` [d] and projected onto the rows of `components` [m, d] in f32 (mme_project;
        enqueues and returns).  normalise=True: the L2-normalised bf16 rows [N, m] (m % 64 == 0); f32=True, or normalise=False:
        the f32 coordinates [N, m]; both: the pair (bf16, f32).  `out_f32`: a float32 CUDA tensor [N, m] whose row pitch may
        exceed m (a multiple of 4; the columns behind m are not written).  The library validates the shapes."""
        t = self.torch
        dev = t.device(f"cuda:{self.device}")
        e = emb_bf16.contiguous()
        if e.dtype != t.bfloat16 or e.dim() != 2 or e.device != dev:
            raise MmeError("project: emb must be a 2-D bfloat16 tensor on this engine's device")
        N, d = e.shape
        mu, w = self._f32_table(mean, "mean").reshape(-1), self._f32_table(components, "components")
        if w.dim() != 2 or w.shape[1] != d or mu.shape[0] != d:
            raise MmeError(f"project: mean must be [d = {d}] and components [m, d = {d}], got {tuple(mu.shape)} and {tuple(w.shape)}")
        m = w.shape[0]
        want_f32 = bool(f32) or not normalise or out_f32 is not None
        y32 = None
        if want_f32:
            y32 = out_f32 if out_f32 is not None else t.empty((max(N, 1), (m + 3) // 4 * 4), dtype=t.float32, device=dev)[:N, :m]
            if y32.dtype != t.float32 or y32.dim() != 2 or tuple(y32.shape) != (N, m) or y32.stride(1) != 1 or y32.device != dev:
                raise MmeError(f"project: out_f32 must be a float32 tensor [N = {N}, m = {m}] with unit column stride on this engine's device")
        y16 = t.empty((max(N, 1), m), dtype=t.bfloat16, device=dev)[:N] if normalise else None
        self._check(self.lib.mme_project(self.h, e.data_ptr(), N, d, mu.data_ptr(), w.data_ptr(), m, self._ptr(y32),
                                         int(y32.stride(0)) if y32 is not None else 0, self._ptr(y16), self._stream()), "mme_project")
        if normalise and want_f32:
            return y16, y32
        return y16 if normalise else y32

    def gemm_bench(self, M, N, K, epilogue=0, variant=0, iters=10):
        """(avg ms, TFLOP/s) for one GEMM shape on random data."""
        ms = C.c_double(0)
        self._check(self.lib.mme_gemm_bench(self.h, M, N, K, epilogue, variant, iters, C.byref(ms)), "mme_gemm_bench")
        return ms.value, 2.0 * M * N * K / (ms.value * 1e-3) / 1e12

    def gemm_stamps(self, M, N, K):
        """uint64[256, 2, 16] in-kernel cycle stamps of the stamped GEMM build (see mme.h)."""
        st = np.zeros((256, 2, 16), dtype=np.uint64)
        self._check(self.lib.mme_gemm_stamps(self.h, M, N, K, st.ctypes.data), "mme_gemm_stamps")
        return st

    # ---- the one collective, without torch.distributed (mme.h: mme_comm_*, mme_allgather) ---------------
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        self._check(self.lib.mme_comm_unique_id(self.h, buf), "mme_comm_unique_id")
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        comm = C.c_void_p()
        self._check(self.lib.mme_comm_init(self.h, buf, int(rank), int(world), C.byref(comm)), "mme_comm_init")
        return comm

    def comm_destroy(self, comm):
        self._check(self.lib.mme_comm_destroy(self.h, comm), "mme_comm_destroy")

    def allgather(self, comm, shard, world: int, out=None):
        """shard: bf16 CUDA tensor [rows, d] (same rows on every rank) -> [world * rows, d] on every rank."""
        t = self.torch
        assert shard.dtype == t.bfloat16 and shard.is_contiguous()
        rows, d = shard.shape
        if out is None:
            out = t.empty((world * rows, d), dtype=t.bfloat16, device=shard.device)
        self._check(self.lib.mme_allgather(self.h, comm, shard.data_ptr(), rows, d, out.data_ptr(), self._stream()), "mme_allgather")
        return out

    def attention_stamps(self, B, iters=5):
        """(avg ms of the product kernel, uint64[B, 8, 8] cycle stamps of the stamped build; see mme.h)."""
        st = np.zeros((B, 8, 8), dtype=np.uint64)
        ms = C.c_double(0)
        self._check(self.lib.mme_attention_stamps(self.h, int(B), int(iters), C.byref(ms), st.ctypes.data), "mme_attention_stamps")
        return ms.value, st

    # ---- timing ------------------------------------------------------------------------------------
    def profile(self, on: bool):
        self._check(self.lib.mme_profile_enable(self.h, int(on)), "mme_profile_enable")
        self._check(self.lib.mme_profile_reset(self.h), "mme_profile_reset")

    def profile_read(self):
        ms = (C.c_double * NUM_KERNEL_CLASSES)()
        cnt = (C.c_int64 * NUM_KERNEL_CLASSES)()
        rc = self.lib.mme_profile_read_sync(self.h, NUM_KERNEL_CLASSES, ms, cnt)
        self._check(min(rc, 0), "mme_profile_read_sync")
        return {KERNEL_CLASSES[i]: (ms[i], cnt[i]) for i in range(NUM_KERNEL_CLASSES)}
