"""ctypes binding of libvstar_hip.so (the C-ABI declared in include/vstar_hip.h).

There is deliberately no CPU / PyTorch fallback: if the HIP library is missing or no GPU is visible, every compute
entry point raises.  Build with `python -c "import __graft_entry__ as g; g.build()"` or `vstar_amd/csrc/build.sh`.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint, c_uint16, c_void_p

from .config import CVqaConfig, CVstarConfig, MASK_RES, MAX_VERIFY, N_BOXES

LIB_PATH = os.environ.get("VSTAR_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libvstar_hip.so")   # VSTAR_LIB: A/B builds

# every symbol include/vstar_hip.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "vstar_create", "vstar_destroy", "vstar_last_error", "vstar_load_tensor", "vstar_finalize_weights",
    "vstar_vsm_score_batch", "vstar_upsample_mask", "vstar_debug_read", "vstar_stream", "vstar_profile_enable",
    "vstar_profile_read", "vstar_profile_read_fp8", "vstar_op_gemm", "vstar_op_layernorm", "vstar_op_rmsnorm", "vstar_op_attention",
    "vstar_op_attention_workspace", "vstar_image_set", "vstar_preprocess_crops", "vstar_heatmap_stats", "vstar_heatmap_stats_batch", "vstar_vsm_generate", "vstar_op_gemm_fp8",
    "vstar_op_gemm_last_tile", "vstar_op_gemm_last_mode", "vstar_op_gemm_plan", "vstar_op_gemm_norm", "vstar_op_rms_rstd", "vstar_op_ln_fold", "vstar_upsample_mask_ex", "vstar_vsm_score_grouped",
    "vstar_image_set_slot", "vstar_image_set_slot_async", "vstar_preprocess_crops_slots", "vstar_comm_unique_id", "vstar_comm_init", "vstar_allgather_results",
    "vstar_comm_destroy", "vstar_build_source_hash", "vstar_op_mx_scale_bytes", "vstar_op_mx_scale_offset", "vstar_op_quantize_mx",
    "vstar_op_gemm_mx", "vstar_op_gemm_fp8_mxout", "vstar_op_attention_mx", "vstar_w8a8_mx_active", "vstar_w8a8_vit_active",
    "vstar_op_layernorm_quant_fp8",
    # doors of the small kernels (tests/test_small_ops_gpu.py)
    "vstar_op_owl_class_logits", "vstar_op_owl_box_finish", "vstar_op_upsample2x_im2col3x3", "vstar_op_hyper_mask",
    "vstar_op_im2col_patch", "vstar_op_vit_assemble_tokens", "vstar_op_llm_embed_text", "vstar_op_add_bcast",
    "vstar_op_add_bcast_repeat", "vstar_op_bcast_rows", "vstar_op_owl_cls_mul", "vstar_op_gather_rows", "vstar_op_argmax_rows",
    "vstar_op_layernorm_ex", "vstar_op_rmsnorm_ex", "vstar_op_ln_rstd", "vstar_op_scale_cols", "vstar_op_fill",
    "vstar_op_quantize_rows_fp8", "vstar_op_rmsnorm_quant_fp8", "vstar_op_small_attention",
    # doors of the prefill-side GEMM / attention features (tests/test_prefill_ops_gpu.py)
    "vstar_op_gemm_ex", "vstar_op_rope", "vstar_op_attention_grouped", "vstar_op_attention_mx_grouped",
    # the batched contextual-cue decode
    "vstar_vsm_generate_batch",
    # doors of the bf16 decode kernels (tests/test_bf16_decode_gpu.py)
    "vstar_op_rope_kv_append", "vstar_op_cached_attention", "vstar_op_embed_rows", "vstar_op_argmax_rows_lp", "vstar_op_gemm_skinny",
]

# every symbol include/vstar_vqa.h declares
EXPORTS_VQA = [
    "vstar_vqa_create", "vstar_vqa_destroy", "vstar_vqa_last_error", "vstar_vqa_load_tensor", "vstar_vqa_finalize_weights",
    "vstar_vqa_encode_images", "vstar_vqa_forward", "vstar_vqa_debug_read", "vstar_vqa_last_forward_ms", "vstar_vqa_op_gemm",
    "vstar_vqa_forward_sample", "vstar_vqa_op_sample", "vstar_vqa_forward_beam", "vstar_vqa_kv_reorder", "vstar_vqa_kv_copy",
    "vstar_vqa_op_beam_select", "vstar_vqa_forward_score", "vstar_vqa_op_score",
    "vstar_vqa_decode_weight_bits", "vstar_vqa_op_quantize_w8", "vstar_vqa_op_gemm_w8",
    "vstar_vqa_op_quantize_w4", "vstar_vqa_op_gemm_w4",
    "vstar_vqa_kv_cache_format", "vstar_vqa_kv_cache_bytes", "vstar_vqa_op_kv_quantize",
    "vstar_vqa_forward_verify", "vstar_vqa_op_verify",
    "vstar_vqa_forward_edits", "vstar_vqa_forward_sample_edits", "vstar_vqa_forward_verify_edits", "vstar_vqa_op_edit",
    "vstar_vqa_logit_edit_capacity",
    "vstar_vqa_forward_logprobs", "vstar_vqa_forward_sample_logprobs", "vstar_vqa_forward_verify_logprobs", "vstar_vqa_op_logprobs",
    "vstar_vqa_forward_sample_warp", "vstar_vqa_forward_verify_warp", "vstar_vqa_op_sample_warp", "vstar_vqa_op_verify_warp",
    # doors of the decode-side kernels (tests/test_decode_ops_gpu.py)
    "vstar_vqa_op_rope_kv_append", "vstar_vqa_op_cached_attention", "vstar_vqa_op_perceiver_attention", "vstar_vqa_op_embed_rows",
    "vstar_vqa_op_argmax_rows",
    # doors of the fp16 prefill kernels (tests/test_f16_prefill_gpu.py)
    "vstar_vqa_op_attention", "vstar_vqa_op_layernorm", "vstar_vqa_op_rmsnorm", "vstar_vqa_op_add_bcast",
    "vstar_vqa_op_vit_assemble_tokens",
    # contrastive search
    "vstar_vqa_forward_contrast_begin", "vstar_vqa_forward_contrast_step", "vstar_vqa_op_contrast",
    # guided decoding against a negative sequence
    "vstar_vqa_forward_guided", "vstar_vqa_forward_sample_guided", "vstar_vqa_guide_rows",
]

F32, F16, BF16 = 0, 1, 2
MAX_IMAGE_SLOTS = 64
EPI_NONE, EPI_QUICK_GELU, EPI_GELU, EPI_RELU, EPI_SILU_MUL = range(5)
EPI_NOSYNC, EPI_TILE128, EPI_TILE256, EPI_TILE4W = 0x100, 0x200, 0x400, 0x800
EPI_VARIANT_MASK = 0x7000


def EPI_VARIANT(v: int) -> int:
    """VSTAR_EPI_VARIANT(v): variant v (2, 5, 6 or 7) of the 128-row GEMM family for this call, OR-ed into `epilogue`."""
    return v << 12


TILE_4W = 2564          # vstar_op_gemm_last_tile() value of the 4-wave / AGPR 256 x 256 kernel
GEN_MAX_BATCH = 16      # VSTAR_GEN_MAX_BATCH
F_SKIP_OWL, F_DEVICE_INPUTS, F_DEVICE_OUTPUT, F_NO_SYNC, F_INTERNAL_PIXELS, F_SHARE_PREFIX = 1, 2, 4, 8, 16, 32


class VstarResult(ctypes.Structure):
    _fields_ = [
        ("pred_logits", c_float * N_BOXES),
        ("pred_boxes", c_float * (N_BOXES * 4)),
        ("lowres_mask", c_float * (MASK_RES * MASK_RES)),
        ("tf_argmax", c_int32 * MAX_VERIFY),
    ]


RESULT_FLOATS = ctypes.sizeof(VstarResult) // 4


class VqaSampling(ctypes.Structure):
    """vstar_vqa_sampling (include/vstar_vqa.h): one row's sampling parameters and Philox coordinates, 32 bytes."""
    _fields_ = [
        ("temperature", c_float),
        ("top_k", c_int32),
        ("top_p", c_float),
        ("step", ctypes.c_uint32),
        ("seed", ctypes.c_uint64),
        ("stream", ctypes.c_uint64),
    ]


class VqaWarpers(ctypes.Structure):
    """vstar_vqa_warpers (include/vstar_vqa.h): one row's min-p / typical-p / epsilon / eta values, 16 bytes."""
    _fields_ = [
        ("min_p", c_float),             # [0, 1]; 0 = off
        ("typical_p", c_float),         # > 0; >= 1 = off
        ("epsilon_cutoff", c_float),    # [0, 1); 0 = off
        ("eta_cutoff", c_float),        # [0, 1); 0 = off
    ]


class VqaLogitEdits(ctypes.Structure):
    """vstar_vqa_logit_edits (include/vstar_vqa.h): the host CSR arrays of one call's logits edits, three pointers."""
    _fields_ = [
        ("off", c_void_p),
        ("tok", c_void_p),
        ("penalty", c_void_p),
    ]


MAX_TOP_LOGPROBS = 32       # VSTAR_VQA_MAX_TOP_LOGPROBS


class VqaLogprobs(ctypes.Structure):
    """vstar_vqa_logprobs (include/vstar_vqa.h): n_top and the four host output arrays of one call's log-probabilities."""
    _fields_ = [
        ("n_top", c_int32),
        ("token_logprob", c_void_p),
        ("token_rank", c_void_p),
        ("top_logprob", c_void_p),
        ("top_token", c_void_p),
    ]


class VqaGuidance(ctypes.Structure):
    """vstar_vqa_guidance (include/vstar_vqa.h): n_out and the three host arrays of one call's guidance."""
    _fields_ = [
        ("n_out", c_int32),
        ("neg", c_void_p),
        ("scale", c_void_p),
        ("log_beta", c_void_p),
    ]


class VqaKvView(ctypes.Structure):
    """vstar_vqa_kv_view (include/vstar_vqa.h): one layer of a KV cache for the decode-side op doors."""
    _fields_ = [
        ("fmt", c_int32), ("heads", c_int32), ("ctx", c_int32), ("slots", c_int32),
        ("dev_k", c_void_p), ("dev_v", c_void_p), ("dev_ks", c_void_p), ("dev_vs", c_void_p),
    ]


class VqaKvRows(ctypes.Structure):
    """vstar_vqa_kv_rows (include/vstar_vqa.h): the HOST index arrays of one call of the decode-side op doors."""
    _fields_ = [
        ("R", c_int32), ("n_seq", c_int32),
        ("row_seq", c_void_p), ("row_pos", c_void_p), ("row_slot", c_void_p),
        ("seq_kv", c_void_p), ("seq_prefix", c_void_p), ("seq_past", c_void_p), ("anc", c_void_p),
    ]


class GemmEx(ctypes.Structure):
    """vstar_gemm_ex (include/vstar_hip.h): one call of vstar_op_gemm_ex, every buffer with its extent in rows."""
    _fields_ = [
        ("A", c_void_p), ("lda", c_int64), ("a_rows", c_int64), ("a_group", c_int32), ("a_gstride", c_int64), ("a_off", c_int64),
        ("W", c_void_p), ("w_rows", c_int64),
        ("bias", c_void_p),
        ("residual", c_void_p), ("ldr", c_int64),
        ("C", c_void_p), ("ldc", c_int64), ("c_rows", c_int64), ("c_group", c_int32), ("c_gstride", c_int64), ("c_off", c_int64),
        ("M", c_int32), ("N", c_int32), ("K", c_int32), ("epilogue", c_int32),
        ("row_scale", c_void_p), ("sumsq_out", c_void_p), ("sumsq_ld", c_int32), ("stats_sum", c_int32),
        ("rope_cs", c_void_p), ("rope_rows", c_int32), ("rope_S", c_int32), ("rope_cols", c_int32), ("rope_R0", c_int32),
        ("rope_Lc", c_int32), ("rope_pos0", c_int32), ("rope_tail", c_int32),
    ]


class VstarError(RuntimeError):
    pass


_lib = None


def load() -> ctypes.CDLL:
    """Loads the shared library and declares the prototypes.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VstarError(f"{LIB_PATH} not built — run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                         "there is no CPU fallback for the HIP engine")
    # torch first: the process must end up with ONE HIP runtime (torch bundles its own libamdhip64; loading ours against
    # /opt/rocm before torch leaves the engine on a runtime that sees no device once torch is imported)
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    H = c_void_p
    lib.vstar_create.argtypes = [POINTER(CVstarConfig), c_int, POINTER(H)]
    lib.vstar_create.restype = c_int
    lib.vstar_destroy.argtypes = [H]
    lib.vstar_destroy.restype = None
    lib.vstar_last_error.argtypes = [H]
    lib.vstar_last_error.restype = c_char_p
    lib.vstar_build_source_hash.argtypes = []
    lib.vstar_build_source_hash.restype = c_char_p
    lib.vstar_load_tensor.argtypes = [H, c_char_p, c_void_p, c_int, c_int, POINTER(c_int64)]
    lib.vstar_load_tensor.restype = c_int
    lib.vstar_finalize_weights.argtypes = [H]
    lib.vstar_finalize_weights.restype = c_int
    lib.vstar_vsm_score_batch.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_uint,
                                          c_void_p]
    lib.vstar_vsm_score_batch.restype = c_int
    lib.vstar_vsm_score_grouped.argtypes = [H, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                            c_uint, c_void_p]
    lib.vstar_vsm_score_grouped.restype = c_int
    lib.vstar_vsm_generate.argtypes = [H, c_void_p, c_void_p, c_int, c_int, c_int, c_uint, c_void_p, c_void_p]
    lib.vstar_vsm_generate.restype = c_int
    lib.vstar_vsm_generate_batch.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_uint, c_void_p, c_void_p]
    lib.vstar_vsm_generate_batch.restype = c_int
    lib.vstar_image_set.argtypes = [H, c_void_p, c_int, c_int]
    lib.vstar_image_set.restype = c_int
    lib.vstar_preprocess_crops.argtypes = [H, c_int, c_void_p]
    lib.vstar_preprocess_crops.restype = c_int
    lib.vstar_image_set_slot.argtypes = [H, c_int, c_void_p, c_int, c_int]
    lib.vstar_image_set_slot.restype = c_int
    lib.vstar_image_set_slot_async.argtypes = [H, c_int, c_void_p, c_int, c_int]
    lib.vstar_image_set_slot_async.restype = c_int
    lib.vstar_preprocess_crops_slots.argtypes = [H, c_int, c_void_p, c_void_p]
    lib.vstar_preprocess_crops_slots.restype = c_int
    lib.vstar_comm_unique_id.argtypes = [c_void_p]
    lib.vstar_comm_unique_id.restype = c_int
    lib.vstar_comm_init.argtypes = [H, c_void_p, c_int, c_int]
    lib.vstar_comm_init.restype = c_int
    lib.vstar_allgather_results.argtypes = [H, c_void_p, c_int, c_void_p, ctypes.c_uint]
    lib.vstar_allgather_results.restype = c_int
    lib.vstar_comm_destroy.argtypes = [H]
    lib.vstar_comm_destroy.restype = c_int
    lib.vstar_heatmap_stats.argtypes = [H, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.vstar_heatmap_stats.restype = c_int
    lib.vstar_heatmap_stats_batch.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_heatmap_stats_batch.restype = c_int
    lib.vstar_upsample_mask.argtypes = [H, c_void_p, c_int, c_int, c_void_p]
    lib.vstar_upsample_mask.restype = c_int
    lib.vstar_upsample_mask_ex.argtypes = [H, c_void_p, c_int, c_int, c_int, c_void_p]
    lib.vstar_upsample_mask_ex.restype = c_int
    lib.vstar_debug_read.argtypes = [H, c_char_p, c_void_p, c_int64]
    lib.vstar_debug_read.restype = c_int64
    lib.vstar_stream.argtypes = [H]
    lib.vstar_stream.restype = c_void_p
    lib.vstar_profile_enable.argtypes = [H, c_int]
    lib.vstar_profile_enable.restype = c_int
    lib.vstar_profile_read.argtypes = [H, POINTER(c_double), POINTER(c_int64), POINTER(c_double)]
    lib.vstar_profile_read.restype = c_int
    lib.vstar_profile_read_fp8.argtypes = [H, POINTER(c_double), POINTER(c_int64), POINTER(c_double)]
    lib.vstar_profile_read_fp8.restype = c_int
    lib.vstar_op_gemm.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                  c_int, c_int, c_int, c_int, c_int]
    lib.vstar_op_gemm.restype = c_int
    lib.vstar_op_gemm_norm.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                       c_int, c_void_p, c_void_p, c_int]
    lib.vstar_op_gemm_norm.restype = c_int
    lib.vstar_op_rms_rstd.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p]
    lib.vstar_op_rms_rstd.restype = c_int
    lib.vstar_op_ln_fold.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int]
    lib.vstar_op_ln_fold.restype = c_int
    lib.vstar_op_gemm_last_tile.argtypes = []
    lib.vstar_op_gemm_last_tile.restype = c_int
    lib.vstar_op_gemm_last_mode.argtypes = []
    lib.vstar_op_gemm_last_mode.restype = c_int
    lib.vstar_op_gemm_plan.argtypes = [c_int] * 7
    lib.vstar_op_gemm_plan.restype = c_int
    lib.vstar_op_gemm_fp8.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      POINTER(c_float)]
    lib.vstar_op_gemm_fp8.restype = c_int
    lib.vstar_op_mx_scale_bytes.argtypes = [c_int, c_int]
    lib.vstar_op_mx_scale_bytes.restype = c_size_t
    lib.vstar_op_mx_scale_offset.argtypes = [c_int, c_int, c_int]
    lib.vstar_op_mx_scale_offset.restype = ctypes.c_int64
    lib.vstar_op_quantize_mx.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int]
    lib.vstar_op_quantize_mx.restype = c_int
    lib.vstar_op_gemm_mx.argtypes = [c_void_p] * 10 + [c_int, c_int, c_int, c_int, c_int, POINTER(c_float)]
    lib.vstar_op_gemm_mx.restype = c_int
    lib.vstar_op_gemm_fp8_mxout.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_float)]
    lib.vstar_op_gemm_fp8_mxout.restype = c_int
    lib.vstar_op_attention_mx.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int]
    lib.vstar_op_attention_mx.restype = c_int
    lib.vstar_op_gemm_ex.argtypes = [c_void_p, POINTER(GemmEx)]
    lib.vstar_op_gemm_ex.restype = c_int
    lib.vstar_op_rope.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int]
    lib.vstar_op_rope.restype = c_int
    lib.vstar_op_attention_grouped.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int]
    lib.vstar_op_attention_grouped.restype = c_int
    lib.vstar_op_attention_mx_grouped.argtypes = [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int]
    lib.vstar_op_attention_mx_grouped.restype = c_int
    lib.vstar_w8a8_mx_active.argtypes = [c_void_p]
    lib.vstar_w8a8_mx_active.restype = c_int
    lib.vstar_w8a8_vit_active.argtypes = [c_void_p]
    lib.vstar_w8a8_vit_active.restype = c_int
    lib.vstar_op_layernorm.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float]
    lib.vstar_op_layernorm.restype = c_int
    lib.vstar_op_rmsnorm.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float]
    lib.vstar_op_rmsnorm.restype = c_int
    lib.vstar_op_attention.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int,
                                       c_float]
    lib.vstar_op_attention.restype = c_int
    lib.vstar_op_attention_workspace.argtypes = [c_int, c_int, c_int, c_int]
    lib.vstar_op_attention_workspace.restype = c_size_t
    # doors of the small kernels: (stream, ...) -> int
    V, I, L, F = c_void_p, c_int, c_int64, c_float
    for name, args in {
        "owl_class_logits": [V, I, I, V, V, I, I, I, I], "owl_box_finish": [V, I, V, I, I, I, I],
        "upsample2x_im2col3x3": [V, V, I, I, I, I], "hyper_mask": [V, V, V, I, I, I, I],
        "im2col_patch": [V, V, I, I, I, I], "vit_assemble_tokens": [V, V, V, V, I, I, I],
        "llm_embed_text": [V, I, I, I, V, I, V, I, I], "add_bcast": [V, V, V, L, I, L],
        "add_bcast_repeat": [V, V, V, I, I, I, I], "bcast_rows": [V, V, I, L, I, I, L], "owl_cls_mul": [V, V, I, I, I],
        "gather_rows": [V, V, V, I, I], "argmax_rows": [V, I, I, I, V, I],
        "layernorm_ex": [V, V, V, V, I, I, F, V, I], "rmsnorm_ex": [V, V, V, I, I, F, V], "ln_rstd": [V, V, I, I, I, F, V],
        "scale_cols": [V, V, L, I], "fill": [V, L, F], "quantize_rows_fp8": [V, L, V, L, V, I, I],
        "rmsnorm_quant_fp8": [V, V, V, V, I, I, F], "layernorm_quant_fp8": [V, V, V, V, V, I, I, F],
        "small_attention": [V, V, V, V, I, I, I, I, I],
    }.items():
        fn = getattr(lib, "vstar_op_" + name)
        fn.argtypes = [c_void_p] + args
        fn.restype = c_int
    # doors of the bf16 decode kernels: the argument lists of their vstar_vqa_op_* twins
    lib.vstar_op_rope_kv_append.argtypes = [c_void_p, c_void_p, c_int, POINTER(VqaKvView), POINTER(VqaKvRows)]
    lib.vstar_op_rope_kv_append.restype = c_int
    lib.vstar_op_cached_attention.argtypes = [c_void_p, c_void_p, c_int, POINTER(VqaKvView), POINTER(VqaKvRows), c_int, c_int, c_int,
                                              c_void_p, POINTER(c_int)]
    lib.vstar_op_cached_attention.restype = c_int
    lib.vstar_op_embed_rows.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int]
    lib.vstar_op_embed_rows.restype = c_int
    lib.vstar_op_argmax_rows_lp.argtypes = [c_void_p, c_int, c_int, c_int64, c_void_p]
    lib.vstar_op_argmax_rows_lp.restype = c_int
    lib.vstar_op_gemm_skinny.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_float, c_int, POINTER(c_int)]
    lib.vstar_op_gemm_skinny.restype = c_int
    # ---- VQA-LLM engine (include/vstar_vqa.h) ----
    lib.vstar_vqa_create.argtypes = [POINTER(CVqaConfig), c_int, POINTER(H)]
    lib.vstar_vqa_create.restype = c_int
    lib.vstar_vqa_destroy.argtypes = [H]
    lib.vstar_vqa_destroy.restype = None
    lib.vstar_vqa_last_error.argtypes = [H]
    lib.vstar_vqa_last_error.restype = c_char_p
    lib.vstar_vqa_load_tensor.argtypes = [H, c_char_p, c_void_p, c_int, c_int, POINTER(c_int64)]
    lib.vstar_vqa_load_tensor.restype = c_int
    lib.vstar_vqa_finalize_weights.argtypes = [H]
    lib.vstar_vqa_finalize_weights.restype = c_int
    lib.vstar_vqa_encode_images.argtypes = [H, c_int, c_void_p, c_int]
    lib.vstar_vqa_encode_images.restype = c_int
    lib.vstar_vqa_forward.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p]
    lib.vstar_vqa_forward.restype = c_int
    lib.vstar_vqa_forward_sample.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                             c_void_p, c_void_p]
    lib.vstar_vqa_forward_sample.restype = c_int
    lib.vstar_vqa_op_sample.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_sample.restype = c_int
    lib.vstar_vqa_forward_beam.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                           c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_beam.restype = c_int
    lib.vstar_vqa_kv_reorder.argtypes = [H, c_int, c_void_p, c_void_p, c_int, c_int]
    lib.vstar_vqa_kv_reorder.restype = c_int
    lib.vstar_vqa_kv_copy.argtypes = [H, c_int, c_int, c_int, c_int]
    lib.vstar_vqa_kv_copy.restype = c_int
    lib.vstar_vqa_op_beam_select.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                             c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_beam_select.restype = c_int
    lib.vstar_vqa_forward_score.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_score.restype = c_int
    lib.vstar_vqa_op_score.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_score.restype = c_int
    lib.vstar_vqa_forward_verify.argtypes = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                             c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_verify.restype = c_int
    lib.vstar_vqa_op_verify.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                        c_void_p]
    lib.vstar_vqa_op_verify.restype = c_int
    lib.vstar_vqa_forward_edits.argtypes = lib.vstar_vqa_forward.argtypes + [c_void_p]
    lib.vstar_vqa_forward_edits.restype = c_int
    lib.vstar_vqa_forward_sample_edits.argtypes = lib.vstar_vqa_forward_sample.argtypes + [c_void_p]
    lib.vstar_vqa_forward_sample_edits.restype = c_int
    lib.vstar_vqa_forward_verify_edits.argtypes = lib.vstar_vqa_forward_verify.argtypes + [c_void_p]
    lib.vstar_vqa_forward_verify_edits.restype = c_int
    lib.vstar_vqa_op_edit.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_edit.restype = c_int
    lib.vstar_vqa_logit_edit_capacity.argtypes = [H]
    lib.vstar_vqa_logit_edit_capacity.restype = c_int64
    lib.vstar_vqa_forward_logprobs.argtypes = lib.vstar_vqa_forward_edits.argtypes + [c_void_p]
    lib.vstar_vqa_forward_logprobs.restype = c_int
    lib.vstar_vqa_forward_sample_logprobs.argtypes = lib.vstar_vqa_forward_sample_edits.argtypes + [c_void_p]
    lib.vstar_vqa_forward_sample_logprobs.restype = c_int
    lib.vstar_vqa_forward_verify_logprobs.argtypes = lib.vstar_vqa_forward_verify_edits.argtypes + [c_void_p]
    lib.vstar_vqa_forward_verify_logprobs.restype = c_int
    #  params / tokens, then warpers, edits, lp; the verify form: ... tokens_out, then warpers, edits, lp
    lib.vstar_vqa_forward_sample_warp.argtypes = lib.vstar_vqa_forward_sample.argtypes + [c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_sample_warp.restype = c_int
    lib.vstar_vqa_forward_verify_warp.argtypes = lib.vstar_vqa_forward_verify.argtypes + [c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_verify_warp.restype = c_int
    lib.vstar_vqa_op_sample_warp.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p]
    lib.vstar_vqa_op_sample_warp.restype = c_int
    lib.vstar_vqa_op_verify_warp.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p]
    lib.vstar_vqa_op_verify_warp.restype = c_int
    lib.vstar_vqa_op_logprobs.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p]
    lib.vstar_vqa_op_logprobs.restype = c_int
    lib.vstar_vqa_op_gemm.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_float]
    lib.vstar_vqa_op_gemm.restype = c_int
    lib.vstar_vqa_decode_weight_bits.argtypes = [H]
    lib.vstar_vqa_decode_weight_bits.restype = c_int
    lib.vstar_vqa_op_quantize_w8.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_quantize_w8.restype = c_int
    lib.vstar_vqa_op_gemm_w8.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_float, c_int]
    lib.vstar_vqa_op_gemm_w8.restype = c_int
    lib.vstar_vqa_kv_cache_format.argtypes = [H]
    lib.vstar_vqa_kv_cache_format.restype = c_int
    lib.vstar_vqa_kv_cache_bytes.argtypes = [H]
    lib.vstar_vqa_kv_cache_bytes.restype = ctypes.c_int64
    lib.vstar_vqa_op_kv_quantize.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_kv_quantize.restype = c_int
    lib.vstar_vqa_op_quantize_w4.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_quantize_w4.restype = c_int
    lib.vstar_vqa_op_gemm_w4.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_float, c_int]
    lib.vstar_vqa_op_gemm_w4.restype = c_int
    lib.vstar_vqa_op_rope_kv_append.argtypes = [c_void_p, c_void_p, c_int, POINTER(VqaKvView), POINTER(VqaKvRows)]
    lib.vstar_vqa_op_rope_kv_append.restype = c_int
    lib.vstar_vqa_op_cached_attention.argtypes = [c_void_p, c_void_p, c_int, POINTER(VqaKvView), POINTER(VqaKvRows), c_int, c_int, c_int,
                                                  c_void_p, POINTER(c_int)]
    lib.vstar_vqa_op_cached_attention.restype = c_int
    lib.vstar_vqa_op_perceiver_attention.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int]
    lib.vstar_vqa_op_perceiver_attention.restype = c_int
    lib.vstar_vqa_op_embed_rows.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int]
    lib.vstar_vqa_op_embed_rows.restype = c_int
    lib.vstar_vqa_op_argmax_rows.argtypes = [c_void_p, c_int, c_int, c_int64, c_void_p]
    lib.vstar_vqa_op_argmax_rows.restype = c_int
    lib.vstar_vqa_op_attention.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int]
    lib.vstar_vqa_op_attention.restype = c_int
    lib.vstar_vqa_op_layernorm.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_int]
    lib.vstar_vqa_op_layernorm.restype = c_int
    lib.vstar_vqa_op_rmsnorm.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p]
    lib.vstar_vqa_op_rmsnorm.restype = c_int
    lib.vstar_vqa_op_add_bcast.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64]
    lib.vstar_vqa_op_add_bcast.restype = c_int
    lib.vstar_vqa_op_vit_assemble_tokens.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int]
    lib.vstar_vqa_op_vit_assemble_tokens.restype = c_int
    _rows8 = [H, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p]      # the eight row arguments behind the handle
    lib.vstar_vqa_forward_contrast_begin.argtypes = _rows8 + [c_int, c_void_p, c_void_p]
    lib.vstar_vqa_forward_contrast_begin.restype = c_int
    lib.vstar_vqa_forward_contrast_step.argtypes = _rows8 + [c_void_p, c_int, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_contrast_step.restype = c_int
    lib.vstar_vqa_op_contrast.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                          c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_op_contrast.restype = c_int
    #  logits / argmax, then guidance, edits, lp; the sampled form: params / tokens, then warpers, guidance, edits, lp
    lib.vstar_vqa_forward_guided.argtypes = lib.vstar_vqa_forward.argtypes + [c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_guided.restype = c_int
    lib.vstar_vqa_forward_sample_guided.argtypes = lib.vstar_vqa_forward_sample.argtypes + [c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_forward_sample_guided.restype = c_int
    lib.vstar_vqa_guide_rows.argtypes = [c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.vstar_vqa_guide_rows.restype = c_int
    lib.vstar_vqa_debug_read.argtypes = [H, c_char_p, c_void_p, c_int64]
    lib.vstar_vqa_debug_read.restype = c_int64
    lib.vstar_vqa_last_forward_ms.argtypes = [H]
    lib.vstar_vqa_last_forward_ms.restype = c_double
    _lib = lib
    return lib


def check_vqa(rc: int, handle=None) -> None:
    if rc != 0:
        msg = load().vstar_vqa_last_error(handle)
        raise VstarError(f"libvstar_hip (vqa) error {rc}: {msg.decode() if msg else '?'}")


def check(rc: int, handle=None) -> None:
    if rc != 0:
        msg = load().vstar_last_error(handle)
        raise VstarError(f"libvstar_hip error {rc}: {msg.decode() if msg else '?'}")
