#!/usr/bin/env python3
"""Records tests/golden/op_door_refusals.json: the calls below, each refused on the host by an op-level door, with the return code and
message of the library that VSTAR_LIB names (default: the in-tree build).  The fixture pins behaviour ACROSS a change, so record it
from the build of the commit BEFORE the change:

    VSTAR_LIB=/path/to/parent/libvstar_hip.so python3 tools/record_op_door_refusals.py

The encoding of the arguments is documented in tests/test_op_door_refusals.py, which replays the records.  Every call here must be
refused with VSTAR_ERR_INVALID before any HIP call (the recorder needs no GPU and refuses to write anything else)."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests.test_op_door_refusals import ERR_INVALID, FIXTURE, replay      # noqa: E402
from vstar_amd import _lib      # noqa: E402

P = 0x10000      # a dummy device pointer (non-null, 16-byte aligned): refused calls dereference host arrays only
F16 = _lib.F16
T128, T256, T4W = _lib.EPI_TILE128, _lib.EPI_TILE256, _lib.EPI_TILE4W
SILU = _lib.EPI_SILU_MUL


def i32(*v):
    return {"i32": list(v)}


def f32(*v):
    return {"f32": list(v)}


OUT = {"out": "int"}
CASES = []


def case(door, *args):
    CASES.append((door, list(args)))


# ---- vstar_op_gemm / _gemm_norm: (stream, A, lda, W, bias, res, ldr, C, ldc, [out_f32,] M, N, K, epilogue, ...) ----
def gemm(epi, M=64, N=64, K=64):
    return [None, P, K, P, None, None, 0, P, N, 0, M, N, K, epi]


def gemm_norm(epi, M=64, N=64, K=64, sumsq=None):
    return [None, P, K, P, None, None, 0, P, N, M, N, K, epi, None, sumsq, N // 64]


case("vstar_op_gemm", *gemm(T128 | T256))
case("vstar_op_gemm", *gemm(_lib.EPI_VARIANT(3)))
case("vstar_op_gemm", *gemm(_lib.EPI_VARIANT(2) | T256))
case("vstar_op_gemm", *gemm(T256))
case("vstar_op_gemm_norm", *gemm_norm(T128 | T256, N=100, sumsq=P))      # the tile overrides come before the door's own rule
case("vstar_op_gemm_norm", *gemm_norm(_lib.EPI_VARIANT(3), N=100, sumsq=P))      # ... and that one before the kernel requests
case("vstar_op_gemm_norm", *gemm_norm(_lib.EPI_GELU, sumsq=P))
case("vstar_op_gemm_norm", *gemm_norm(_lib.EPI_VARIANT(3)))
case("vstar_op_gemm_norm", *gemm_norm(T256))
case("vstar_op_gemm_plan", 0, 64, 64, 0, 0, 0, 256)
case("vstar_op_gemm_plan", 64, 64, 64, _lib.EPI_VARIANT(3), 0, 0, 256)
case("vstar_op_gemm_plan", 2048, 3072, 1024, _lib.EPI_VARIANT(2), 0, 1, 256)
# ---- the W8A8 bench doors, the attention workspace, the LayerNorm statistics ----
case("vstar_op_gemm_fp8", None, None, P, None, None, P, 1024, 256, 256, 0, 0, None)
case("vstar_op_gemm_fp8", None, P, P, None, None, P, 1024, 0, 256, 0, 0, None)
case("vstar_op_gemm_mx", None, P, None, None, P, None, P, None, None, None, 1024, 256, 256, 0, 0, None)
case("vstar_op_gemm_mx", None, P, P, None, P, None, None, None, None, None, 1024, 256, 256, 0, 0, None)
case("vstar_op_gemm_fp8_mxout", None, P, P, P, None, 1024, 256, 256, 0, None)
case("vstar_op_attention", None, P, P, P, 0, 1, 128, 2, 128, 1, 0.0)
case("vstar_op_ln_rstd", None, None, None, 4, 8, 64, 1e-5, P)


# ---- vstar_op_gemm_ex ----
def gemm_ex(**kw):
    f = dict(A=P, lda=64, a_rows=64, W=P, w_rows=256, C=P, ldc=64, c_rows=64, M=64, N=64, K=64, epilogue=0)
    f.update(kw)
    return [None, {"struct": "GemmEx", "fields": f}]


ROPE_SHAPE = dict(M=1024, N=256, K=128, lda=128, ldc=256, a_rows=1024, c_rows=1024, rope_cs=P, rope_S=1024, rope_cols=256)
case("vstar_op_gemm_ex", None, None)
case("vstar_op_gemm_ex", *gemm_ex(A=None))
case("vstar_op_gemm_ex", *gemm_ex(K=96))
case("vstar_op_gemm_ex", *gemm_ex(epilogue=_lib.EPI_NOSYNC))
case("vstar_op_gemm_ex", *gemm_ex(epilogue=T128 | T256))
case("vstar_op_gemm_ex", *gemm_ex(epilogue=_lib.EPI_VARIANT(3)))
case("vstar_op_gemm_ex", *gemm_ex(a_rows=10))
case("vstar_op_gemm_ex", *gemm_ex(c_rows=10))
case("vstar_op_gemm_ex", *gemm_ex(stats_sum=4))
case("vstar_op_gemm_ex", *gemm_ex(rope_S=64))
case("vstar_op_gemm_ex", *gemm_ex(rope_rows=100, **ROPE_SHAPE))
case("vstar_op_gemm_ex", *gemm_ex(epilogue=T256))
case("vstar_op_gemm_ex", *gemm_ex(epilogue=T4W))
# ---- vstar_op_rope (stream, qkv, qkv_rows, cos_sin, table_rows, B, S, H, D, R0, Lc), the grouped attention doors ----
case("vstar_op_rope", None, None, 64, P, 64, 1, 64, 2, 128, 0, 0)
case("vstar_op_rope", None, P, 64, P, 64, 1, 64, 2, 96, 0, 0)
case("vstar_op_rope", None, P, 64, P, 64, 1, 64, 2, 128, 0, 5)
case("vstar_op_rope", None, P, 63, P, 64, 1, 64, 2, 128, 0, 0)
case("vstar_op_rope", None, P, 64, P, 10, 1, 64, 2, 128, 0, 0)
case("vstar_op_attention_grouped", None, None, 256, P, 256, 1, 256, 2, 0, 0)
case("vstar_op_attention_grouped", None, P, 256, P, 256, 1, 256, 2, 64, 32)
case("vstar_op_attention_grouped", None, P, 256, P, 256, 1, 256, 2, 128, 32 + 128)
case("vstar_op_attention_grouped", None, P, 256, P, 255, 1, 256, 2, 128, 32)
case("vstar_op_attention_mx_grouped", None, P, 256, None, 256, P, 1, 256, 2, 0, 0)
case("vstar_op_attention_mx_grouped", None, P, 200, P, 200, P, 1, 200, 2, 0, 0)
case("vstar_op_attention_mx_grouped", None, P, 256, P, 256, P, 1, 256, 2, 0, 7)
case("vstar_op_attention_mx_grouped", None, P, 255, P, 256, P, 1, 256, 2, 128, 32)


# ---- the decode-side doors, through both of their names (op_doors.hpp: kv_op_check and the door bodies) ----
def kv_view(**kw):
    f = dict(fmt=0, heads=2, ctx=16, slots=2, dev_k=P, dev_v=P)
    f.update(kw)
    return {"struct": "VqaKvView", "fields": f}


def kv_rows(**kw):
    f = dict(R=2, n_seq=2, row_seq=i32(0, 1), row_pos=i32(3, 4), row_slot=i32(0, 1), seq_kv=i32(0, 1), seq_prefix=i32(0, 1),
             seq_past=i32(0, 0))
    f.update(kw)
    return {"struct": "VqaKvRows", "fields": f}


for half in ("vstar_op_", "vstar_vqa_op_"):
    append, attend = half + "rope_kv_append", half + "cached_attention"
    case(append, None, P, 16, kv_view(), kv_rows())
    case(append, P, P, 16, None, kv_rows())
    case(append, P, P, 16, kv_view(fmt=3), kv_rows())
    case(append, P, P, 16, kv_view(fmt=1), kv_rows())
    case(append, P, P, 16, kv_view(), kv_rows(row_pos=i32(3, 16)))
    case(append, P, P, 16, kv_view(), kv_rows(seq_past=i32(4, 0)))
    case(append, P, P, 16, kv_view(), kv_rows(anc=i32(*([0] * 31 + [5]))))      # the last rule of the append door
    case(attend, None, P, 16, kv_view(), kv_rows(), 8, 0, 1, P, OUT)
    case(attend, P, P, 16, kv_view(), kv_rows(), 8, -1, 1, P, OUT)
    case(attend, P, None, 16, kv_view(), kv_rows(), 8, 1, 1, P, OUT)
    case(attend, P, P, 16, kv_view(), kv_rows(), 8, 0, 17, P, OUT)
    case(attend, P, P, 16, kv_view(), None, 8, 0, 1, P, OUT)
    case(attend, P, P, 16, kv_view(), kv_rows(), 8, 3, 1, P, OUT)
    case(attend, P, P, 16, kv_view(), kv_rows(), 4, 0, 1, P, OUT)
    case(attend, P, P, 16, kv_view(), kv_rows(row_slot=i32(1, 1)), 8, 1, 1, P, OUT)
    case(attend, P, P, 10240, kv_view(ctx=10240), kv_rows(), 10240, 0, 1, P, OUT)
    case(attend, P, P, 256, kv_view(heads=128, ctx=256), kv_rows(), 256, 2, 1, P, OUT)      # the last rule of the chain
    case(half + "embed_rows", None, 2, P, 32, None, 0, P, 64)
    case(half + "embed_rows", i32(0, 1), 2, P, 32, None, 0, P, 60)
case("vstar_op_rope_kv_append", P, P, 16, kv_view(fmt=1, dev_ks=P, dev_vs=P), kv_rows())      # kv_format_ok: the bf16 half has format 0 only
case("vstar_op_argmax_rows_lp", P, 2, 32, 16, P)
case("vstar_vqa_op_argmax_rows", P, 0, 32, 32, P)


# ---- vstar_op_gemm_skinny (A, W, bias, res, C, M, N, K, epilogue, kernel, out_f32, norm_w, norm_eps, layout, kernel_ran) ----
def skinny(A=P, M=4, N=64, K=64, epi=0, kernel=1, out_f32=0, layout=0, ran=OUT):
    return [A, P, None, None, P, M, N, K, epi, kernel, out_f32, None, 0.0, layout, ran]


case("vstar_op_gemm_skinny", *skinny(A=None))
case("vstar_op_gemm_skinny", *skinny(ran=None))
case("vstar_op_gemm_skinny", *skinny(M=65))
case("vstar_op_gemm_skinny", *skinny(K=96))
case("vstar_op_gemm_skinny", *skinny(epi=5))
case("vstar_op_gemm_skinny", *skinny(epi=SILU, N=63))
case("vstar_op_gemm_skinny", *skinny(kernel=2))
case("vstar_op_gemm_skinny", *skinny(out_f32=2))
case("vstar_op_gemm_skinny", *skinny(layout=1, N=72))
case("vstar_op_gemm_skinny", *skinny(layout=1, N=48, epi=SILU))

# ---- the tails: (dev_logits, dtype, rows, vocab, ld, ...) ----
SAMP = {"records": "VqaSampling", "rows": [[1.0, 0, 1.0, 0, 0, 0], [0.5, 4, 0.9, 1, 7, 1]]}
SAMP_BAD = {"records": "VqaSampling", "rows": [[1.0, 0, 1.0, 0, 0, 0], [0.0, 0, 1.0, 0, 0, 0]]}
WARP_BAD = {"records": "VqaWarpers", "rows": [[0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 1.0]]}
case("vstar_vqa_op_sample", None, F16, 2, 8, 8, SAMP, P, None, None)
case("vstar_vqa_op_sample", P, F16, 2, 8, 7, SAMP, P, None, None)
case("vstar_vqa_op_sample", P, F16, 2, 8, 8, SAMP_BAD, P, None, None)
case("vstar_vqa_op_sample_warp", P, 0, 2, 8, 8, SAMP, None, P, None, None, None)
case("vstar_vqa_op_sample_warp", P, F16, 2, 8, 8, SAMP_BAD, WARP_BAD, P, None, None, None)
case("vstar_vqa_op_sample_warp", P, F16, 2, 8, 8, SAMP, WARP_BAD, P, None, None, None)
case("vstar_vqa_op_beam_select", P, F16, 1, 8, 8, f32(0.0), 1, i32(0, 1), 2, None, P, P, None)
case("vstar_vqa_op_beam_select", P, F16, 1, 8, 8, f32(0.0), 1, i32(0, 1), 33, P, P, P, None)
case("vstar_vqa_op_beam_select", P, F16, 1, 8, 8, f32("inf"), 1, i32(0, 1), 2, P, P, P, None)
case("vstar_vqa_op_score", P, F16, 2, 8, 8, i32(1, 2), None, None, None)
case("vstar_vqa_op_score", P, F16, 2, 8, 8, None, P, None, None)
case("vstar_vqa_op_score", P, F16, 2, 8, 8, i32(1, 8), P, None, None)
case("vstar_vqa_op_verify", P, F16, 2, 8, 8, i32(0, 2), 1, i32(3, -1), None, None, P)
case("vstar_vqa_op_verify", P, F16, 2, 8, 8, i32(0, 2), 1, i32(3, 4), None, P, P)
case("vstar_vqa_op_verify", P, F16, 2, 8, 8, i32(0, 2), 1, i32(3, -1), SAMP_BAD, P, P)
case("vstar_vqa_op_verify_warp", P, F16, 2, 8, 8, i32(0, 2), 1, i32(3, -1), None, None, P, None)
case("vstar_vqa_op_verify_warp", P, F16, 2, 8, 8, i32(0, 2), 1, i32(8, -1), SAMP, WARP_BAD, P, P)
case("vstar_vqa_op_verify_warp", P, F16, 2, 8, 8, i32(0, 2), 1, i32(3, -1), SAMP, WARP_BAD, P, P)
case("vstar_vqa_op_edit", None, F16, 1, 8, 8, i32(0, 1, 1, 1), i32(2), f32(1.5))
case("vstar_vqa_op_edit", P, F16, 1, 8, 8, i32(0, 1, 0, 1), i32(2), f32(1.5))
case("vstar_vqa_op_edit", P, F16, 1, 8, 8, i32(0, 1, 1, 1), i32(2), f32(0.0))
case("vstar_vqa_op_logprobs", P, F16, 1, 8, 8, None, 0, P, None, None, None)
case("vstar_vqa_op_logprobs", P, F16, 1, 8, 8, i32(1), 33, P, None, None, None)
case("vstar_vqa_op_logprobs", P, F16, 1, 8, 8, i32(1), 0, P, None, P, None)
case("vstar_vqa_op_logprobs", P, F16, 1, 8, 8, i32(1), 2, P, None, P, None)


def contrast(logits=P, hidden=8, hist_len=(3,), alpha=0.5, prob=(0.5, 0.25)):
    return [logits, F16, 2, 8, 8, P, hidden, P, P, 1, 4, i32(*hist_len), i32(0, 2), f32(*prob), alpha, 2, P, P, P, None]


case("vstar_vqa_op_contrast", *contrast(logits=None))
case("vstar_vqa_op_contrast", *contrast(hidden=12))
case("vstar_vqa_op_contrast", *contrast(alpha=1.5))
case("vstar_vqa_op_contrast", *contrast(prob=(0.5, 1.5)))
case("vstar_vqa_op_contrast", *contrast(hist_len=(4,)))      # the last rule of the chain


# ---- the fp16 GEMM, quantiser and prefill doors ----
def gemm_wq(A=P, M=4, N=64, K=128, epi=0, kernel=1, layout=0):
    return [A, P, P, None, None, P, M, N, K, epi, kernel, None, 0.0, layout]


case("vstar_vqa_op_gemm", P, P, None, None, P, 4, 64, 96, 0, 0, None, 0.0)
case("vstar_vqa_op_quantize_w8", P, 4, 60, P, P, None)
case("vstar_vqa_op_quantize_w4", P, 4, 64, P, P, None)
for door, k_bad in (("vstar_vqa_op_gemm_w8", 96), ("vstar_vqa_op_gemm_w4", 192)):
    case(door, *gemm_wq(A=None))
    case(door, *gemm_wq(K=k_bad))
    case(door, *gemm_wq(kernel=2))
    case(door, *gemm_wq(M=65))
    case(door, *gemm_wq(layout=1, N=72))
    case(door, *gemm_wq(layout=1, N=48, epi=SILU))
case("vstar_vqa_op_kv_quantize", P, 0, P, P, None)
case("vstar_vqa_op_perceiver_attention", P, P, P, 1, 8, 64, 2, 48)
case("vstar_vqa_op_attention", None, 64, P, 64, 1, 64, 2, 128, 1)
case("vstar_vqa_op_attention", P, 64, P, 64, 1, 64, 2, 96, 1)
case("vstar_vqa_op_attention", P, 64, P, 64, 1, 64, 2, 128, 2)
case("vstar_vqa_op_attention", P, 1 << 25, P, 1 << 25, 1 << 13, 1 << 12, 2, 128, 1)
case("vstar_vqa_op_attention", P, 64, P, 63, 1, 64, 2, 128, 1)
case("vstar_vqa_op_layernorm", None, 4, P, P, P, 4, 64, 1e-5, None, 2)      # act comes before the shared rules
case("vstar_vqa_op_layernorm", None, 4, P, P, P, 4, 64, 1e-5, None, 0)
case("vstar_vqa_op_layernorm", P, 3, P, P, P, 4, 64, 1e-5, None, 0)
case("vstar_vqa_op_layernorm", P, 4, P, P, P, 4, 64, 1e-5, i32(0, 1, 2, 4), 1)
case("vstar_vqa_op_rmsnorm", P, 4, None, P, 4, 64, 1e-5, None)
case("vstar_vqa_op_rmsnorm", P, 4, P, P, 0, 64, 1e-5, None)
case("vstar_vqa_op_rmsnorm", P, 4, P, P, 4, 60, 1e-5, None)
case("vstar_vqa_op_rmsnorm", P, 4, P, P, 4, 64, 1e-5, i32(0, -1, 2, 3))
case("vstar_vqa_op_add_bcast", P, None, P, 4, 64, 1)
case("vstar_vqa_op_add_bcast", P, P, P, 4, 64, 5)
case("vstar_vqa_op_add_bcast", P, P, P, 4, 60, 1)
case("vstar_vqa_op_vit_assemble_tokens", P, P, None, P, 1, 4, 64)
case("vstar_vqa_op_vit_assemble_tokens", P, P, P, P, 0, 4, 64)
case("vstar_vqa_op_vit_assemble_tokens", P, P, P, P, 1, 4, 60)


def main():
    lib = _lib.load()
    records = []
    for door, args in CASES:
        rc, message = replay(lib, door, args)
        if rc != ERR_INVALID or not message:
            sys.exit(f"{door}{args}: rc {rc}, message {message!r}: not a host-side refusal")
        records.append({"door": door, "args": args, "rc": rc, "message": message})
    FIXTURE.write_text("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")
    print(f"{len(records)} records from {_lib.LIB_PATH} -> {FIXTURE}")


if __name__ == "__main__":
    main()
