"""The refusals of the op-level doors (csrc/ops.hip: vstar_op_*, csrc/vqa_ops.hip: vstar_vqa_op_*), pinned byte for byte.

tests/golden/op_door_refusals.json is a list of {door, args, rc, message} records: calls that a door refuses with VSTAR_ERR_INVALID on
the host, before any HIP call, so the answer is the same with and without a device and nothing is launched.  The records were taken
from the library as it was BEFORE the doors moved into files of their own (tools/record_op_door_refusals.py, run against that build);
this test replays them against the library under test.  Doors whose checks are a chain contribute their first and their last refusal,
so a reordered chain shows.

Encoding of `args` (one entry per C argument): a number or null is passed as it is (a number in a pointer position is a dummy device
pointer: refused calls dereference host arrays only); {"i32": [...]} / {"f32": [...]} is a host array; {"struct": NAME, "fields": {...}}
a _lib structure passed by pointer, its fields encoded the same way; {"records": NAME, "rows": [[...], ...]} an array of _lib
structures; {"out": "int"} an int the door may write."""
import ctypes
import json
from pathlib import Path

import numpy as np
import pytest

from vstar_amd import _lib

FIXTURE = Path(__file__).resolve().parent / "golden" / "op_door_refusals.json"
ERR_INVALID = -1      # VSTAR_ERR_INVALID (include/vstar_hip.h)

# doors without a refusing host-side check: one launcher, then synchronise (or a pure host function that cannot fail)
NO_HOST_CHECK = {
    "vstar_op_layernorm", "vstar_op_rmsnorm", "vstar_op_rms_rstd", "vstar_op_ln_fold", "vstar_op_quantize_mx", "vstar_op_attention_mx",
    "vstar_op_gemm_last_tile", "vstar_op_gemm_last_mode", "vstar_op_mx_scale_bytes", "vstar_op_mx_scale_offset",
    "vstar_op_attention_workspace",
    "vstar_op_owl_class_logits", "vstar_op_owl_box_finish", "vstar_op_upsample2x_im2col3x3", "vstar_op_hyper_mask",
    "vstar_op_im2col_patch", "vstar_op_vit_assemble_tokens", "vstar_op_llm_embed_text", "vstar_op_add_bcast",
    "vstar_op_add_bcast_repeat", "vstar_op_bcast_rows", "vstar_op_owl_cls_mul", "vstar_op_gather_rows", "vstar_op_argmax_rows",
    "vstar_op_layernorm_ex", "vstar_op_rmsnorm_ex", "vstar_op_scale_cols", "vstar_op_fill", "vstar_op_quantize_rows_fp8",
    "vstar_op_layernorm_quant_fp8", "vstar_op_rmsnorm_quant_fp8", "vstar_op_small_attention",
}
# doors whose checks are a chain: at least two different refusals each (the first and the last rule of the chain)
CHAINED = {
    "vstar_op_gemm", "vstar_op_gemm_norm", "vstar_op_gemm_plan", "vstar_op_gemm_ex", "vstar_op_gemm_skinny", "vstar_op_rope",
    "vstar_op_attention_grouped", "vstar_op_attention_mx_grouped",
    "vstar_op_rope_kv_append", "vstar_op_cached_attention", "vstar_vqa_op_rope_kv_append", "vstar_vqa_op_cached_attention",
    "vstar_vqa_op_layernorm", "vstar_vqa_op_rmsnorm", "vstar_vqa_op_gemm_w8", "vstar_vqa_op_gemm_w4",
    "vstar_vqa_op_sample", "vstar_vqa_op_sample_warp", "vstar_vqa_op_beam_select", "vstar_vqa_op_score", "vstar_vqa_op_verify",
    "vstar_vqa_op_verify_warp", "vstar_vqa_op_edit", "vstar_vqa_op_logprobs", "vstar_vqa_op_contrast",
    "vstar_vqa_op_attention", "vstar_vqa_op_add_bcast", "vstar_vqa_op_vit_assemble_tokens",
}


def _decode(a, keep):
    """One encoded argument (or structure field) as what ctypes takes; `keep` holds what must outlive the call."""
    if not isinstance(a, dict):
        return a
    if "i32" in a or "f32" in a:
        key = "i32" if "i32" in a else "f32"
        arr = np.array([float(v) for v in a[key]], dtype=np.int32 if key == "i32" else np.float32)
        keep.append(arr)
        return arr.ctypes.data
    if "struct" in a:
        s = getattr(_lib, a["struct"])(**{k: _decode(v, keep) for k, v in a["fields"].items()})
        keep.append(s)
        return ctypes.byref(s)
    if "records" in a:
        T = getattr(_lib, a["records"])
        recs = (T * len(a["rows"]))(*[T(*row) for row in a["rows"]])
        keep.append(recs)
        return ctypes.addressof(recs)
    if a.get("out") == "int":
        v = ctypes.c_int(-7)
        keep.append(v)
        return ctypes.byref(v)
    raise ValueError(a)


def replay(lib, door, args):
    """(rc, message) of one encoded call; the message is the thread's, read through the door's half of the library."""
    keep = []
    rc = getattr(lib, door)(*[_decode(a, keep) for a in args])
    last_error = lib.vstar_vqa_last_error if door.startswith("vstar_vqa_") else lib.vstar_last_error
    return rc, last_error(None).decode()


@pytest.fixture(scope="module")
def records():
    return json.loads(FIXTURE.read_text())


def test_every_door_is_covered_or_excluded(records):
    doors = {n for n in _lib.EXPORTS + _lib.EXPORTS_VQA if "_op_" in n}
    covered = {r["door"] for r in records}
    assert not covered & NO_HOST_CHECK
    assert covered | NO_HOST_CHECK == doors, sorted(doors ^ (covered | NO_HOST_CHECK))
    assert CHAINED <= covered
    for door in sorted(CHAINED):
        assert len({r["message"] for r in records if r["door"] == door}) >= 2, door


def test_fixture_holds_host_side_refusals_only(records):
    assert all(r["rc"] == ERR_INVALID and r["message"] for r in records)


def test_refusals_replay_byte_for_byte(records):
    lib = _lib.load()
    for r in records:
        rc, message = replay(lib, r["door"], r["args"])
        assert (rc, message) == (r["rc"], r["message"]), (r["door"], r["args"])
