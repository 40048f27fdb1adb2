"""The int4 group-scaled weight-only decode contract (tests/_w4_oracle.py) on hand-worked groups, the storage
order of the nibbles, the ABI surface of the mode and the user-level spelling `decode_weight_bits=4`."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest

from tests._w4_oracle import dequant_fp16, gemv_w4, pack_words, quantize_groups, unpack_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # the smallest fp16 subnormal


def _groups(*firsts):
    """One row per argument: a group of 128 whose leading elements are given, the rest zero."""
    W = np.zeros((len(firsts), 128), np.float16)
    for i, f in enumerate(firsts):
        W[i, :len(f)] = f
    return W


def test_hand_worked_groups():
    W = _groups([],                                             # 0: a zero group
                [7, -7, 0.5, 1.5, 2.5, -2.5, 3.5, 6.5],         # 1: s = 1 exactly: the fp32 quotient is x.5 -> half to even
                [14, 1, 3, 5, -1, -3, 13, -14],                 # 2: s = 2 exactly: 0.5, 1.5, 2.5, ... again
                [65504, -65504, 9352, 4676, 0, 1, -1, 60000],   # 3: the largest fp16
                [1 * U, -1 * U],                                # 4: a / 7 rounds to zero -> s = 1
                [3 * U, 2 * U],                                 # 5: 3/7 of the smallest subnormal rounds to zero too
                [7 * U, -3 * U, 4 * U],                         # 6: s = 2^-24 exactly
                [10 * U, -10 * U, 3 * U, 7.0 * U],              # 7: 10/7 rounds DOWN to s = 2^-24: |W| / s = 10 > 7 clamps
                [1023 * U, -512 * U, 100 * U, 73 * U])          # 8: subnormal weights, subnormal scale
    q, s = quantize_groups(W)
    assert q.dtype == np.int8 and s.dtype == np.float16 and s.shape == (9, 1)
    What = dequant_fp16(q, s)
    assert What.dtype == np.float16 and np.isfinite(What.astype(np.float32)).all()
    assert s[0, 0] == 1 and not q[0].any() and not What[0].any()
    assert s[1, 0] == 1 and q[1, :8].tolist() == [7, -7, 0, 2, 2, -2, 4, 6]
    assert s[2, 0] == 2 and q[2, :8].tolist() == [7, 0, 2, 2, 0, -2, 6, -7]
    # 65504 / 7 = 9357.7 -> fp16 9360, and 7 * 9360 = 65520 rounds to inf in fp16: the scale is capped at 9352
    assert float(np.float16(np.float32(65504) / np.float32(7))) == 9360.0 and s[3, 0] == 9352
    assert q[3, :4].tolist() == [7, -7, 1, 0]                   # 4676 / 9352 = 0.5 exactly -> 0 (half to even)
    assert float(What[3, 0]) == 65472.0 and float(What[3, 1]) == -65472.0     # 7 * 9352 = 65464, one rounding (ulp 32): finite
    assert s[4, 0] == 1 and not q[4].any()
    assert s[5, 0] == 1 and not q[5].any()
    assert float(s[6, 0]) == U and q[6, :3].tolist() == [7, -3, 4] and What[6, :3].tolist() == [7 * U, -3 * U, 4 * U]
    assert float(s[7, 0]) == U and q[7, :4].tolist() == [7, -7, 3, 7] and float(What[7, 0]) == 7 * U
    assert 0 < float(s[8, 0]) < 2.0 ** -14 and abs(int(q[8, 0])) == 7          # a subnormal scale; +-amax -> +-7
    assert q.min() >= -7 and q.max() <= 7                       # -8 is never produced


def test_random_groups_keep_the_contract():
    g = np.random.default_rng(0)
    W = (g.standard_normal((64, 512)) * np.exp(g.uniform(-12, 9, (64, 4)).repeat(128, axis=1))).astype(np.float16)
    W[7] = -np.abs(W[7])
    q, s = quantize_groups(W)
    What = dequant_fp16(q, s)
    assert q.min() >= -7 and q.max() <= 7 and (s > 0).all() and (s <= 9352).all()
    assert np.isfinite(What.astype(np.float32)).all()
    # the group's extreme maps to +-7 with its sign
    w = W.astype(np.float32).reshape(64, 4, 128)
    am = np.abs(w).argmax(axis=2)
    qa = np.take_along_axis(q.reshape(64, 4, 128), am[:, :, None], axis=2)[:, :, 0]
    wa = np.take_along_axis(w, am[:, :, None], axis=2)[:, :, 0]
    assert (np.abs(qa.astype(np.int32)) == 7).all() and (np.sign(qa) == np.sign(wa)).all()
    # per element: within s / 2 (the rounding of q) + one fp16 ulp (the rounding of What); Gaussian groups land near rel-L2 0.117
    err = np.abs(What.astype(np.float64) - W.astype(np.float64)).reshape(64, 4, 128)
    ulp = np.spacing(np.abs(What)).astype(np.float64).reshape(64, 4, 128)
    assert (err <= s.astype(np.float64)[:, :, None] / 2 + ulp).all()
    G = g.standard_normal((256, 128)).astype(np.float16)
    qg, sg = quantize_groups(G)
    rel = np.linalg.norm(dequant_fp16(qg, sg).astype(np.float64) - G.astype(np.float64)) / np.linalg.norm(G.astype(np.float64))
    assert 0.09 < rel < 0.14, rel


def test_pack_unpack_all_nibbles_in_all_positions():
    q = np.zeros((16, 64), np.int8)
    for v in range(16):
        for e in range(8):
            q[v, e * 8:(e + 1) * 8] = 0                 # word e of row v: value v - 8 at position e, zero elsewhere
            q[v, e * 8 + e] = v - 8
    words = pack_words(q)
    assert words.dtype == np.uint32 and words.shape == (16, 8)
    assert np.array_equal(unpack_words(words), q)
    for v in range(16):
        for e in range(8):
            nib = (e >> 1) + 4 * (e & 1)
            assert int(words[v, e]) == (0x88888888 & ~(0xF << (4 * nib))) | (v << (4 * nib))
    # the order makes `x & 0x000F000F | 0x64006400` the fp16 pair (1024 + u_e0, 1024 + u_e1); shifted by 4, 8, 12: pairs 1, 2, 3
    g = np.random.default_rng(1)
    qq = g.integers(-8, 8, (4, 64)).astype(np.int8)
    x = pack_words(qq)
    for pair in range(4):
        h = (((x >> np.uint32(4 * pair)) & np.uint32(0x000F000F)) | np.uint32(0x64006400))
        lo = (h & np.uint32(0xFFFF)).astype(np.uint16).view(np.float16).astype(np.float32) - 1032
        hi = (h >> np.uint32(16)).astype(np.uint16).view(np.float16).astype(np.float32) - 1032
        assert np.array_equal(lo, qq.reshape(4, 8, 8)[:, :, 2 * pair]) and np.array_equal(hi, qq.reshape(4, 8, 8)[:, :, 2 * pair + 1])
    all_q = np.arange(-8, 8, dtype=np.int8).repeat(8)[None, :]
    assert np.array_equal(unpack_words(pack_words(all_q)), all_q)


def test_gemv_reference_equals_dequantised_matmul():
    g = np.random.default_rng(2)
    A = g.standard_normal((3, 256)).astype(np.float16)
    W = (g.standard_normal((32, 256)) / 8).astype(np.float16)
    q, s = quantize_groups(W)
    ref = A.astype(np.float64) @ dequant_fp16(q, s).astype(np.float64).T
    assert np.allclose(gemv_w4(A, q, s), ref, rtol=1e-12, atol=1e-12)
    assert gemv_w4(A, q, s, epi=4).shape == (3, 16)


def test_abi_surface_of_the_mode():
    from vstar_amd import _lib
    from vstar_amd.config import WFMT_W4G128, CVqaConfig, VQAConfig
    header = open(os.path.join(ROOT, "include", "vstar_vqa.h")).read()
    for sym in ("vstar_vqa_op_quantize_w4", "vstar_vqa_op_gemm_w4"):
        assert sym in _lib.EXPORTS_VQA and sym + "(" in header
    assert "VSTAR_VQA_WFMT_W4G128 1" in header and WFMT_W4G128 == 1
    assert ctypes.sizeof(CVqaConfig) == 4 * 33
    assert CVqaConfig.decode_weight_bits.offset == 4 * 25
    assert CVqaConfig.decode_weight_format.offset == 4 * 26
    assert VQAConfig.tiny().decode_weight_format == 0
    c = VQAConfig.tiny(decode_weight_format=1).to_c()
    assert c.decode_weight_format == 1 and c.decode_weight_bits == 0
    lib = _lib.load()
    for name in ("vstar_vqa_op_quantize_w4", "vstar_vqa_op_gemm_w4"):
        assert hasattr(lib, name)
    for bad in (VQAConfig.tiny(decode_weight_format=1, decode_weight_bits=8), VQAConfig.tiny(decode_weight_format=2),
                VQAConfig.tiny(decode_weight_format=1, llm_mlp=320), VQAConfig.tiny(decode_weight_format=-1)):
        h = ctypes.c_void_p()
        c = bad.to_c()
        assert lib.vstar_vqa_create(ctypes.byref(c), 0, ctypes.byref(h)) == -1      # VSTAR_ERR_INVALID, with or without a GPU
        assert b"decode_weight_format" in lib.vstar_vqa_last_error(None)
    # the value 4 in decode_weight_bits stays invalid, whatever the format says
    h = ctypes.c_void_p()
    c = VQAConfig.tiny(decode_weight_bits=4, decode_weight_format=1).to_c()
    assert lib.vstar_vqa_create(ctypes.byref(c), 0, ctypes.byref(h)) == -1
    assert b"decode_weight_bits" in lib.vstar_vqa_last_error(None)


def test_user_level_translation_of_four_bits():
    from vstar_amd.api import load_pretrained_model
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa import VQA_LLM
    c4 = VQAConfig.tiny().with_decode_bits(4)
    assert (c4.decode_weight_bits, c4.decode_weight_format, c4.decode_bits()) == (0, 1, 4)
    c8 = c4.with_decode_bits(8)
    assert (c8.decode_weight_bits, c8.decode_weight_format, c8.decode_bits()) == (8, 0, 8)
    c0 = c8.with_decode_bits(0)
    assert c0 == VQAConfig.tiny() and c0.decode_bits() == 0
    with pytest.raises(ValueError):
        VQAConfig.tiny().with_decode_bits(2)
    # VQA_LLM: the engine's mode is fixed when it is built; asking for what it has is fine, asking for another mode is an error
    eng4 = SimpleNamespace(cfg=c4)
    assert VQA_LLM(engine=eng4, decode_weight_bits=4).cfg == c4
    with pytest.raises(ValueError, match="decode_weight_bits"):
        VQA_LLM(engine=SimpleNamespace(cfg=VQAConfig.tiny()), decode_weight_bits=4)
    # bitsandbytes NF4 is another format: load_4bit keeps raising, and points at the engine's own mode
    with pytest.raises(NotImplementedError, match="decode_weight_bits=4"):
        load_pretrained_model("nowhere", load_4bit=True)
    import vstar_bench_eval
    assert vstar_bench_eval.parse_args(["--vqa-decode-bits", "4"]).vqa_decode_bits == 4
