"""The int8 weight-only decode contract (tests/_w8_oracle.py) on hand-worked rows, and the ABI surface of the mode."""
import ctypes
import os

import numpy as np

from tests._w8_oracle import dequant_fp16, gemv_w8, quantize_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_worked_rows():
    W = np.zeros((5, 8), np.float16)
    W[1] = [127, -127, 0.5, 1.5, 2.5, -2.5, 126.5, -0.5]        # s = 1 exactly: ties round to even
    W[2] = [254, 1, 3, 5, -1, -3, 253, -254]                    # s = 2 exactly: 0.5, 1.5, 2.5, ... again
    W[3] = [65504, -65504, 257.9, 0, 1, -1, 32752, 515.5]       # the largest fp16
    W[4] = [6e-8, -6e-8, 1.2e-7, 5.96e-8, 0, 0, 0, 0]           # subnormals only
    q, s = quantize_rows(W)
    assert q.dtype == np.int8 and s.dtype == np.float32
    assert s[0] == 1.0 and not q[0].any()                       # all-zero row: s = 1, q = 0
    assert s[1] == 1.0 and q[1].tolist() == [127, -127, 0, 2, 2, -2, 126, 0]
    assert s[2] == 2.0 and q[2].tolist() == [127, 0, 2, 2, 0, -2, 126, -127]
    assert s[3] == np.float32(65504.0) / np.float32(127.0)
    assert q[3, 0] == 127 and q[3, 1] == -127 and q[3, 3] == 0
    # 32752 / s = 63.4999983...: the fp32 divide of the contract rounds it to 63.5 exactly, and rint takes the tie to the even 64
    # (a float64 quotient would give 63): the quantiser is defined in fp32
    assert np.float32(32752.0) / s[3] == np.float32(63.5) and q[3, 6] == 64
    assert abs(int(q[4, 0])) == 127 or abs(int(q[4, 2])) == 127     # +-amax -> +-127 for the subnormal row too
    assert q.min() >= -127                                      # -128 is never produced
    What = dequant_fp16(q, s)
    assert What.dtype == np.float16
    assert What[1].tolist() == [127, -127, 0, 2, 2, -2, 126, 0]
    assert float(What[3, 0]) == 65504.0 and float(What[3, 1]) == -65504.0


def test_minus_128_never_produced_and_amax_maps_to_127():
    g = np.random.default_rng(0)
    W = (g.standard_normal((64, 256)) * np.exp(g.uniform(-8, 8, (64, 1)))).astype(np.float16)
    W[7] = -np.abs(W[7])                                        # a row whose extreme is negative
    q, s = quantize_rows(W)
    assert q.min() >= -127 and q.max() <= 127
    am = np.abs(W.astype(np.float32)).argmax(axis=1)
    assert (np.abs(q[np.arange(64), am].astype(np.int32)) == 127).all()
    assert (np.sign(q[np.arange(64), am]) == np.sign(W[np.arange(64), am].astype(np.float32))).all()


def test_round_trip_error_bound():
    """dequant(quantize(W)) is within s/2 (the rounding of q) + 1 fp16 ulp (the rounding of What) of W, per element."""
    g = np.random.default_rng(1)
    W = (g.standard_normal((48, 512)) * np.exp(g.uniform(-6, 6, (48, 1)))).astype(np.float16)
    W[3] = 0
    q, s = quantize_rows(W)
    What = dequant_fp16(q, s).astype(np.float64)
    ulp = np.spacing(np.abs(What).astype(np.float16)).astype(np.float64)
    err = np.abs(What - W.astype(np.float64))
    assert (err <= s.astype(np.float64)[:, None] / 2 + ulp).all(), float((err - s[:, None] / 2 - ulp).max())
    assert not What[3].any()


def test_gemv_reference_equals_dequantised_matmul():
    g = np.random.default_rng(2)
    A = g.standard_normal((3, 64)).astype(np.float16)
    W = (g.standard_normal((32, 64)) / 8).astype(np.float16)
    q, s = quantize_rows(W)
    ref = A.astype(np.float64) @ (q.astype(np.float64) * s.astype(np.float64)[:, None]).T
    assert np.allclose(gemv_w8(A, q, s), ref, rtol=1e-12, atol=1e-12)
    out = gemv_w8(A, q, s, epi=4)
    assert out.shape == (3, 16)


def test_abi_surface_of_the_mode():
    from vstar_amd import _lib
    from vstar_amd.config import CVqaConfig, VQAConfig
    header = open(os.path.join(ROOT, "include", "vstar_vqa.h")).read()
    for sym in ("vstar_vqa_decode_weight_bits", "vstar_vqa_op_quantize_w8", "vstar_vqa_op_gemm_w8"):
        assert sym in _lib.EXPORTS_VQA and sym + "(" in header
    assert ctypes.sizeof(CVqaConfig) == 4 * 33
    assert CVqaConfig.decode_weight_bits.offset == 4 * 25
    assert VQAConfig.tiny().decode_weight_bits == 0
    assert VQAConfig.tiny(decode_weight_bits=8).to_c().decode_weight_bits == 8
    lib = _lib.load()
    h = ctypes.c_void_p()
    c = VQAConfig.tiny(decode_weight_bits=4).to_c()
    assert lib.vstar_vqa_create(ctypes.byref(c), 0, ctypes.byref(h)) == -1      # VSTAR_ERR_INVALID, with or without a GPU
    assert b"decode_weight_bits" in lib.vstar_vqa_last_error(None)
