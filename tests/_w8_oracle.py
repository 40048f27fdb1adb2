"""numpy restatement of the int8 weight-only decode contract (include/vstar_vqa.h):

  quantize_rows  per row n of W [N, K] (fp16): a = max|W[n,:]|, s = float32(a) / float32(127) (one correctly rounded fp32
                 divide; 1 when a == 0), q = clamp(rint(float32(W) / s), -127, 127) as int8 — -128 never occurs
  dequant_fp16   What = fp16(float32(q) * s): what the fp16 masters hold once the mode is on (prefill, calls of > 64 rows)
  gemv_w8        C = epilogue((A . q^T) * s + bias) (+ residual) in float64, with the fp16 rounding points of gemm_epilogue_store

numpy's float32 divide and multiply are IEEE (correctly rounded), np.rint rounds half to even like rintf, and float32 -> float16
rounds to nearest even like v_cvt_f16_f32: the device results must equal these bit for bit.
"""
from __future__ import annotations

import numpy as np


def quantize_rows(W):
    """W [N, K] float16 -> (q int8 [N, K], s float32 [N])."""
    W = np.asarray(W)
    assert W.dtype == np.float16 and W.ndim == 2
    w32 = W.astype(np.float32)
    a = np.abs(w32).max(axis=1)
    s = np.where(a == 0, np.float32(1.0), a / np.float32(127.0)).astype(np.float32)
    q = np.rint(w32 / s[:, None])
    q = np.clip(q, -127, 127).astype(np.int8)
    return q, s


def dequant_fp16(q, s):
    """fp16(float32(q) * s): one fp32 multiply, one rounding to fp16."""
    return (np.asarray(q, np.int8).astype(np.float32) * np.asarray(s, np.float32)[:, None]).astype(np.float16)


def _h(x):
    """round through fp16 (a rounding point of the epilogue)"""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def gemv_w8(A, q, s, bias=None, res=None, epi=0, norm_w=None, norm_eps=1e-5):
    """float64 reference of the W8 GEMV: A [M, K] fp16, q [N, K] int8, s [N] fp32; epi 0 none, 2 exact GELU, 4 SiLU(gate) * up on
    packed rows (blocks of 16 gate rows followed by 16 up rows).  The fused RMSNorm has LlamaRMSNorm's rounding points."""
    from math import erf
    x = np.asarray(A, np.float16).astype(np.float64)
    if norm_w is not None:
        rstd = 1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + norm_eps)
        x = _h(np.asarray(norm_w, np.float16).astype(np.float64) * _h(x * rstd))
    y = (x @ np.asarray(q, np.int8).astype(np.float64).T) * np.asarray(s, np.float32).astype(np.float64)[None, :]
    if bias is not None:
        y = y + np.asarray(bias, np.float16).astype(np.float64)[None, :y.shape[1]]
    if epi == 2:
        t = _h(y)
        y = 0.5 * t * (1.0 + np.vectorize(erf)(t * 0.70710678118654752))
    elif epi == 4:
        M, N = y.shape
        r = y.reshape(M, N // 32, 2, 16)
        g = _h(r[:, :, 0])
        y = (_h(g / (1.0 + np.exp(-g))) * _h(r[:, :, 1])).reshape(M, N // 2)
    elif epi != 0:
        raise ValueError(epi)
    if res is not None:
        y = _h(y) + np.asarray(res, np.float16).astype(np.float64)
    return y
