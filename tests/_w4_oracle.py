"""numpy restatement of the int4 group-scaled weight-only decode contract (W4A16, groups of 128; DESIGN.md §8.6,
include/vstar_vqa.h):

  quantize_groups  per row n of W [N, K] (fp16, K % 128 == 0) and group j = k / 128: a = max|W[n, 128 j .. 128 j + 127]|,
                   s = fp16(float32(a) / float32(7)) (one correctly rounded fp32 divide, one round-to-nearest-even conversion),
                   s = min(s, 9352) (7 * 9352 = 65464 is finite in fp16; fp16(65504 / 7) = 9360 would give 7 * s = inf), s = 1 if
                   s == 0; q = clamp(rint(float32(W) / float32(s)), -7, 7) as int8 — -8 never occurs
  pack_words       u = q + 8; eight elements per little-endian 32-bit word, element e in nibble (e >> 1) + 4 (e & 1)
  unpack_words     the inverse, for every nibble value (u = 0 decodes to q = -8)
  dequant_fp16     What = fp16(q) * s as ONE fp16 multiply (RNE, subnormals kept): what the MFMAs see and what the fp16 masters hold
  gemv_w4          C = epilogue(A . What^T + bias) (+ residual) in float64 with _w8_oracle's epilogue rounding points (_h)

numpy's float32 divide is IEEE, np.rint rounds half to even like rintf, float32 -> float16 rounds to nearest even, and
np.float16 * np.float16 is the exact product rounded once (it is computed in float32, which holds the 22-bit product exactly):
the device results must equal these bit for bit.
"""
from __future__ import annotations

import numpy as np

from tests._w8_oracle import _h

GROUP = 128
S_MAX = np.float16(9352.0)


def quantize_groups(W):
    """W [N, K] float16 -> (q int8 [N, K] in -7..7, s float16 [N, K / 128])."""
    W = np.asarray(W)
    assert W.dtype == np.float16 and W.ndim == 2 and W.shape[1] % GROUP == 0
    N, K = W.shape
    w32 = W.astype(np.float32).reshape(N, K // GROUP, GROUP)
    a = np.abs(w32).max(axis=2)
    with np.errstate(over="ignore"):
        s = (a / np.float32(7.0)).astype(np.float16)
    s = np.minimum(s, S_MAX)
    s = np.where(s == 0, np.float16(1.0), s).astype(np.float16)
    q = np.rint(w32 / s.astype(np.float32)[:, :, None])
    q = np.clip(q, -7, 7).astype(np.int8).reshape(N, K)
    return q, s


def pack_words(q):
    """q int8 [N, K] in -8..7 -> uint32 [N, K / 8]."""
    q = np.asarray(q, np.int8)
    N, K = q.shape
    u = (q.astype(np.int32) + 8).astype(np.uint32).reshape(N, K // 8, 8)
    assert u.max() <= 15
    words = np.zeros((N, K // 8), np.uint32)
    for e in range(8):
        words |= u[:, :, e] << np.uint32(4 * ((e >> 1) + 4 * (e & 1)))
    return words


def unpack_words(words):
    """uint32 [N, K / 8] -> q int8 [N, K] in -8..7."""
    words = np.asarray(words, np.uint32)
    N, W8 = words.shape
    q = np.zeros((N, W8, 8), np.int8)
    for e in range(8):
        q[:, :, e] = ((words >> np.uint32(4 * ((e >> 1) + 4 * (e & 1)))) & np.uint32(15)).astype(np.int8) - 8
    return q.reshape(N, W8 * 8)


def dequant_fp16(q, s):
    """fp16(q) * s: one fp16 multiply per weight."""
    q = np.asarray(q, np.int8)
    s = np.asarray(s, np.float16)
    N, K = q.shape
    with np.errstate(over="ignore"):
        out = q.astype(np.float16).reshape(N, K // GROUP, GROUP) * s[:, :, None]
    assert out.dtype == np.float16
    return out.reshape(N, K)


def gemv_w4(A, q, s, bias=None, res=None, epi=0, norm_w=None, norm_eps=1e-5):
    """float64 reference of the W4 GEMV: A [M, K] fp16, q [N, K] int8, s [N, K / 128] fp16; the weights are the dequantised fp16
    values.  Epilogues (0 none, 2 exact GELU, 4 SiLU(gate) * up on packed rows) and the fused RMSNorm have gemv_w8's rounding
    points (_w8_oracle._h)."""
    from math import erf
    x = np.asarray(A, np.float16).astype(np.float64)
    if norm_w is not None:
        rstd = 1.0 / np.sqrt((x * x).mean(axis=1, keepdims=True) + norm_eps)
        x = _h(np.asarray(norm_w, np.float16).astype(np.float64) * _h(x * rstd))
    y = x @ dequant_fp16(q, s).astype(np.float64).T
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
