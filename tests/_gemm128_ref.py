"""References, input builders and shapes of the op tests of the four 128-row GEMM variants (tests/test_gemm128_gpu.py; pinned on
the CPU by tests/test_gemm128_ref.py): 2 = the double buffer, 5 / 6 / 7 = the loader-wave ring on the 128 x 128 / 128 x 64 /
128 x 256 tile (csrc/gemm.hip: gemm128_kernel).

Plain numpy in the idiom of tests/_prefill_ops_ref.py, whose bf16 helpers, probes and sentinels are imported, not copied.  A GEMM
computes C [M, n_out] = epilogue(A [M, K] . W [N, K]^T); bf16 values travel as float32 arrays whose low 16 bits are zero.

`tiled_product` restates the kernels' geometry — K-tiles of 64 through a ring of three slots, 128-row tiles cut into wave rows of
MF 16-row fragments, 64-column spans owned by wave columns — only so that a FAULT of that geometry can be applied to the
reference: the CPU test shows that every probe of the GPU test changes under the fault it is meant to catch."""
import numpy as np
import torch

from tests._prefill_ops_ref import F32, F64, IDENT, SENT16, SENT32, RowMap, bf, bits, int_operands, is_bf16, map_probe  # noqa: F401

VARIANTS = (2, 5, 6, 7)
BM, BK, RING = 128, 64, 3
TILE_N = {2: 128, 5: 128, 6: 64, 7: 256}            # columns of a tile
MF = {2: 4, 5: 4, 6: 2, 7: 4}                        # 16-row fragments of a wave (wave rows of a tile: 128 / (16 MF))
EPI_NONE, EPI_QUICK_GELU, EPI_GELU, EPI_RELU, EPI_SILU_MUL = range(5)

# ---------------------------------------------------------------- shapes (M, N, K): the smallest at which each mechanism is live
# K: 64 one tile, 128 two (nothing re-issued), 192 the ring depth, 256 the first slot reuse, 448 an odd count of wraps, 832 four wraps
# M: the edges of one 128-row tile; 1300 = 11 row tiles (a last GROUP_M group of 3, a tile count that is no multiple of 8)
# N: narrow outputs, the 64 / 128 tile edge, a 44-column tail inside the second 256-wide tile, a wide output with a tail
K_VALUES, M_VALUES, N_VALUES = (64, 128, 192, 256, 448, 832), (1, 127, 128, 129, 200, 1300), (4, 60, 64, 130, 300, 514)
PROBE_SHAPES = [(1, 4, 64), (127, 60, 128), (128, 64, 192), (129, 130, 256), (200, 300, 448), (1300, 130, 832), (1300, 300, 192),
                (200, 514, 832), (128, 514, 64)]
KTILE_SHAPES = [(1, 4, 64), (127, 60, 128), (128, 64, 192), (129, 130, 256), (200, 300, 448), (1300, 300, 832), (200, 514, 832)]
INT_SHAPES = [(127, 64, 64), (200, 300, 128), (1300, 130, 192), (129, 514, 256)]
EPI_SHAPES = [(1300, 130, 64), (200, 60, 192), (129, 300, 256)]
ACT_SHAPES = [(129, 130, 448), (200, 300, 832)]          # SILU_MUL: N = 128 and 320 packed at the same M, K
SILU_N = {130: 128, 300: 320}
RANDOM_SHAPES = [(1300, 300, 832), (200, 514, 832)]
MAP_SHAPES = [(70, 192, 64), (200, 320, 256)]
MAP_A, MAP_C = RowMap(7, 12, 3), RowMap(7, 9, 2)


def probe_col(M, K):
    """One-hot column of the index probe's row r: (r * 37) % K walks every K-tile also where K > M."""
    return (np.arange(M) * 37) % K


def index_probe(M, N, K):
    return map_probe(M, N, K, IDENT, IDENT, col=probe_col(M, K))


def ktile_probe(M, N, K):
    """A = 1 and W[n, k] = 2^(k // 64) where k % 64 == n % 64, else 0: K-tile kt adds exactly 2^kt to every output, so
    C = 2^(K / 64) - 1 everywhere iff every K-tile entered exactly once."""
    A = np.ones((M, K), F32)
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    W = np.where(k % BK == n % BK, 2.0 ** (k // BK), 0.0).astype(F32)
    return A, W, np.full((M, N), 2.0 ** (K // BK) - 1, F64)


def bias_quarters(N):
    """Small multiples of 1/4, both signs."""
    return ((np.arange(N) % 9 - 4) / 4.0).astype(F32)


def residual_mod8(M, N):
    return ((np.arange(M)[:, None] + np.arange(N)[None, :]) % 8).astype(F32)


def pack_gate_up(gate, up):
    """[F, K] x 2 -> the packed [2 F, K] weight of VSTAR_EPI_SILU_MUL: blocks of 16 gate rows followed by their 16 up rows."""
    F_, K = gate.shape
    assert up.shape == gate.shape and F_ % 16 == 0
    return np.stack([gate.reshape(F_ // 16, 16, K), up.reshape(F_ // 16, 16, K)], axis=1).reshape(2 * F_, K)


def unpack_gate_up(acc):
    """[M, 2 F] accumulators of the packed columns -> (gate [M, F], up [M, F])."""
    M, N = acc.shape
    x = acc.reshape(M, N // 32, 2, 16)
    return x[:, :, 0].reshape(M, N // 2), x[:, :, 1].reshape(M, N // 2)


# ---------------------------------------------------------------- exactness
def exact_fp32(A, W, unit=1.0):
    """Whether every product a * w is a multiple of `unit` and every partial sum of a row of them, in ANY order, stays an integer
    multiple of `unit` below 2^24 units: then fp32 accumulation is exact whatever the order, and so are the bits."""
    A, W = np.asarray(A, F64), np.asarray(W, F64)
    if not (np.array_equal(A / unit, np.round(A / unit)) and np.array_equal(W, np.round(W))):
        return False
    return float((np.abs(A) @ np.abs(W).T).max()) / unit < 2.0 ** 24


def is_fp32(x):
    return bool(np.array_equal(np.asarray(x, F64), np.asarray(x, F64).astype(F32).astype(F64)))


# ---------------------------------------------------------------- the epilogue (gemm_epilogue.hpp: gemm_epilogue_store)
def _act(t, epi):
    x = torch.from_numpy(np.ascontiguousarray(t, F64))
    if epi == EPI_QUICK_GELU:
        x = x * torch.sigmoid(1.702 * x)
    elif epi == EPI_GELU:
        x = torch.nn.functional.gelu(x)
    elif epi == EPI_RELU:
        x = torch.relu(x)
    return x.numpy()


def epilogue(acc, epi=EPI_NONE, out_f32=False, bias=None, res=None, row_scale=None):
    """float64 reference of the rounding points.  16-bit output: acc (x row_scale) + bias -> round; activation -> round; + residual ->
    round.  fp32 output: nothing is rounded.  SILU_MUL: acc holds the packed gate | up columns, the result is
    round(silu(round(gate))) x round(up), then as above.  Returned as float64 (bf16 values for 16-bit output)."""
    r = (lambda x: x) if out_f32 else (lambda x: bf(x).astype(F64))
    acc = np.asarray(acc, F64)
    if row_scale is not None:
        acc = acc * np.asarray(row_scale, F64)[:, None]
    if epi == EPI_SILU_MUL:
        assert bias is None and not out_f32
        gate, up = unpack_gate_up(acc)
        g = bf(gate).astype(F64)
        t = bf(g / (1.0 + np.exp(-g))).astype(F64) * bf(up).astype(F64)
    else:
        t = r(acc + (0 if bias is None else np.asarray(bias, F64)[None, :]))
        t = _act(t, epi)
    if res is not None:
        t = r(t) + np.asarray(res, F64)
    return r(t)


def product(A, W):
    return np.asarray(A, F64) @ np.asarray(W, F64).T


def fp32_sum_bound(A, W, bias=None):
    """(K + 2) 2^-24 (|A| |W|^T + |bias|): K products (exact: 8 x 8 significant bits) added in fp32 in ANY order — at most K roundings
    of relative 2^-24 each on partial sums bounded by sum |a w| — plus the bias add, first order in 2^-24 with one spare unit."""
    K = np.asarray(A).shape[1]
    mag = np.abs(np.asarray(A, F64)) @ np.abs(np.asarray(W, F64)).T
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, F64))[None, :]
    return (K + 2) * 2.0 ** -24 * mag


def act_bound(ref, epi):
    """The bound tests/test_ops_gpu.py uses for these epilogues against the fp32 computation."""
    return np.abs(ref) * 2.0 ** -7 + (1e-2 if epi == EPI_SILU_MUL else 2e-2)


# ---------------------------------------------------------------- the kernels' geometry, with faults
def stale_tile(kt, nk):
    """What ring slot (kt - 1) % 3 holds while K-tile kt is due: K-tile kt - 1, or — before anything was consumed — K-tile kt + 2
    where the loader has issued it; None: the slot was never written."""
    if kt >= 1:
        return kt - 1
    return kt + 2 if kt + 2 < nk else None


def tiled_product(A, W, variant, fault=None):
    """A . W^T in float64, assembled the way gemm128_kernel does.  fault (None = none):
      ("drop", kt) / ("twice", kt)        K-tile kt of every output tile left out / added twice
      ("stale", kt)                        K-tile kt read from ring slot (kt - 1) % 3 (stale_tile)
      ("frag_shift", m)                    fragment m of every wave takes the A rows of the fragment after it (cyclic in the wave)
      ("wave_rows",)                       A rows fetched with the wave-row stride of the OTHER fragment count (MF 2 <-> 4), stored with this one's
      ("span",)                            every 64-column span stored where its neighbouring span (s ^ 1) belongs"""
    A, W = np.asarray(A, F64), np.asarray(W, F64)
    M, K = A.shape
    N, nk, mf = W.shape[0], K // BK, MF[variant]
    kind = fault[0] if fault else None
    # rows: which A row each output row accumulates
    src = np.arange(M)
    if kind in ("frag_shift", "wave_rows"):
        r = np.arange(M)
        m0, rr = r // BM * BM, r % BM
        wr, m, fr = rr // (16 * mf), rr // 16 % mf, rr % 16
        if kind == "frag_shift":
            m = np.where(m == fault[1], (m + 1) % mf, m)
            rr = wr * 16 * mf + m * 16 + fr
        else:
            rr = (wr * 16 * (6 - mf) + m * 16 + fr) % BM
        src = np.minimum(m0 + rr, M - 1)                       # the loaders clamp rows >= M to M - 1
    C = np.zeros((M, N), F64)
    for kt in range(nk):
        use, times = kt, 1
        if kind == "drop" and kt == fault[1]:
            times = 0
        elif kind == "twice" and kt == fault[1]:
            times = 2
        elif kind == "stale" and kt == fault[1]:
            use = stale_tile(kt, nk)
            times = 0 if use is None else 1
        if times:
            C += times * (A[src, use * BK:(use + 1) * BK] @ W[:, use * BK:(use + 1) * BK].T)
    if kind == "span":
        spans = (N + 63) // 64
        pad = np.zeros((M, (spans + spans % 2) * 64), F64)      # W rows >= N are zero padding: their columns compute 0
        pad[:, :N] = C
        C = pad.reshape(M, -1, 2, 64)[:, :, ::-1].reshape(M, -1)[:, :N]
    return C


def k_faults(K):
    nk = K // BK
    f = []
    for kt in sorted({0, nk // 2, nk - 1}):
        f += [("drop", kt), ("twice", kt)]
        if nk > 1:
            f.append(("stale", kt))
    return f


def geometry_faults(variant):
    return [("frag_shift", m) for m in range(MF[variant])] + [("wave_rows",), ("span",)]
