"""tests/_gemm128_ref.py pinned on the CPU: the builders, that every case the GPU test calls exact IS exact (all partial sums
representable: any summation order gives the same bits), and that every probe changes under the fault it is meant to catch —
the fault applied to the reference's restatement of the kernels' geometry (tiled_product)."""
import numpy as np
import pytest

from tests import _gemm128_ref as G

F64 = np.float64


def test_shapes_cover_every_value_of_every_axis():
    # every case runs once per variant, so a value that appears in a list appears with every variant
    for shapes in (G.PROBE_SHAPES, G.KTILE_SHAPES + G.INT_SHAPES):
        assert {m for m, _, _ in shapes} == set(G.M_VALUES)
        assert {k for _, _, k in shapes} == set(G.K_VALUES)
        assert {n for _, n, _ in shapes} == set(G.N_VALUES)
    assert {(1300, 130), (1300, 300)} <= {(m, n) for m, n, _ in G.PROBE_SHAPES}
    every = G.PROBE_SHAPES + G.KTILE_SHAPES + G.INT_SHAPES + G.EPI_SHAPES + G.ACT_SHAPES + G.RANDOM_SHAPES + G.MAP_SHAPES
    assert all(m <= 1300 and n <= 514 and k <= 832 and k % 64 == 0 for m, n, k in every)
    assert all(k <= 256 for _, _, k in G.INT_SHAPES + G.MAP_SHAPES)          # int_operands: |C| <= K must be a bf16 integer
    assert all(n % 64 == 0 for _, n, _ in G.MAP_SHAPES)                      # the statistics need whole spans
    # (200, 320, 256): the ring wraps and the 256-wide tile holds a second, partial tile
    assert (200, 320, 256) in G.MAP_SHAPES and 256 // G.BK > G.RING and 256 < 320 < 512


def test_tiled_product_is_the_product():
    A, W = G.int_operands(200, 130, 256, 1)
    for v in G.VARIANTS:
        assert np.array_equal(G.tiled_product(A, W, v), G.product(A, W))


@pytest.mark.parametrize("M,N,K", G.PROBE_SHAPES)
def test_index_probe_is_exact_and_names_rows_and_columns(M, N, K):
    p = G.index_probe(M, N, K)
    col = G.probe_col(M, K)
    assert G.exact_fp32(p.A, p.W) and G.is_bf16(p.A) and G.is_bf16(p.W) and G.is_bf16(p.C)
    assert np.array_equal(p.C, G.product(p.A, p.W)) and p.c_written.all()
    assert np.array_equal(p.C, p.W[:, col].T)
    if M >= K:
        assert set(col) == set(range(K))                     # 37 is odd: every column, so every K-tile, is hit
    else:
        assert len({c // G.BK for c in col}) == min(M, K // G.BK)
    assert len({tuple(r) for r in p.W.T}) == min(K, 251)     # the probe's answers tell the k apart (W repeats after 251)


@pytest.mark.parametrize("variant", G.VARIANTS)
@pytest.mark.parametrize("M,N,K", [s for s in G.PROBE_SHAPES if s[0] >= 127])
def test_index_probe_detects_row_and_span_faults(M, N, K, variant):
    p = G.index_probe(M, N, K)
    for fault in G.geometry_faults(variant):
        assert not np.array_equal(G.tiled_product(p.A, p.W, variant, fault), p.C), fault


@pytest.mark.parametrize("M,N,K", G.KTILE_SHAPES)
def test_ktile_probe_is_exact_and_counts_k_tiles(M, N, K):
    A, W, C = G.ktile_probe(M, N, K)
    assert G.exact_fp32(A, W) and G.is_bf16(A) and G.is_bf16(W)
    assert np.array_equal(G.product(A, W), C) and (C == 2.0 ** (K // 64) - 1).all()
    assert G.is_bf16(C) if K // 64 <= 8 else G.is_fp32(C)    # K = 832 needs 13 bits: fp32 output there
    for fault in G.k_faults(K):
        bad = G.tiled_product(A, W, 5, fault)
        assert (bad != C).all(), fault                       # every output of every tile names the fault
    # the ring: the slot (kt - 1) % 3 never holds K-tile kt
    assert all(G.stale_tile(kt, K // 64) != kt for kt in range(K // 64))


@pytest.mark.parametrize("M,N,K", G.INT_SHAPES)
def test_int_case_is_exact_and_detects_every_fault(M, N, K):
    A, W = G.int_operands(M, N, K, 11)
    C = G.product(A, W)
    assert G.exact_fp32(A, W) and G.is_bf16(C) and np.abs(C).max() <= K
    for v in G.VARIANTS:
        for fault in G.k_faults(K) + G.geometry_faults(v):
            assert not np.array_equal(G.tiled_product(A, W, v, fault), C), (v, fault)


def test_stale_slot_model():
    assert [G.stale_tile(kt, 5) for kt in range(5)] == [2, 0, 1, 2, 3]
    assert G.stale_tile(0, 2) is None and G.stale_tile(0, 1) is None
    assert all((G.stale_tile(kt, 13) - (kt - 1)) % G.RING == 0 for kt in range(13))     # the same slot


def test_pack_gate_up_round_trip():
    g0 = np.random.default_rng(0)
    gate, up = g0.standard_normal((32, 64)), g0.standard_normal((32, 64))
    W = G.pack_gate_up(gate, up)
    assert np.array_equal(W[:16], gate[:16]) and np.array_equal(W[16:32], up[:16]) and np.array_equal(W[32:48], gate[16:])
    x = g0.standard_normal((5, 64))
    a, b = G.unpack_gate_up(x @ W.T)
    assert np.array_equal(a, x @ gate.T) and np.array_equal(b, x @ up.T)


@pytest.mark.parametrize("M,N,K", G.EPI_SHAPES)
def test_exact_epilogue_cases_are_exact_in_fp32(M, N, K):
    A, W = G.int_operands(M, N, K, 5)
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    assert G.exact_fp32(A, W) and G.is_bf16(bias) and G.is_bf16(res)
    assert np.array_equal(bias * 4, np.round(bias * 4)) and np.abs(bias).max() <= 1 and (bias < 0).any() and (bias > 0).any()
    acc = G.product(A, W)
    for epi in (G.EPI_NONE, G.EPI_RELU):
        for b, r in ((bias, None), (None, res), (bias, res)):
            # fp32 output: every intermediate is a multiple of 1/4 below 2^22 — nothing to round, the order cannot matter
            f = G.epilogue(acc, epi, True, b, r)
            assert G.is_fp32(f) and np.array_equal(f * 4, np.round(f * 4)) and np.abs(f).max() < 2.0 ** 20
            # 16-bit output: every fp32 step before a rounding point is exact, so the rounding points alone decide the bits
            h = G.epilogue(acc, epi, False, b, r)
            assert G.is_bf16(h)
            if epi == G.EPI_RELU and r is None:
                assert (h >= 0).all() and (h == 0).any()


def test_epilogue_rounding_points():
    acc = np.array([[256.0, 3.0, -300.0, 100.5]])
    bias = np.array([0.25, 0.25, 0.25, 0.25], np.float32)
    res = np.array([[1.0, 1.0, 1.0, 1.0]], np.float32)
    # 256.25 -> 256 (bf16 has 8 significant bits), then + 1 -> 257 -> 256 (ties to even); -299.75 -> -300, + 1 -> -299 -> -300
    assert G.epilogue(acc, G.EPI_NONE, False, bias, res).tolist() == [[256.0, 4.25, -300.0, 102.0]]
    assert G.epilogue(acc, G.EPI_NONE, True, bias, res).tolist() == [[257.25, 4.25, -298.75, 101.75]]
    assert G.epilogue(acc, G.EPI_RELU, False, bias, res).tolist() == [[256.0, 4.25, 1.0, 102.0]]
    assert G.epilogue(acc, G.EPI_NONE, False, None, None, row_scale=np.array([0.5])).tolist() == [[128.0, 1.5, -150.0, 50.25]]
    # SILU_MUL: gate | up in blocks of 16; silu(round(gate)) is rounded before the product
    a = np.zeros((1, 32))
    a[0, 0], a[0, 16] = 1.0, 3.0
    want = G.bf([1.0 / (1.0 + np.exp(-1.0))])[0] * 3.0
    out = G.epilogue(a, G.EPI_SILU_MUL)
    assert out.shape == (1, 16) and out[0, 0] == G.bf([want])[0] and not out[0, 1:].any()


@pytest.mark.parametrize("M,N,K", G.MAP_SHAPES)
def test_row_map_cases_are_exact(M, N, K):
    p = G.map_probe(M, N, K, G.MAP_A, G.MAP_C, True)
    assert G.exact_fp32(p.A[p.A[:, 0] != 3.0], p.W) and p.sumsq is not None
    stored = p.C[p.c_written]
    assert np.array_equal(stored * 4, np.round(stored * 4)) and np.abs(stored).max() < 64      # squares: multiples of 1/16 below 2^12
    assert G.is_fp32(p.sumsq) and not p.c_written.all()
    A, W = G.int_operands(M, N, K, 3)
    C = G.product(A, W)
    assert G.is_bf16(C) and np.abs(C).max() <= 256
    assert (C.reshape(M, -1, 64) ** 2).sum(axis=2).max() <= 2.0 ** 22                             # sums of 64 squares: exact in fp32


def test_bounds():
    A, W = np.ones((2, 64), np.float32), np.ones((3, 64), np.float32)
    assert np.allclose(G.fp32_sum_bound(A, W, np.full(3, 2.0)), 66 * 2.0 ** -24 * 66.0)
    ref = np.array([-2.0, 0.0])
    assert np.array_equal(G.act_bound(ref, G.EPI_GELU), np.abs(ref) * 2.0 ** -7 + 2e-2)
    assert np.array_equal(G.act_bound(ref, G.EPI_SILU_MUL), np.abs(ref) * 2.0 ** -7 + 1e-2)
