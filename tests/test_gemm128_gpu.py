"""Op tests of the four kernels behind gemm128_kernel on the MI355X — 2 = the double buffer, 5 / 6 / 7 = the loader-wave ring on the
128 x 128 / 128 x 64 / 128 x 256 tile — each requested per call (VSTAR_EPI_VARIANT) at the smallest shapes at which its mechanisms
are live: one to thirteen K-tiles through the three-slot ring, row edges around one 128-row tile, eleven row tiles, narrow outputs and
tails inside each tile width.  References, shapes and what each probe detects: tests/_gemm128_ref.py, pinned on the CPU by
tests/test_gemm128_ref.py.

Conventions of every test:
  * every case runs once per variant, and every call asserts vstar_op_gemm_last_tile() == 128 and vstar_op_gemm_last_mode() == variant;
  * C has two rows behind M and ldc > n_out, pre-filled with a sentinel NaN pattern: rows >= M and columns >= n_out must keep it;
  * EXACT = equal bits.  The two non-exact comparisons print one `GEMM128_ERR` line with the measured share of their bound
    (run with -s to record them).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _gemm128_ref as G
from tests import _prefill_ops_ref as R
from tests.test_prefill_ops_gpu import Gemm, as_f32, host16, pad_w, sent16, sent32, up16
from vstar_amd import _lib

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
variants = pytest.mark.parametrize("variant", G.VARIANTS)


class Operands:
    """The device copies of one case's inputs, uploaded once and shared by the four variants (never written)."""

    def __init__(self, cuda, A, W, bias=None, res=None):
        self.M, self.K = A.shape
        self.N = W.shape[0]
        self.A, self.W = up16(cuda, A), up16(cuda, pad_w(W))          # W: ceil(N / 256) * 256 rows, zero padded (library contract)
        self.bias = up16(cuda, bias)
        self.res = up16(cuda, res)


def run(lib, cuda, ops, variant, epi=G.EPI_NONE, f32=False, bias=True, res=True):
    """One vstar_op_gemm call on variant `variant` over a freshly sentinel-filled C -> the [M, n_out] bit patterns (uint32 for fp32
    output, uint16 else), after checking which kernel ran and that nothing outside [0, M) x [0, n_out) was written."""
    M, N, K = ops.M, ops.N, ops.K
    n_out = N // 2 if epi == G.EPI_SILU_MUL else N
    ldc = n_out + 8
    C = (sent32 if f32 else sent16)(cuda, M + 2, ldc)
    dres = ops.res if res else None
    rc = lib.vstar_op_gemm(None, P(ops.A), K, P(ops.W), P(ops.bias if bias else None), P(dres), n_out if dres is not None else 0, P(C), ldc,
                           1 if f32 else 0, M, N, K, epi | _lib.EPI_VARIANT(variant))
    assert rc == 0, lib.vstar_last_error(None)
    assert lib.vstar_op_gemm_last_tile() == 128 and lib.vstar_op_gemm_last_mode() == variant, \
        (lib.vstar_op_gemm_last_tile(), lib.vstar_op_gemm_last_mode(), variant)
    got = C.cpu().numpy().view(np.uint32) if f32 else host16(C)
    sent = R.SENT32 if f32 else R.SENT16
    assert (got[M:] == sent).all(), "a row behind the output was written"
    assert (got[:, n_out:] == sent).all(), "a column behind the output was written"
    return got[:M, :n_out]


def want_bits(C, f32):
    C = np.ascontiguousarray(np.asarray(C, np.float32))
    return C.view(np.uint32) if f32 else R.bits(C)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), "first (row, col):", bad[:6].tolist())


_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ================================================================ 1. index probe
@variants
@pytest.mark.parametrize("M,N,K", G.PROBE_SHAPES)
def test_index_probe(lib, cuda, M, N, K, variant):
    """One-hot rows at column (r * 37) % K: C[r, n] == W[n, (r * 37) % K] in bits, fp32 and bf16 output — every row, fragment, wave
    row and 64-column span lands where it belongs."""
    def build():
        p = G.index_probe(M, N, K)
        return Operands(cuda, p.A, p.W), p.C
    ops, C = cached(("probe", M, N, K), build)
    for f32 in (True, False):
        same(run(lib, cuda, ops, variant, f32=f32, bias=False, res=False), want_bits(C, f32), ("f32" if f32 else "bf16", variant))


# ================================================================ 2. every K-tile exactly once
@variants
@pytest.mark.parametrize("M,N,K", G.KTILE_SHAPES)
def test_every_k_tile_exactly_once(lib, cuda, M, N, K, variant):
    """K-tile kt adds 2^kt to every output: C == 2^(K / 64) - 1 everywhere, in bits (bf16 up to eight tiles, fp32 for thirteen)."""
    def build():
        A, W, C = G.ktile_probe(M, N, K)
        return Operands(cuda, A, W), C
    ops, C = cached(("ktile", M, N, K), build)
    for f32 in ((True, False) if K // 64 <= 8 else (True,)):
        got = run(lib, cuda, ops, variant, f32=f32, bias=False, res=False)
        bad = np.argwhere(got != want_bits(C, f32))
        if len(bad):
            r, c = bad[0]
            val = got.view(np.float32)[r, c] if f32 else as_f32(got)[r, c]
            pytest.fail(f"variant {variant}: {len(bad)} outputs, first at ({r}, {c}): {val} instead of {C[r, c]} — as a sum of 2^kt it "
                        f"names the K-tiles that entered")


@variants
@pytest.mark.parametrize("M,N,K", G.INT_SHAPES)
def test_int_operands_exact(lib, cuda, M, N, K, variant):
    """Random {-1, 0, 1} operands: the integer result in bits (every partial sum exact in any order)."""
    def build():
        A, W = G.int_operands(M, N, K, 11)
        return Operands(cuda, A, W), G.product(A, W)
    ops, C = cached(("int", M, N, K), build)
    for f32 in (True, False):
        same(run(lib, cuda, ops, variant, f32=f32, bias=False, res=False), want_bits(C, f32), ("f32" if f32 else "bf16", variant))


# ================================================================ 3. exact epilogues
@variants
@pytest.mark.parametrize("epi", [G.EPI_NONE, G.EPI_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("M,N,K", G.EPI_SHAPES)
def test_exact_epilogues(lib, cuda, M, N, K, epi, variant):
    """Integer operands, a bias of quarters, a residual (r + n) % 8, each with and without the other, bf16 and fp32 output: the bits
    of the reference's rounding points (acc + bias -> round; activation -> round; + residual -> round; fp32: nothing rounded)."""
    def build():
        A, W = G.int_operands(M, N, K, 5)
        return Operands(cuda, A, W, G.bias_quarters(N), G.residual_mod8(M, N)), G.product(A, W)
    ops, acc = cached(("epi", M, N, K), build)
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    for f32 in (True, False):
        for b, r in ((True, False), (False, True), (True, True)):
            want = cached(("epi_ref", M, N, K, epi, f32, b, r),
                          lambda: want_bits(G.epilogue(acc, epi, f32, bias if b else None, res if r else None), f32))
            same(run(lib, cuda, ops, variant, epi=epi, f32=f32, bias=b, res=r), want, (variant, epi, f32, b, r))


# ================================================================ 4. transcendental epilogues
@pytest.mark.parametrize("epi", [G.EPI_QUICK_GELU, G.EPI_GELU, G.EPI_SILU_MUL], ids=["quick_gelu", "gelu", "silu_mul"])
@pytest.mark.parametrize("M,N,K", G.ACT_SHAPES)
def test_transcendental_epilogues(lib, cuda, M, N, K, epi):
    """Random bf16 operands: the four variants agree bit for bit, and variant 2 stays within the bound tests/test_ops_gpu.py uses for
    these epilogues against the computation with exact sums: |ref| 2^-7 + 2e-2 (1e-2 for SILU_MUL)."""
    g0 = np.random.default_rng(M + N + K + epi)
    A = R.bf(g0.standard_normal((M, K)))
    if epi == G.EPI_SILU_MUL:
        F_ = G.SILU_N[N] // 2
        W = G.pack_gate_up(R.bf(g0.standard_normal((F_, K)) / np.sqrt(K)), R.bf(g0.standard_normal((F_, K)) / np.sqrt(K)))
        bias = res = None
    else:
        W = R.bf(g0.standard_normal((N, K)) / np.sqrt(K))
        bias, res = R.bf(g0.standard_normal(N)), R.bf(g0.standard_normal((M, N)))
    ops = Operands(cuda, A, W, bias, res)
    got = {v: run(lib, cuda, ops, v, epi=epi, bias=bias is not None, res=res is not None) for v in G.VARIANTS}
    for v in G.VARIANTS:
        same(got[v], got[2], f"variant {v} against variant 2")
    ref = G.epilogue(G.product(A, W), epi, False, bias, res)
    out = as_f32(got[2]).astype(np.float64)
    assert np.isfinite(out).all()
    err, gate = np.abs(out - ref), G.act_bound(ref, epi)
    print(f"GEMM128_ERR epilogue {epi} ({M},{W.shape[0]},{K}): abs {err.max():.3e}, worst err/bound {(err / gate).max():.3f}")
    assert (err <= gate).all(), float((err / gate).max())


# ================================================================ 5. random data, fp32 output, K = 832
@pytest.mark.parametrize("M,N,K", G.RANDOM_SHAPES)
def test_random_f32_variants_identical_and_bounded(lib, cuda, M, N, K):
    """Thirteen K-tiles of random data, three runs per variant (a misplaced counted wait shows as a rare wrong tile): all twelve
    outputs equal in bits, and each within (K + 2) 2^-24 (|A| |W|^T + |bias|) of the float64 product — K fp32 additions in any order."""
    g0 = np.random.default_rng(M + N)
    A, W, bias = R.bf(g0.standard_normal((M, K))), R.bf(g0.standard_normal((N, K)) / np.sqrt(K)), R.bf(g0.standard_normal(N))
    ops = Operands(cuda, A, W, bias)
    ref = G.product(A, W) + bias.astype(np.float64)[None, :]
    bound = G.fp32_sum_bound(A, W, bias)
    first = None
    for rep in range(3):
        for v in G.VARIANTS:
            got = run(lib, cuda, ops, v, f32=True, res=False)
            if first is None:
                first = got
            same(got, first, f"variant {v}, run {rep}, against variant 2's first run")
            if rep == 0:
                out = got.view(np.float32).astype(np.float64)
                assert np.isfinite(out).all()
                share = np.abs(out - ref) / bound
                print(f"GEMM128_ERR random f32 ({M},{N},{K}) variant {v}: max err/bound {share.max():.4f}")
                assert (share <= 1).all(), (v, float(share.max()))


# ================================================================ 6. row maps, row_scale, sumsq_out, stats_sum
@variants
@pytest.mark.parametrize("M,N,K", G.MAP_SHAPES)
def test_row_maps_scale_and_sumsq(lib, cuda, M, N, K, variant):
    """The scaled row-map probe through vstar_op_gemm_ex: row_scale by mapped A row, residual and sums of squares by mapped C row, all
    exact; gap rows of C and of the statistics keep their sentinels (checked by Gemm.output / Gemm.partials)."""
    p = cached(("map", M, N, K), lambda: G.map_probe(M, N, K, G.MAP_A, G.MAP_C, True))
    g = Gemm(lib, cuda, p.A, p.W, M, 128, am=G.MAP_A, cm=G.MAP_C, row_scale=p.row_scale, res=p.res, sumsq=True, variant=variant)
    same(g.output(), R.bits(p.C[g.cr]), variant)
    sq, _ = g.partials()
    assert np.array_equal(sq.astype(np.float64), p.sumsq[g.cr])


@variants
@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "c_map"])
@pytest.mark.parametrize("M,N,K", G.MAP_SHAPES)
def test_statistics_exact(lib, cuda, M, N, K, mapped, variant):
    """Integer-valued C: the sums of squares and the sums (stats_sum) of every 64-column span equal the float64 reference exactly,
    nothing else written."""
    A, W = G.int_operands(M, N, K, 3)
    C = G.product(A, W)
    g = Gemm(lib, cuda, A, W, M, 128, cm=G.MAP_C if mapped else R.IDENT, sumsq=True, stats=True, variant=variant)
    same(g.output(), R.bits(C.astype(np.float32)), variant)
    sm, sq = R.span_sums(C)
    got_sq, got_sm = g.partials()
    assert np.array_equal(got_sq.astype(np.float64), sq) and np.array_equal(got_sm.astype(np.float64), sm)


# ================================================================ 7. refusals
def test_refusals_launch_nothing(lib, cuda):
    """A variant next to a request only the 256 x 256 kernels serve, or a value that names no kernel: VSTAR_ERR_INVALID with a message
    that names the conflict, and the sentinel-filled C untouched.  The shape is inside the domain of both 256 x 256 kernels."""
    M, N, K = 1024, 256, 128
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=cuda)
    W = torch.zeros(N, K, dtype=torch.bfloat16, device=cuda)
    table = torch.zeros(1024, 128, dtype=torch.bfloat16, device=cuda)
    C = sent16(cuda, M + 2, N + 8)

    def gemm(flags):
        return lib.vstar_op_gemm(None, P(A), K, P(W), None, None, 0, P(C), N + 8, 0, M, N, K, flags)

    def gemm_norm(flags):
        return lib.vstar_op_gemm_norm(None, P(A), K, P(W), None, None, 0, P(C), N + 8, M, N, K, flags, None, None, 0)

    def gemm_ex(flags, **kw):
        g = R.gemm_ex(A=A.data_ptr(), W=W.data_ptr(), C=C.data_ptr(), M=M, N=N, K=K, lda=K, ldc=N + 8, a_rows=M, c_rows=M, w_rows=N,
                      epilogue=flags, **kw)
        return lib.vstar_op_gemm_ex(None, ctypes.byref(g))

    def refused(rc, fragment, what):
        assert rc == ERR_INVALID, what
        assert fragment in lib.vstar_last_error(None).decode(), (what, lib.vstar_last_error(None))

    for door in (gemm, gemm_norm, gemm_ex):
        for v in G.VARIANTS:
            refused(door(_lib.EPI_VARIANT(v) | _lib.EPI_TILE256), "VSTAR_EPI_VARIANT with VSTAR_EPI_TILE256", (door.__name__, v))
            refused(door(_lib.EPI_VARIANT(v) | _lib.EPI_TILE4W), "VSTAR_EPI_TILE4W", (door.__name__, v))
        for v in (1, 3, 4):
            refused(door(_lib.EPI_VARIANT(v)), "2, 5, 6 and 7", (door.__name__, v))
            refused(door(_lib.EPI_VARIANT(v) | _lib.EPI_TILE128), "2, 5, 6 and 7", (door.__name__, v))
    rope = dict(rope_cs=table.data_ptr(), rope_rows=512, rope_S=512, rope_cols=256)
    for v in G.VARIANTS:
        refused(gemm_ex(_lib.EPI_VARIANT(v), **rope), "rope_cs with VSTAR_EPI_VARIANT", v)
    torch.cuda.synchronize()
    assert (host16(C) == R.SENT16).all()
    # the same fused-RoPE request without the variant is served (by a 256 x 256 kernel): the refusals above were about the variant
    assert gemm_ex(0, **rope) == 0, lib.vstar_last_error(None)
    assert lib.vstar_op_gemm_last_tile() in (256, _lib.TILE_4W) and lib.vstar_op_gemm_last_mode() == 0


# ================================================================ 8. the dispatcher's answer is the one that runs
def _find(lib, code, cus, M, K):
    """The narrowest N (a multiple of 128) the plan sends to `code` on `cus` compute units."""
    for N in range(128, 16384 + 1, 128):
        if lib.vstar_op_gemm_plan(M, N, K, 0, 0, 0, cus) == code:
            return N
    raise AssertionError(f"no N <= 16384 is planned as {code} at M = {M}, K = {K} on {cus} CUs")


@functools.lru_cache(None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


F32_OUT_SHAPES = [(128, 128, 64), (256, 384, 128), (200, 130, 192), (1, 514, 768), (777, 1024, 640), (4096, 4096, 1024), (37, 4, 768)]


@pytest.mark.parametrize("shape", F32_OUT_SHAPES + ["ring_128x128", "ring_128x256", "split"], ids=str)
def test_plan_is_what_runs(lib, cuda, shape):
    """After an unforced vstar_op_gemm, last_tile * 10 + last_mode equals vstar_op_gemm_plan at the device's CU count: the host-side
    dispatch table (tests/test_dispatch.py) describes real launches.  Two shapes are searched so that the plan sends them to the
    128 x 128 and the 128 x 256 loader-wave tile on this device, a third is the smallest M (step 128) the plan splits at N = 1024,
    K = 128: one full round of 256^2 tiles plus a remainder — 16512 rows on 256 CUs."""
    cus = _cus()
    if shape == "ring_128x128":
        M, K = 1000, 256
        M, N, K = M, _find(lib, 1285, cus, M, K), K
    elif shape == "ring_128x256":
        M, K = 640, 2048
        M, N, K = M, _find(lib, 1287, cus, M, K), K
    elif shape == "split":
        N, K = 1024, 128
        M = next(M for M in range(128, 1 << 16, 128) if lib.vstar_op_gemm_plan(M, N, K, 0, 0, 0, cus) // 10 == 384)
    else:
        M, N, K = shape
    plan = lib.vstar_op_gemm_plan(M, N, K, 0, 0, 0, cus)
    assert plan > 0
    if isinstance(shape, str):
        assert plan == {"ring_128x128": 1285, "ring_128x256": 1287, "split": 3842}[shape]
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).bfloat16().to(cuda)
    w = torch.zeros((N + 255) // 256 * 256, K, dtype=torch.bfloat16, device=cuda)
    w[:N] = (torch.randn(N, K, generator=g) / np.sqrt(K)).bfloat16().to(cuda)
    c = sent16(cuda, M + 2, N + 8)
    assert lib.vstar_op_gemm(None, P(a), K, P(w), None, None, 0, P(c), N + 8, 0, M, N, K, 0) == 0, lib.vstar_last_error(None)
    ran = lib.vstar_op_gemm_last_tile() * 10 + lib.vstar_op_gemm_last_mode()
    assert ran == plan, (ran, plan)
    got = host16(c)
    assert (got[M:] == R.SENT16).all() and (got[:, N:] == R.SENT16).all() and np.isfinite(as_f32(got[:M, :N])).all()
