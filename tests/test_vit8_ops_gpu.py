"""Operator-level tests of what VSMConfig.vit_w8a8 adds below the engine (MI355X): the LayerNorm that emits quantised rows
(vstar_op_layernorm_quant_fp8, quant.hip) and the quick-GELU epilogue on the two W8A8 256 x 256 kernels (vstar_op_gemm_fp8 with
epilogue 1), plus the tower shapes of the epilogue those kernels already had (bias + residual).

Gates:
  * layernorm_quant: EXACT bytes and scales against vstar_op_layernorm -> vstar_op_quantize_rows_fp8 (the kernel's contract), and the
    decoded row against torch's fp32 LayerNorm within (2^-4 + 2^-7) |ref| + 2^-10 scale: half an e4m3 step over the normal range (three
    mantissa bits) plus the 16-bit rounding of the LayerNorm output, and half a subnormal step below it — e4m3 subnormals are 2^-9
    apart in CODE units, the decode is code x scale, so half a step is 2^-10 scale in value units;
  * quick-GELU GEMM: torch on the SAME quantised operands (the fake-quant model of tests/test_ops_gpu.py::test_gemm_w8a8_fp8), every
    element within 2^-6 |ref| + 2e-2 (the quick-GELU gate of test_gemm256_bench_shapes), no outliers;
  * the 4-wave kernel against the 8-wave one wherever both take a shape: bit-identical, three launches."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _small_ops_ref as R
from vstar_amd import _lib

pytestmark = pytest.mark.gpu

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
SENT = 0xAB


def _ln_quant(lib, cuda, x, gam, beta, eps):
    """(bytes, scales) of the fused kernel and of the two-kernel chain it must equal; outputs carry a sentinel row behind them."""
    rows, cols = x.shape
    xd, gd, bd = x.to(cuda), gam.to(cuda), beta.to(cuda)
    q = torch.full((rows + 1, cols), SENT, dtype=torch.uint8, device=cuda)
    sc = torch.full((rows + 1,), float("nan"), dtype=torch.float32, device=cuda)
    rc = lib.vstar_op_layernorm_quant_fp8(None, P(xd), P(gd), P(bd), P(q), P(sc), rows, cols, eps)
    assert rc == 0, lib.vstar_last_error(None)
    y = torch.empty_like(xd)
    assert lib.vstar_op_layernorm(None, P(xd), P(gd), P(bd), P(y), rows, cols, eps) == 0, lib.vstar_last_error(None)
    q2 = torch.empty(rows, cols, dtype=torch.uint8, device=cuda)
    s2 = torch.empty(rows, dtype=torch.float32, device=cuda)
    assert lib.vstar_op_quantize_rows_fp8(None, P(y), cols, P(q2), cols, P(s2), rows, cols) == 0, lib.vstar_last_error(None)
    qc, scc = q.cpu(), sc.cpu()
    assert (qc[rows] == SENT).all() and torch.isnan(scc[rows]), "the kernel wrote past its last row"
    return qc[:rows], scc[:rows], q2.cpu(), s2.cpu()


@pytest.mark.parametrize("cols", [256, 264, 768, 1024, 4096])
@pytest.mark.parametrize("rows", [1, 5, 1028])
def test_layernorm_quant_fp8_equals_layernorm_then_quantize(lib, cuda, rows, cols):
    eps = 1e-5
    g = torch.Generator().manual_seed(rows * 10000 + cols)
    x = (0.3 + 2 * torch.randn(rows, cols, generator=g)).bfloat16()
    if rows > 1:
        x[1, cols // 3] = (x[1].float().abs().max() * 100).bfloat16()       # one x100 outlier channel: the rest of the row sits low in the code range
    gam = (1 + 0.1 * torch.randn(cols, generator=g)).bfloat16()
    beta = (0.2 * torch.randn(cols, generator=g)).bfloat16()
    got_q, got_s, want_q, want_s = _ln_quant(lib, cuda, x, gam, beta, eps)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32))
    assert torch.equal(got_q, want_q), f"{(got_q != want_q).sum().item()} of {want_q.numel()} bytes differ"
    ref = F.layer_norm(x.float(), (cols,), gam.float(), beta.float(), eps).double()
    deq = R.fp8_decode(got_q).double() * got_s.double()[:, None]
    lim = ref.abs() * (2 ** -4 + 2 ** -7) + got_s.double()[:, None] * 2 ** -10
    over = (deq - ref).abs() - lim
    print(f"layernorm_quant rows {rows} cols {cols}: worst |err| - gate {over.max().item():.3e}")
    assert (over <= 0).all(), int((over > 0).sum())
    # beta = 0 and a constant row: LayerNorm gives exactly zero, the quantiser takes its scale = 1 branch
    xc = x.clone()
    xc[rows // 2] = -0.75
    zero = torch.zeros(cols, dtype=torch.bfloat16)
    got_q, got_s, want_q, want_s = _ln_quant(lib, cuda, xc, gam, zero, eps)
    assert torch.equal(got_s.view(torch.int32), want_s.view(torch.int32)) and torch.equal(got_q, want_q)
    assert got_s[rows // 2] == 1.0 and (got_q[rows // 2] == 0).all()


@pytest.mark.parametrize("cols", [4104, 260])
def test_layernorm_quant_fp8_refuses_rows_it_cannot_hold(lib, cuda, cols):
    """More than 4096 columns (one wave holds a row in registers) or a width that is no multiple of 8: refused, nothing launched."""
    x = torch.ones(5, cols, dtype=torch.bfloat16, device=cuda)
    q = torch.full((5, cols), SENT, dtype=torch.uint8, device=cuda)
    s = torch.full((5,), 7.0, dtype=torch.float32, device=cuda)
    assert lib.vstar_op_layernorm_quant_fp8(None, P(x), P(x[0]), P(x[0]), P(q), P(s), 5, cols, 1e-5) != 0
    torch.cuda.synchronize()
    assert (q == SENT).all() and (s == 7.0).all()


# ---------------------------------------------------------------- the W8A8 GEMMs at tower shapes
_CASES = {}


def _case(M, N, K, epi):
    """Operands and the fake-quant reference of one shape, computed once (CPU, fp32) and shared by the tests that use the shape."""
    key = (M, N, K, epi)
    if key not in _CASES:
        g = torch.Generator().manual_seed(M + N + K + epi)
        A = (torch.randn(M, K, generator=g) * (0.2 + 3 * torch.rand(M, 1, generator=g))).bfloat16()
        W = (torch.randn(N, K, generator=g) / math.sqrt(K) * (0.5 + torch.rand(N, 1, generator=g))).bfloat16()
        bias = (torch.randn(N, generator=g) * 0.5).bfloat16()
        res = (torch.randn(M, N, generator=g) * 0.5).bfloat16() if epi == _lib.EPI_NONE else None

        def fq(x):
            s = x.float().abs().amax(dim=1, keepdim=True) / 448.0
            s = torch.where(s > 0, s, torch.ones_like(s))
            return (x.float() * (1.0 / s)).to(torch.float8_e4m3fn).float(), s
        aq, sa = fq(A)
        wq, sw = fq(W)
        t = ((aq @ wq.T) * sa * sw.T + bias.float()).bfloat16().float()
        if epi == _lib.EPI_QUICK_GELU:
            ref = t * torch.sigmoid(1.702 * t)
        else:
            ref = t + res.float()
        _CASES[key] = (A, W, bias, res, ref)
    return _CASES[key]


def _run(lib, cuda, case, M, N, K, epi):
    A, W, bias, res, _ = case
    dA, dW, dB = A.to(cuda), W.to(cuda), bias.to(cuda)
    dR = res.to(cuda) if res is not None else None
    C = torch.full((M + 1, N), float("nan"), dtype=torch.bfloat16, device=cuda)
    rc = lib.vstar_op_gemm_fp8(None, P(dA), P(dW), P(dB), P(dR), P(C), M, N, K, epi, 0, None)
    assert rc == 0, lib.vstar_last_error(None)
    torch.cuda.synchronize()
    tile = lib.vstar_op_gemm_last_tile()
    out = C.cpu()
    assert torch.isnan(out[M].float()).all(), "the kernel wrote past row M - 1"
    return out[:M], tile


def _gate(got, ref, what):
    assert not torch.isnan(got.float()).any(), what
    err = (got.float() - ref).abs()
    tol = ref.abs() * 2 ** -6 + 2e-2
    print(f"{what}: worst |err| / gate {(err / tol).max().item():.3f}")
    bad = int((err > tol).sum())
    assert bad == 0, (what, bad, float(err.max()))


GELU_SHAPES = [(1028, 768, 256),        # ragged last row tile, one pair of K-tiles: the K loop runs zero times
               (1028, 3072, 768),       # three pairs of K-tiles (odd)
               (1300, 1024, 4096),      # ragged AND inside the 4-wave kernel's domain (K >= 4096)
               (2304, 1024, 1024)]      # whole tiles only


@pytest.mark.parametrize("M,N,K", GELU_SHAPES)
def test_gemm_fp8_quick_gelu(lib, cuda, M, N, K):
    """epilogue 1 with bias, as the dispatcher routes it, and forced onto the 8-wave kernel."""
    case = _case(M, N, K, _lib.EPI_QUICK_GELU)
    got, tile = _run(lib, cuda, case, M, N, K, _lib.EPI_QUICK_GELU)
    both = M % 256 == 0 or K >= 4096
    assert tile == (_lib.TILE_4W if both else 256)
    _gate(got, case[4], f"fp8 quick-GELU {M}x{N}x{K} (tile {tile})")
    got256, tile = _run(lib, cuda, case, M, N, K, _lib.EPI_QUICK_GELU | _lib.EPI_TILE256)
    assert tile == 256
    _gate(got256, case[4], f"fp8 quick-GELU {M}x{N}x{K} (8-wave kernel)")


@pytest.mark.parametrize("M,N,K", [(2305, 768, 768), (2305, 768, 3072)])
def test_gemm_fp8_bias_residual_owl_shapes(lib, cuda, M, N, K):
    """out_proj / fc2 of one OWL-ViT crop (2305 rows: a ragged tile of one row): epilogue 0 with bias and residual."""
    case = _case(M, N, K, _lib.EPI_NONE)
    got, tile = _run(lib, cuda, case, M, N, K, _lib.EPI_NONE)
    assert tile == 256
    assert not torch.isnan(got.float()).any()
    err = (got.float() - case[4]).abs()
    tol = case[4].abs() * 2 ** -7 + 2e-2      # one bf16 step: the plain-epilogue gate of test_gemm256_bench_shapes
    print(f"fp8 bias + residual {M}x{N}x{K}: worst |err| / gate {(err / tol).max().item():.3f}")
    assert int((err > tol).sum()) == 0, float(err.max())


@pytest.mark.parametrize("M,N,K", [(1300, 1024, 4096), (2304, 1024, 1024)])
def test_gemm4w_fp8_quick_gelu_equals_gemm256(lib, cuda, M, N, K):
    """Same K order per MFMA, same dequantisation, same epilogue: the 4-wave instantiation is bit-identical to the 8-wave one."""
    case = _case(M, N, K, _lib.EPI_QUICK_GELU)
    want, tile = _run(lib, cuda, case, M, N, K, _lib.EPI_QUICK_GELU | _lib.EPI_TILE256)
    assert tile == 256 and not torch.isnan(want.float()).any()
    for rep in range(3):
        got, tile = _run(lib, cuda, case, M, N, K, _lib.EPI_QUICK_GELU | _lib.EPI_TILE4W)
        assert tile == _lib.TILE_4W
        bad = int((got.view(torch.int16) != want.view(torch.int16)).sum())
        assert bad == 0, (rep, bad)


def test_gemm_fp8_still_refuses_epilogues_it_does_not_have(lib, cuda):
    a = torch.randn(1024, 256, device=cuda).bfloat16()
    w = torch.randn(256, 256, device=cuda).bfloat16()
    c = torch.empty(1024, 256, device=cuda, dtype=torch.bfloat16)
    for epi in (_lib.EPI_GELU, _lib.EPI_RELU):
        assert lib.vstar_op_gemm_fp8(None, P(a), P(w), None, None, P(c), 1024, 256, 256, epi, 0, None) != 0
