"""CPU pins of tests/_f16_prefill_ref.py (no GPU): a restatement of each kernel's documented rounding points stays inside the derived
gate for every case tests/test_f16_prefill_gpu.py runs, the preconditions of the fp16 overflow-window case hold, and the input
builders have the properties the gates lean on."""
import math

import numpy as np
import pytest
import torch

from tests import _f16_prefill_ref as R
from tests import _small_ops_ref as S
from vstar_amd import _lib

F16, F32, F64 = np.float16, np.float32, np.float64


def inside(got, ref, gate):
    got = np.asarray(got, F64)
    assert np.isfinite(got).all()
    share = np.abs(got - np.asarray(ref, F64)) / np.asarray(gate, F64)
    assert (share <= 1.0).all(), float(share.max())
    return float(share.max())


def test_doors_are_declared():
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.__file__), "..", "include", "vstar_vqa.h")).read()
    for sym in ("vstar_vqa_op_attention", "vstar_vqa_op_layernorm", "vstar_vqa_op_rmsnorm", "vstar_vqa_op_add_bcast",
                "vstar_vqa_op_vit_assemble_tokens"):
        assert sym in _lib.EXPORTS_VQA and sym + "(" in header


def test_the_case_lists_are_the_bf16_tests_lists():
    from tests import test_small_ops_gpu as T
    assert R.NORM_SHAPES == T.NORM_SHAPES and R.LAYOUT_SHAPES == T.LAYOUT_SHAPES
    x16, idx16, g16, b16 = R.norm_inputs(7, 72, 3)
    xb, idxb, gb, bb = T._norm_inputs(7, 72, 3)
    assert torch.equal(idx16, idxb)                                   # the same draws, stored as fp16
    assert (x16.float() - xb.float()).abs().max() <= 2.0 ** -8 * 60 and (g16.float() - gb.float()).abs().max() <= 2.0 ** -8 * 2


def test_ulp_and_tie_slack():
    assert R.ulp16(1.0) == 2.0 ** -10 and R.ulp16(1.999) == 2.0 ** -10 and R.ulp16(2.0) == 2.0 ** -9 and R.ulp16(0.0) == 2.0 ** -24
    mid = 1.0 + 2.0 ** -11                                            # the tie between 1 and 1 + 2^-10
    assert R.tie_slack(mid + 1e-6, 2e-6) == 2.0 ** -10 and R.tie_slack(mid - 1e-6, 2e-6) == 2.0 ** -10
    assert R.tie_slack(mid + 1e-5, 2e-6) == 0 and R.tie_slack(1.0, 2e-6) == 0
    t = torch.tensor([0.1, 1.0 + 2.0 ** -11 + 2.0 ** -20, 60000.0, -3.3], dtype=torch.float32)
    assert torch.equal(S.rf16(t), t.half().double())                  # fp32 values: torch's one-step conversion agrees
    # ONE rounding from float64: 1 + 2^-11 + 2^-30 is above the tie, but float32 would land on it first (and then round to even)
    assert S.rf16(torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)).item() == 1.0 + 2.0 ** -10


# ---------------------------------------------------------------- attention
@pytest.mark.parametrize("B,S_,H,D,causal", R.ATTN_SHAPES)
def test_attention_restated_inside_gate(B, S_, H, D, causal):
    qkv = R.random_qkv(B, S_, H, D, S_ + D)
    cases = [qkv] + ([R.spiked(qkv, B, S_, H, D)] if S_ >= 64 else [])
    for x in cases:
        ref, gate = R.attention_ref(x, B, S_, H, D, causal)
        inside(R.attn2_restated(x, B, S_, H, D, causal), ref, gate)


@pytest.mark.parametrize("S_,H,D,causal", R.RANGE_SHAPES)
@pytest.mark.parametrize("profile", R.RANGE_PROFILES)
def test_attention_dynamic_range_restated_inside_gate(S_, H, D, causal, profile):
    x = R.range_qkv(S_, H, D, profile)
    assert np.isfinite(x.astype(F64)).all()
    ref, gate = R.attention_ref(x, 1, S_, H, D, causal)
    inside(R.attn2_restated(x, 1, S_, H, D, causal), ref, gate)


@pytest.mark.parametrize("D,causal", R.WINDOW_SHAPES)
def test_window_preconditions(D, causal):
    """The spike's probability against the stale maximum 0 is at most 65536 — no lane's partial row sum exceeds the bf16 build's
    threshold — and rounds to +inf in fp16; 1e-4 to either edge of the window; every other probability is exactly 1 or exactly 0."""
    k0, k1 = R.window_spike_key(D)
    s, q0, q1 = R.window_score(D, k0, k1)
    assert s.dtype == F32
    assert math.log2(65520.0) + 1e-4 <= float(s) <= 16.0 - 1e-4
    exact = F64(q0) * F64(k0) + F64(q1) * F64(k1)                      # the products are exact in fp32; the sum rounds once
    assert abs(float(s) - exact) <= 2.0 ** -20
    p = np.exp2(s)
    with np.errstate(over="ignore"):
        assert np.isinf(R.h(p))
    assert p + F32(0) <= F32(65536.0) and p > F32(R.BIG_F16)
    assert q0 == float(R.prescaled_q(np.array([math.sqrt(D)], F32).astype(F16), D)[0])
    other = F32(q0) * F32(-20.0)
    assert R.h(np.exp2(other)) == 0 and R.h(np.exp2(other)) * 16 + p <= F32(65536.0)
    for spike_at in R.WINDOW_SPIKES:
        x = R.window_qkv(D, spike_at).reshape(R.WINDOW_S, 3, R.WINDOW_H, D)
        assert not x[:32, 1].any() and (x[32:, 1, :, 0] == -20).sum() == (R.WINDOW_S - 33) * R.WINDOW_H
        assert (x[spike_at, 1, :, 0] == k0).all() and (x[spike_at, 1, :, 1] == k1).all() and not x[:, 1, :, 2:].any()
    assert R.WINDOW_SPIKES == (40, 100) and 40 // 64 == 0 and 40 // 32 == 1 and 100 // 64 == 1      # tile 0's second sub-tile; tile 1


@pytest.mark.parametrize("D,causal", R.WINDOW_SHAPES)
@pytest.mark.parametrize("spike_at", R.WINDOW_SPIKES)
def test_window_restated(D, causal, spike_at):
    """With the fp16 threshold the restatement is finite and inside the gate; with the bf16 build's 65536 it reproduces the defect:
    the rows that see the spike come out non-finite."""
    x = R.window_qkv(D, spike_at)
    ref, gate = R.attention_ref(x, 1, R.WINDOW_S, R.WINDOW_H, D, causal)
    inside(R.attn2_restated(x, 1, R.WINDOW_S, R.WINDOW_H, D, causal, big=R.BIG_F16), ref, gate)
    bad = R.attn2_restated(x, 1, R.WINDOW_S, R.WINDOW_H, D, causal, big=R.BIG_BF16).astype(F64)
    sees = np.arange(R.WINDOW_S) >= (spike_at if causal else 0)
    assert not np.isfinite(bad[sees]).all(axis=1).any() and np.isfinite(bad[~sees]).all()
    # rows that see the spike are ~ V[spike]; causal rows below it are the plain average of their visible V rows
    v = x.reshape(R.WINDOW_S, 3, R.WINDOW_H, D)[:, 2].astype(F64)
    assert np.abs(ref.reshape(R.WINDOW_S, R.WINDOW_H, D)[sees] - v[spike_at]).max() < 2e-3
    if causal:
        r = spike_at - 1
        assert np.allclose(ref.reshape(R.WINDOW_S, R.WINDOW_H, D)[r], v[:32].mean(axis=0), atol=1e-6)


# ---------------------------------------------------------------- norms
def _norm_fp32(x, gam, bet, eps, idx, act, rms):
    """norm_kernel's arithmetic in torch float32 (another summation order than the kernel's)."""
    xs = x.float()[idx.long()]
    cols = xs.shape[-1]
    if rms:
        rstd = torch.rsqrt((xs * xs).sum(-1, keepdim=True) / cols + eps)
        return (gam.float() * (xs * rstd).half().float()).half()
    mean = xs.sum(-1, keepdim=True) / cols
    d = xs - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / cols + eps)
    r = d * rstd * gam.float() + (bet.float() if bet is not None else 0.0)
    if act == 1:
        t = r.half().float()
        r = 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752))
    return r.half()


@pytest.mark.parametrize("rows,cols", R.NORM_SHAPES)
def test_norms_restated_inside_gate(rows, cols):
    for act, use_beta in R.NORM_VARIANTS:
        x, idx, gam, bet = R.norm_inputs(rows, cols, rows * 31 + cols + act)
        b = bet if use_beta else None
        ref, gate = R.layernorm_ref(x, gam, b, 1e-6, idx, act)
        inside(_norm_fp32(x, gam, b, 1e-6, idx, act, False).double().numpy(), ref.numpy(), gate.numpy())
        assert float((gate - 2.0 ** -10 * ref.abs()).max()) < 1e-2 / 2       # the absolute part: well under the bf16 tests' scalar
    x, idx, gam, _ = R.norm_inputs(rows, cols, rows * 17 + cols)
    ref, gate = R.rmsnorm_ref(x, gam, 1e-6, idx)
    inside(_norm_fp32(x, gam, None, 1e-6, idx, 0, True).double().numpy(), ref.numpy(), gate.numpy())
    assert float(((gate - 2.0 ** -10 * ref.abs()) > 0).double().mean()) < 0.01  # the tie slack applies to under 1 % of the elements


def test_layout_refs_round_once():
    a, b = R.f16_mid_codes(577 * 72, 1).view(577, 72), R.f16_mid_codes(5 * 72, 2).view(5, 72)
    assert len(set(a.view(torch.int16).flatten().tolist())) == min(a.numel(), 16 * 2048)
    want = (a.numpy().astype(F32) + np.tile(b.numpy(), (116, 1))[:577].astype(F32)).astype(F16)
    assert np.array_equal(R.bits(R.add_bcast(a, b).numpy()), R.bits(want))
    assert np.isfinite(want.astype(F64)).all()
    patch, cls, pos = R.f16_mid_codes(3 * 4 * 72, 1).view(3, 4, 72), R.f16_mid_codes(72, 2), R.f16_mid_codes(5 * 72, 3).view(5, 72)
    tok = R.vit_assemble_tokens(patch, cls, pos)
    assert torch.equal(tok[1, 0], (cls.float() + pos[0].float()).half()) and torch.equal(tok[2, 3], (patch[2, 2].float() + pos[3].float()).half())


# ---------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K,kernel", R.GEMM_CASES)
@pytest.mark.parametrize("epi", [R.EPI_NONE, R.EPI_SILU_MUL])
def test_gemm_inputs_have_exact_accumulators(M, N, K, kernel, epi):
    A, W, bias, res = R.gemm_inputs(M, N, K, epi, "exact")
    assert M > 64 and K % 64 == 0 and W.shape[0] % 256 == 0 and not W[N:].any()
    a64 = A.astype(F64) @ W.astype(F64).T
    assert np.array_equal(a64 * 64, np.round(a64 * 64)) and np.abs(a64).max() + 2 < 2.0 ** 24 / 64
    a32 = (A.astype(F32)[:, ::-1] @ W.astype(F32).T[::-1]).astype(F64)          # fp32, another order
    assert np.array_equal(a32, a64)
    assert np.abs(a64).max() > 16                                                # h(acc) does round somewhere
    ref, gate = R.gemm_ref(A, W, bias, res, N, epi)
    assert ref.shape == (M, N // 2 if epi == R.EPI_SILU_MUL else N) and (gate >= 0).all() and np.isfinite(ref).all()
    if epi == R.EPI_SILU_MUL:
        # the fp32 epilogue restated with an exact sigmoid lands inside the gate
        c = np.arange(N // 2)
        g = a32[:, (c // 16) * 32 + c % 16].astype(F16).astype(F32)
        u = a32[:, (c // 16) * 32 + 16 + c % 16].astype(F16).astype(F32)
        got = ((g / (F32(1) + np.exp(-g))).astype(F16).astype(F32) * u).astype(F16)
        ok = gate > 0
        inside(got.astype(F64)[ok], ref[ok], gate[ok])
        assert not got[~ok].astype(F64).any() and not ref[~ok].any()
    else:
        got = ((a32[:, :N].astype(F32) + bias[:N].astype(F32)).astype(F16).astype(F32) + res.astype(F32)).astype(F16)
        ok = gate > 0
        inside(got.astype(F64)[ok], ref[ok], gate[ok])


@pytest.mark.parametrize("M,N,K,kernel", R.GEMM_CASES[:2])
@pytest.mark.parametrize("epi", [R.EPI_NONE, R.EPI_SILU_MUL])
def test_gemm_random_operands_restated_inside_gate(M, N, K, kernel, epi):
    """The fp32 epilogue on an fp32 accumulator (numpy's summation order) lands inside the gate with the tie slack; the slack applies
    to a few per cent of the elements at most and is what separates this gate from the exact-operand one."""
    A, W, bias, res = R.gemm_inputs(M, N, K, epi, "random")
    a32 = A.astype(F32) @ W.astype(F32).T
    ref, gate = R.gemm_ref(A, W, bias, res, N, epi, acc_err=True)
    plain = R.gemm_ref(A, W, bias, res, N, epi)[1]
    assert ((gate - plain) > 2.0 ** -24).mean() < 0.08
    if epi == R.EPI_SILU_MUL:
        c = np.arange(N // 2)
        g = a32[:, (c // 16) * 32 + c % 16].astype(F16).astype(F32)
        u = a32[:, (c // 16) * 32 + 16 + c % 16].astype(F16).astype(F32)
        got = ((g / (F32(1) + np.exp(-g))).astype(F16).astype(F32) * u).astype(F16)
    else:
        got = ((a32[:, :N] + bias[:N].astype(F32)).astype(F16).astype(F32) + res.astype(F32)).astype(F16)
    inside(got.astype(F64), ref, gate)
