"""Operator-level tests of the fp16 PREFILL kernels on the MI355X — the -DVSTAR_LP_F16 build of attn2_kernel, layernorm_lp,
rmsnorm_lp, add_bcast and vit_assemble_tokens that every VQA prefill, the fp16 CLIP tower and the Perceiver run, and the tile GEMMs
above the weight-streaming domain — each driven alone through its vstar_vqa_op_* door against tests/_f16_prefill_ref.py (pinned on
the CPU by tests/test_f16_prefill_ref.py, which also holds a restatement of every kernel's rounding points to the same gates).

Conventions of every test:
  * outputs are allocated with two sentinel rows behind them (fp16 NaN) that must come back bit-unchanged (`Out`);
  * EXACT = equal bits.  Everything else is |got - ref| <= gate with the gate DERIVED in _f16_prefill_ref.py from u = 2^-11 and the
    kernel's rounding points; each such test prints one `F16OP_ERR` line with the measured error and its share of the gate (run
    with -s to record them).

test_attention_overflow_window is the case the bf16 suite cannot see: a probability in [65520, 65536] against the stale running
maximum stayed on the fast path of the bf16 build's re-centre threshold (65536) and rounded to +inf in fp16.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _f16_prefill_ref as R

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
NAN = float("nan")
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
HP = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731


def ok(lib, rc):
    assert rc == 0, lib.vstar_vqa_last_error(None)


def refused(lib, rc, out=None):
    assert rc == ERR_INVALID, rc
    assert lib.vstar_vqa_last_error(None)
    if out is not None:
        out.untouched()


def dev(cuda, a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(cuda)


class Out:
    """An fp16 output [rows + 2, cols] filled with NaN; the two rows behind the payload must come back bit-unchanged."""

    def __init__(self, cuda, rows, cols):
        self.full = torch.full((rows + 2, cols), NAN, dtype=torch.float16, device=cuda)
        self.before = self.full.cpu().numpy().copy()
        self.rows = rows

    def get(self):
        got = self.full.cpu().numpy()
        assert np.array_equal(R.bits(got[self.rows:]), R.bits(self.before[self.rows:])), "the kernel wrote behind its output"
        return got[: self.rows]

    def untouched(self):
        assert np.array_equal(R.bits(self.full.cpu().numpy()), R.bits(self.before)), "a refused call wrote to its output"


def gate_check(name, got, ref, gate):
    """|got - ref| <= gate elementwise, finite; prints the recorded-error line first."""
    got, ref, gate = (np.asarray(a.numpy() if isinstance(a, torch.Tensor) else a, np.float64) for a in (got, ref, gate))
    err = np.abs(got - ref)
    share = np.where(gate > 0, err / np.where(gate > 0, gate, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"F16OP_ERR {name}: abs {np.nanmax(err):.3e} rel {np.nanmax(err) / max(np.abs(ref).max(), 1e-30):.3e} "
          f"worst err/gate {np.nanmax(share):.3f} non-finite {int((~np.isfinite(got)).sum())}")
    assert np.isfinite(got).all(), f"{int((~np.isfinite(got)).sum())} non-finite outputs"
    assert (err <= gate).all(), float(share.max())


# ================================================================ attention
def run_attention(lib, cuda, qkv, B, S, H, D, causal):
    out = Out(cuda, B * S, H * D)
    x = dev(cuda, qkv)
    ok(lib, lib.vstar_vqa_op_attention(P(x), B * S, P(out.full), B * S + 2, B, S, H, D, causal))
    assert np.array_equal(R.bits(x.cpu().numpy()), R.bits(qkv))
    return out.get()


@pytest.mark.parametrize("B,S,H,D,causal", R.ATTN_SHAPES)
def test_attention_random(lib, cuda, B, S, H, D, causal):
    """Random unit-variance operands, then (S >= 64) the spiked-key variant of test_ops_gpu.py::test_attention."""
    qkv = R.random_qkv(B, S, H, D, S + D)
    ref, gate = R.attention_ref(qkv, B, S, H, D, causal)
    gate_check(f"attention B{B} S{S} H{H} D{D} c{causal}", run_attention(lib, cuda, qkv, B, S, H, D, causal), ref, gate)
    if S >= 64:
        x = R.spiked(qkv, B, S, H, D)
        ref, gate = R.attention_ref(x, B, S, H, D, causal)
        gate_check(f"attention spike B{B} S{S} H{H} D{D} c{causal}", run_attention(lib, cuda, x, B, S, H, D, causal), ref, gate)


@pytest.mark.parametrize("S,H,D,causal", R.RANGE_SHAPES)
@pytest.mark.parametrize("profile", R.RANGE_PROFILES)
def test_attention_dynamic_range(lib, cuda, S, H, D, causal, profile):
    """The four score profiles of test_ops_gpu.py::test_attention_softmax_dynamic_range in fp16: finite and inside the gate."""
    qkv = R.range_qkv(S, H, D, profile)
    ref, gate = R.attention_ref(qkv, 1, S, H, D, causal)
    gate_check(f"attention range S{S} D{D} c{causal} {profile}", run_attention(lib, cuda, qkv, 1, S, H, D, causal), ref, gate)


@pytest.mark.parametrize("D,causal", R.WINDOW_SHAPES)
@pytest.mark.parametrize("spike_at", R.WINDOW_SPIKES)
def test_attention_overflow_window(lib, cuda, D, causal, spike_at):
    """One key whose probability against the stale maximum 0 lies in [65520, 65536] (preconditions: test_f16_prefill_ref.py), in the
    second sub-tile of tile 0 (key 40) or in tile 1 (key 100): every row finite and inside the gate — rows that see the spike are
    ~ V[spike], causal rows below it the plain average of their visible V rows.
    Before the re-centre threshold depended on the storage type (65536 in both builds) every row that sees the spike came back NaN:
    all four cases failed, 160 / 160 rows non-finite in the two non-causal ones, 120 / 160 and 60 / 160 in the causal ones."""
    S, H = R.WINDOW_S, R.WINDOW_H
    qkv = R.window_qkv(D, spike_at)
    ref, gate = R.attention_ref(qkv, 1, S, H, D, causal)
    got = run_attention(lib, cuda, qkv, 1, S, H, D, causal)
    bad_rows = int((~np.isfinite(got.astype(np.float64))).any(axis=1).sum())
    print(f"F16OP_WINDOW D{D} c{causal} spike@{spike_at}: rows with a non-finite output {bad_rows} / {S}")
    gate_check(f"attention window D{D} c{causal} spike@{spike_at}", got, ref, gate)


# ================================================================ norms
@pytest.mark.parametrize("rows,cols", R.NORM_SHAPES)
@pytest.mark.parametrize("act,use_beta", R.NORM_VARIANTS)
def test_layernorm(lib, cuda, rows, cols, act, use_beta):
    """layernorm_lp with a row index; act 1: the reference rounds the affine result to fp16 before the exact-erf GELU."""
    x, idx, gam, bet = R.norm_inputs(rows, cols, rows * 31 + cols + act)
    bet = bet if use_beta else None
    out = Out(cuda, rows, cols)
    xd, gd, bd = dev(cuda, x), dev(cuda, gam), dev(cuda, bet) if use_beta else None
    hidx = np.ascontiguousarray(idx.numpy(), np.int32)
    ok(lib, lib.vstar_vqa_op_layernorm(P(xd), x.shape[0], P(gd), P(bd), P(out.full), rows, cols, 1e-6, HP(hidx), act))
    ref, gate = R.layernorm_ref(x, gam, bet, 1e-6, idx, act)
    gate_check(f"layernorm r{rows} c{cols} act{act} beta{int(use_beta)}", out.get(), ref, gate)


@pytest.mark.parametrize("rows,cols", R.NORM_SHAPES)
def test_rmsnorm(lib, cuda, rows, cols):
    """rmsnorm_lp with a row index: gamma * h(x * rstd)."""
    x, idx, gam, _ = R.norm_inputs(rows, cols, rows * 17 + cols)
    out = Out(cuda, rows, cols)
    xd, gd = dev(cuda, x), dev(cuda, gam)
    hidx = np.ascontiguousarray(idx.numpy(), np.int32)
    ok(lib, lib.vstar_vqa_op_rmsnorm(P(xd), x.shape[0], P(gd), P(out.full), rows, cols, 1e-6, HP(hidx)))
    ref, gate = R.rmsnorm_ref(x, gam, 1e-6, idx)
    gate_check(f"rmsnorm r{rows} c{cols}", out.get(), ref, gate)


def test_norms_without_a_row_index_read_row_by_row(lib, cuda):
    """EXACT against the same door with the identity index."""
    x, _, gam, bet = R.norm_inputs(7, 72, 99)
    xd, gd, bd = dev(cuda, x), dev(cuda, gam), dev(cuda, bet)
    ident = np.arange(7, dtype=np.int32)
    outs = [Out(cuda, 7, 72) for _ in range(4)]
    ok(lib, lib.vstar_vqa_op_layernorm(P(xd), x.shape[0], P(gd), P(bd), P(outs[0].full), 7, 72, 1e-5, None, 0))
    ok(lib, lib.vstar_vqa_op_layernorm(P(xd), x.shape[0], P(gd), P(bd), P(outs[1].full), 7, 72, 1e-5, HP(ident), 0))
    ok(lib, lib.vstar_vqa_op_rmsnorm(P(xd), x.shape[0], P(gd), P(outs[2].full), 7, 72, 1e-6, None))
    ok(lib, lib.vstar_vqa_op_rmsnorm(P(xd), x.shape[0], P(gd), P(outs[3].full), 7, 72, 1e-6, HP(ident)))
    got = [o.get() for o in outs]
    assert np.isfinite(got[0].astype(np.float64)).all() and np.isfinite(got[2].astype(np.float64)).all()
    assert np.array_equal(R.bits(got[0]), R.bits(got[1])) and np.array_equal(R.bits(got[2]), R.bits(got[3]))


# ================================================================ layout ops (EXACT)
@pytest.mark.parametrize("rows,cols,b_rows", R.ADD_BCAST_CASES)
def test_add_bcast(lib, cuda, rows, cols, b_rows):
    """EXACT: one fp32 add, one rounding; distinct fp16 codes."""
    a, b = R.f16_mid_codes(rows * cols, 1).view(rows, cols), R.f16_mid_codes(b_rows * cols, 2).view(b_rows, cols)
    out = Out(cuda, rows, cols)
    ad, bd = dev(cuda, a), dev(cuda, b)
    ok(lib, lib.vstar_vqa_op_add_bcast(P(ad), P(bd), P(out.full), rows, cols, b_rows))
    assert np.array_equal(R.bits(out.get()), R.bits(R.add_bcast(a, b).numpy()))


@pytest.mark.parametrize("B,Pn,C", R.ASSEMBLE_CASES)
def test_vit_assemble_tokens(lib, cuda, B, Pn, C):
    """EXACT, the class row of every batch included."""
    patch, cls, pos = R.f16_mid_codes(B * Pn * C, 1).view(B, Pn, C), R.f16_mid_codes(C, 2), R.f16_mid_codes((Pn + 1) * C, 3).view(Pn + 1, C)
    out = Out(cuda, B * (Pn + 1), C)
    pd, cd, sd = dev(cuda, patch), dev(cuda, cls), dev(cuda, pos)
    ok(lib, lib.vstar_vqa_op_vit_assemble_tokens(P(pd), P(cd), P(sd), P(out.full), B, Pn, C))
    assert np.array_equal(R.bits(out.get()), R.bits(R.vit_assemble_tokens(patch, cls, pos).view(-1, C).numpy()))


# ================================================================ fp16 tile GEMM above the weight-streaming domain
@pytest.mark.parametrize("M,N,K,kernel", R.GEMM_CASES)
@pytest.mark.parametrize("epi", [R.EPI_NONE, R.EPI_SILU_MUL])
@pytest.mark.parametrize("operands", ["exact", "random"])
def test_tile_gemm(lib, cuda, M, N, K, kernel, epi, operands):
    """vstar_vqa_op_gemm with the tile kernels forced (kernel 2: the dispatcher's tile kernel; 5: the 8-wave 256 x 256 kernel) at
    M > 64, NONE with bias + residual and SILU_MUL.  "exact": operands whose accumulators are exact in fp32, under the gate
    2^-10 |ref| + 2^-22 sum |a w| as it stands; "random": the same gate plus one fp16 step where an accumulator lies within
    2^-22 sum |a w| of a rounding tie, and the subnormal store's 2^-25 (gemm_inputs says why the plain gate cannot hold there)."""
    A, W, bias, res = R.gemm_inputs(M, N, K, epi, operands)
    n_out = N // 2 if epi == R.EPI_SILU_MUL else N
    out = Out(cuda, M, n_out)
    Ad, Wd, bd, rd = dev(cuda, A), dev(cuda, W), dev(cuda, bias) if bias is not None else None, dev(cuda, res) if res is not None else None
    ok(lib, lib.vstar_vqa_op_gemm(P(Ad), P(Wd), P(bd), P(rd), P(out.full), M, N, K, epi, kernel, None, 0.0))
    ref, gate = R.gemm_ref(A, W, bias, res, N, epi, acc_err=operands == "random")
    gate_check(f"gemm {operands} M{M} N{N} K{K} kernel{kernel} epi{epi}", out.get(), ref, gate)


# ================================================================ refusals
def test_doors_refuse_what_they_cannot_run(lib, cuda):
    """VSTAR_ERR_INVALID with a message and nothing written: D = 96, too few qkv / out rows, a row_index entry >= x_rows,
    cols % 8 != 0."""
    B, S, H = 1, 40, 1
    out = Out(cuda, B * S, H * 128)
    qkv = dev(cuda, R.random_qkv(B, S, H, 128, 1))
    refused(lib, lib.vstar_vqa_op_attention(P(qkv), B * S, P(out.full), B * S, B, S, H, 96, 0), out)
    refused(lib, lib.vstar_vqa_op_attention(P(qkv), B * S - 1, P(out.full), B * S, B, S, H, 128, 0), out)
    refused(lib, lib.vstar_vqa_op_attention(P(qkv), B * S, P(out.full), B * S - 1, B, S, H, 128, 0), out)
    refused(lib, lib.vstar_vqa_op_attention(None, B * S, P(out.full), B * S, B, S, H, 128, 0), out)

    x, idx, gam, bet = R.norm_inputs(5, 72, 1)
    xd, gd, bd = dev(cuda, x), dev(cuda, gam), dev(cuda, bet)
    out = Out(cuda, 5, 72)
    bad = np.ascontiguousarray(idx.numpy(), np.int32)
    bad[3] = x.shape[0]
    neg = np.ascontiguousarray(idx.numpy(), np.int32)
    neg[1] = -1
    for hidx in (bad, neg):
        refused(lib, lib.vstar_vqa_op_layernorm(P(xd), x.shape[0], P(gd), P(bd), P(out.full), 5, 72, 1e-5, HP(hidx), 0), out)
        refused(lib, lib.vstar_vqa_op_rmsnorm(P(xd), x.shape[0], P(gd), P(out.full), 5, 72, 1e-6, HP(hidx)), out)
    refused(lib, lib.vstar_vqa_op_layernorm(P(xd), 4, P(gd), P(bd), P(out.full), 5, 72, 1e-5, None, 0), out)       # x_rows < rows
    refused(lib, lib.vstar_vqa_op_rmsnorm(P(xd), 4, P(gd), P(out.full), 5, 72, 1e-6, None), out)
    refused(lib, lib.vstar_vqa_op_layernorm(P(xd), x.shape[0], P(gd), P(bd), P(out.full), 5, 68, 1e-5, None, 0), out)
    refused(lib, lib.vstar_vqa_op_rmsnorm(P(xd), x.shape[0], P(gd), P(out.full), 5, 68, 1e-6, None), out)
    refused(lib, lib.vstar_vqa_op_layernorm(P(xd), x.shape[0], P(gd), P(bd), P(out.full), 5, 72, 1e-5, None, 2), out)
    refused(lib, lib.vstar_vqa_op_add_bcast(P(xd), P(bd), P(out.full), 5, 68, 1), out)
    refused(lib, lib.vstar_vqa_op_add_bcast(P(xd), P(bd), P(out.full), 5, 72, 0), out)
    refused(lib, lib.vstar_vqa_op_vit_assemble_tokens(P(xd), P(gd), P(xd), P(out.full), 1, 4, 68), out)
    refused(lib, lib.vstar_vqa_op_vit_assemble_tokens(P(xd), None, P(xd), P(out.full), 1, 4, 72), out)
