"""Operator-level tests of the prefill-side GemmParams / attn_* features on the MI355X that no other door reaches: GEMM row maps,
the RoPE fused into the GEMM epilogue (three implementations, three position rules), the LayerNorm sums (`stats_sum`) and grouped
attention — each driven alone through vstar_op_gemm_ex / vstar_op_rope / vstar_op_attention_grouped / vstar_op_attention_mx_grouped
against tests/_prefill_ops_ref.py (pinned on the CPU by tests/test_prefill_ops_ref.py, which also asserts every condition of the
input builders used here and the doors' refusals).

Conventions of every test:
  * every buffer has exactly the extent the door is told plus two rows behind it (RoPE tables are allocated whole and the door is
    told only the rows the call may read), and the door has checked every mapped / derived row against those extents before it
    launches;
  * every output buffer — gap rows of a row map, gap columns (ldc > N), the rows behind it — is pre-filled with a sentinel NaN
    pattern, and everything outside the reference's touched set must come back bit-unchanged;
  * vstar_op_gemm_last_tile() must name the kernel the case was written for;
  * EXACT = equal bits.  TIGHT / LOOSE: the gates of _prefill_ops_ref.masked_attention, derived from the formats.  Every non-exact
    comparison prints one `PREFILLOP_ERR` line with the measured error and its share of the gate (run with -s to record them).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _prefill_ops_ref as R
from tests.test_small_ops_gpu import dv  # noqa: F401  (the fixture)
from vstar_amd import _lib

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
FLAG = {128: _lib.EPI_TILE128, 256: _lib.EPI_TILE256, _lib.TILE_4W: _lib.EPI_TILE4W}
VARIANTS = (2, 5, 6, 7)                 # of the 128-row family: double buffer, loader-wave ring on the 128 x 128 / 128 x 64 / 128 x 256 tile


def ok(lib, rc):
    assert rc == 0, lib.vstar_last_error(None)


def up16(cuda, x):
    """float32-held bf16 values -> device bf16."""
    return None if x is None else R.to_t(x).to(cuda)


def sent16(cuda, rows, cols):
    return torch.full((rows, cols), R.SENT16 - 65536 if R.SENT16 >= 32768 else R.SENT16, dtype=torch.int16, device=cuda)


def sent32(cuda, rows, cols):
    return torch.full((rows, cols), R.SENT32, dtype=torch.int32, device=cuda)


def host16(t):
    """device int16 / bf16 tensor -> uint16 bit patterns."""
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def as_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def pad_w(W):
    n = (len(W) + 255) // 256 * 256
    out = np.zeros((n, W.shape[1]), np.float32)
    out[: len(W)] = W
    return out


class Gemm:
    """One vstar_op_gemm_ex call over freshly sentinel-filled outputs.  A / row_scale are BUFFERS (a_rows rows), res a buffer of
    c_rows rows; the C buffer gets `ldc` columns and two rows behind the c_rows the door is told.  variant: VSTAR_EPI_VARIANT of the
    128-row family for this call (tile 128), and vstar_op_gemm_last_mode() must name it."""

    def __init__(self, lib, cuda, A, W, M, tile, *, am=R.IDENT, cm=R.IDENT, ldc=None, row_scale=None, res=None, sumsq=False, stats=False,
                 rope=None, variant=0):
        N, K = W.shape                      # (a device W is already padded: only for N % 256 == 0)
        assert not torch.is_tensor(W) or N % 256 == 0
        self.M, self.N = M, N
        self.c_rows = R.extent(M, cm)
        self.cr = R.touched_rows(M, cm)
        a_rows = R.extent(M, am)
        assert A.shape == (a_rows, K), (A.shape, a_rows)
        self.ldc = ldc or N + 8
        dA = A if torch.is_tensor(A) else up16(cuda, A)
        dW = W if torch.is_tensor(W) else up16(cuda, pad_w(W))
        self.C = sent16(cuda, self.c_rows + 2, self.ldc)
        keep = [dA, dW, self.C]
        f = dict(A=P(dA), lda=K, a_rows=a_rows, a_group=am.group, a_gstride=am.gstride, a_off=am.off, W=P(dW), w_rows=dW.shape[0],
                 C=P(self.C), ldc=self.ldc, c_rows=self.c_rows, c_group=cm.group, c_gstride=cm.gstride, c_off=cm.off, M=M, N=N, K=K,
                 epilogue=_lib.EPI_NONE | FLAG[tile] | _lib.EPI_VARIANT(variant))
        if row_scale is not None:
            assert len(row_scale) == a_rows
            keep.append(torch.from_numpy(np.ascontiguousarray(row_scale, np.float32)).to(cuda))
            f["row_scale"] = P(keep[-1])
        if res is not None:
            assert res.shape == (self.c_rows, N)
            keep.append(up16(cuda, res))
            f.update(residual=P(keep[-1]), ldr=N)
        self.spans = N // 64
        self.S = None
        if sumsq:
            self.sum_at = self.spans + 1 if stats else 0          # one gap column between the sums of squares and the sums
            self.sld = (self.sum_at + self.spans if stats else self.spans) + 3
            self.S = sent32(cuda, self.c_rows + 2, self.sld)
            keep.append(self.S)
            f.update(sumsq_out=P(self.S), sumsq_ld=self.sld, stats_sum=self.sum_at)
        if rope is not None:
            table, rope_rows, mode = rope            # (the whole device table, the rows of it this call may read)
            keep.append(table)
            f.update(rope_cs=P(table), rope_rows=rope_rows, rope_S=mode.S, rope_cols=R.ROPE_COLS, rope_R0=mode.R0, rope_Lc=mode.Lc,
                     rope_pos0=mode.pos0, rope_tail=mode.tail)
        self.keep = keep
        g = R.gemm_ex(**f)
        ok(lib, lib.vstar_op_gemm_ex(None, ctypes.byref(g)))
        assert lib.vstar_op_gemm_last_tile() == tile, (lib.vstar_op_gemm_last_tile(), tile)
        if variant:
            assert tile == 128 and lib.vstar_op_gemm_last_mode() == variant, (lib.vstar_op_gemm_last_mode(), variant)

    def output(self):
        """[M, N] bit patterns of the compact rows, after checking that every gap row, gap column and row behind kept the sentinel."""
        got = host16(self.C)
        mask = np.zeros(got.shape, bool)
        mask[self.cr, : self.N] = True
        assert (got[~mask] == R.SENT16).all(), "the GEMM wrote outside the mapped rows / its N columns"
        return got[self.cr, : self.N]

    def partials(self):
        """(sums of squares, sums or None) [M, N / 64] as float32, after the same check on the statistics buffer."""
        got = self.S.cpu().numpy().view(np.uint32)
        mask = np.zeros(got.shape, bool)
        mask[self.cr, : self.spans] = True
        if self.sum_at:
            mask[self.cr, self.sum_at: self.sum_at + self.spans] = True
        assert (got[~mask] == R.SENT32).all(), "statistics written outside [0, N/64) and [stats_sum, stats_sum + N/64) of the mapped rows"
        f = got.view(np.float32)
        return f[self.cr, : self.spans], (f[self.cr, self.sum_at: self.sum_at + self.spans] if self.sum_at else None)


def err_line(name, err, gate, ref, kind):
    share = np.where(gate > 0, err / np.where(gate > 0, gate, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"PREFILLOP_ERR {name}: abs {err.max():.3e} rel {err.max() / max(np.abs(ref).max(), 1e-30):.3e} "
          f"worst err/gate {share.max():.3f} [{kind}]")
    assert (err <= gate).all(), float(share.max())


# ================================================================ row maps
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", list(R.MAP_CASES))
def test_row_map_probe(lib, cuda, name, scaled, variant=0):
    """One-hot compact rows: C[crow(r), n] == W[n, r % K] in bits; with row_scale (by mapped A row), residual and sums of squares (by
    mapped C row) the stored value is still exact.  Gap rows of A / row_scale / residual hold poison."""
    (M, N, K), am, cm, tile = R.MAP_CASES[name]
    p = R.map_probe(M, N, K, am, cm, scaled)
    g = Gemm(lib, cuda, p.A, p.W, M, tile, am=am, cm=cm, row_scale=p.row_scale, res=p.res, sumsq=p.sumsq is not None, variant=variant)
    assert np.array_equal(g.output(), R.bits(p.C[g.cr]))
    if p.sumsq is not None:
        sq, _ = g.partials()
        assert np.array_equal(sq.astype(np.float64), p.sumsq[g.cr])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("name", ["g128", "g128_stats"])
def test_row_map_probe_gemm128_variants(lib, cuda, name, scaled, variant):
    """test_row_map_probe's 128-row cases on each of the family's four kernels, requested per call."""
    test_row_map_probe(lib, cuda, name, scaled, variant)


@pytest.mark.parametrize("name", list(R.MAP_CASES))
def test_row_map_random_equals_gathered(lib, cuda, name, variant=0):
    """Random inputs: the mapped call equals, bit for bit, the same forced kernel on the gathered A (row_scale, residual gathered
    likewise) with its output scattered here."""
    (M, N, K), am, cm, tile = R.MAP_CASES[name]
    g0 = np.random.default_rng(M + N)
    ar, cr = R.touched_rows(M, am), R.touched_rows(M, cm)
    A = R.bf(g0.standard_normal((R.extent(M, am), K)))
    W = R.bf(g0.standard_normal((N, K)) / np.sqrt(K))
    rs = np.exp(g0.standard_normal(R.extent(M, am))).astype(np.float32)
    res = R.bf(g0.standard_normal((R.extent(M, cm), N)))
    stats = N % 64 == 0
    mapped = Gemm(lib, cuda, A, W, M, tile, am=am, cm=cm, row_scale=rs, res=res, sumsq=stats, stats=stats, variant=variant)
    dense = Gemm(lib, cuda, A[ar], W, M, tile, row_scale=rs[ar], res=res[cr], sumsq=stats, stats=stats, variant=variant)
    out = mapped.output()
    assert not np.isnan(as_f32(out)).any()
    assert np.array_equal(out, dense.output())
    if stats:
        for a, b in zip(mapped.partials(), dense.partials()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["g128", "g128_stats"])
def test_row_map_random_equals_gathered_gemm128_variants(lib, cuda, name, variant):
    test_row_map_random_equals_gathered(lib, cuda, name, variant)


def test_gemm_ex_refusals_launch_nothing(lib, cuda):
    """Every refusal of the table, now with real buffers of the sizes the fields name: VSTAR_ERR_INVALID, a message, C and the
    statistics untouched."""
    C, S = sent16(cuda, 2048, 768), sent32(cuda, 2048, 24)
    bufs = {"A": torch.zeros(2048, 128, dtype=torch.bfloat16, device=cuda), "W": torch.zeros(768, 128, dtype=torch.bfloat16, device=cuda), "C": C,
            "sumsq_out": S, "rope_cs": torch.zeros(1024, 128, dtype=torch.bfloat16, device=cuda)}
    for name, fields, fragment in R.gemm_refusals():
        g = R.gemm_ex(ptr=lambda k: bufs[k].data_ptr(), **fields)
        assert lib.vstar_op_gemm_ex(None, ctypes.byref(g)) == ERR_INVALID, name
        assert fragment in lib.vstar_last_error(None).decode(), name
    torch.cuda.synchronize()
    assert (host16(C) == R.SENT16).all() and (S.cpu().numpy().view(np.uint32) == R.SENT32).all()


# ================================================================ fused RoPE
# name -> (M, K, tile, VSTAR_GEMM_DEBUG or None)
ROPE_KERNELS = {
    "gemm4w": (1024, 128, _lib.TILE_4W, None),
    "gemm256_direct": (1024, 128, 256, None),
    "gemm256_lds": (1024, 128, 256, "4"),
    "gemm256_ragged": (1030, 128, 256, None),            # interior tiles direct, the edge row tile through the LDS epilogue
    "gemm4w_rowguard": (1030, 4096, _lib.TILE_4W, None),  # ragged last row tile inside the direct epilogue (ROWGUARD)
}


def set_debug(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("VSTAR_GEMM_DEBUG", raising=False)
    else:
        monkeypatch.setenv("VSTAR_GEMM_DEBUG", value)


def table_rows(M, mode):
    """How many table rows a call over M rows in `mode` may read: exactly up to its largest position."""
    return int(R.rope_pos(np.arange(M), mode).max()) + 1


@pytest.mark.parametrize("kernel", list(ROPE_KERNELS))
def test_fused_rope_position_probe(lib, cuda, monkeypatch, kernel):
    """Pre-rotation value exactly 1 | 0 per head half, table entries naming (position, column): every stored q | k element is the table
    entry of the position and column the kernel read (EXACT), the v columns the raw pattern.  All three position rules; the
    shared-prefix rule also through its row map (where the kernel takes row maps)."""
    M, K, tile, debug = ROPE_KERNELS[kernel]
    set_debug(monkeypatch, debug)
    A, W = R.rope_probe_operands(M, K)
    dA, dW = up16(cuda, A), up16(cuda, pad_w(W))
    full = R.probe_table(1024)
    dT = up16(cuda, full)
    for mode in R.rope_modes(M):
        n_tab = table_rows(M, mode)
        want = R.bits(R.rope_probe_expected(M, mode, full[:n_tab]))
        g = Gemm(lib, cuda, dA, dW, M, tile, rope=(dT, n_tab, mode))
        got = g.output()
        bad = np.argwhere(got != want)
        assert not len(bad), (kernel, mode, bad[:4].tolist(), as_f32(got[tuple(bad[0])]), as_f32(want[tuple(bad[0])]))
        if mode.tail and tile == 256:
            m = R.prefix_map(mode)
            Ab = np.full((R.extent(M, m), K), 3.0, np.float32)          # gap rows: poison
            Ab[R.touched_rows(M, m)] = A
            g = Gemm(lib, cuda, Ab, dW, M, tile, am=m, cm=m, rope=(dT, n_tab, mode))
            assert np.array_equal(g.output(), want), (kernel, mode, "with the row map")


def _rope_random(lib, cuda, monkeypatch, kernels, M, K, seed):
    """Per kernel and mode: the fused output.  Asserts, per kernel, fused == rope_apply on that kernel's un-fused output (all three
    rules; the v columns therefore in bits too) and == the same un-fused output rotated by vstar_op_rope (plain and grouped rules)."""
    g0 = np.random.default_rng(seed)
    A = R.bf(g0.standard_normal((M, K)))
    W = R.bf(g0.standard_normal((R.ROPE_N, K)) / np.sqrt(K))
    dA, dW = up16(cuda, A), up16(cuda, pad_w(W))
    full = R.llama_table(1024)
    dT = up16(cuda, full)
    outs = {}
    for kernel, (tile, debug) in kernels.items():
        set_debug(monkeypatch, debug)
        raw = Gemm(lib, cuda, dA, dW, M, tile, ldc=R.ROPE_N)
        c0 = raw.output()
        assert not np.isnan(as_f32(c0)).any()
        for mode in R.rope_modes(M):
            n_tab = table_rows(M, mode)
            pos = R.rope_pos(np.arange(M), mode)
            fused = Gemm(lib, cuda, dA, dW, M, tile, ldc=R.ROPE_N, rope=(dT, n_tab, mode)).output()
            want = R.bits(R.rope_qk(as_f32(c0), full[:n_tab], pos, R.ROPE_HEADS))
            assert np.array_equal(fused, want), (kernel, mode)
            assert np.array_equal(fused[:, R.ROPE_COLS:], c0[:, R.ROPE_COLS:])
            assert not np.array_equal(fused[:, : R.ROPE_COLS], c0[:, : R.ROPE_COLS])
            outs[kernel, mode] = fused
            if not mode.tail:           # the door's rule covers it: rotate the un-fused rows on the device
                rows = -(-M // mode.S) * mode.S              # whole sequences; the rows behind M are zero
                buf = torch.zeros(rows + 2, R.ROPE_N, dtype=torch.int16, device=cuda)
                buf[:M] = raw.C[:M]
                ok(lib, lib.vstar_op_rope(None, P(buf), rows, P(dT), n_tab, rows // mode.S, mode.S, 2, 128, mode.R0, mode.Lc))
                assert np.array_equal(host16(buf)[:M], fused), (kernel, mode, "vstar_op_rope")
    return outs


def test_fused_rope_random_three_kernels(lib, cuda, monkeypatch):
    """M = 1024: gemm4w, gemm256's direct epilogue and its LDS epilogue agree with the reference and with each other in bits."""
    kernels = {k: ROPE_KERNELS[k][2:] for k in ("gemm4w", "gemm256_direct", "gemm256_lds")}
    outs = _rope_random(lib, cuda, monkeypatch, kernels, 1024, 128, 21)
    for mode in R.rope_modes(1024):
        assert np.array_equal(outs["gemm256_direct", mode], outs["gemm256_lds", mode]), mode
        assert np.array_equal(outs["gemm4w", mode], outs["gemm256_direct", mode]), mode


def test_fused_rope_random_ragged(lib, cuda, monkeypatch):
    """M = 1030: gemm256 with its ragged edge tile (both epilogues in one launch) against the reference and the all-LDS launch."""
    outs = _rope_random(lib, cuda, monkeypatch, {"gemm256_ragged": (256, None), "all_lds": (256, "4")}, 1030, 128, 22)
    for mode in R.rope_modes(1030):
        assert np.array_equal(outs["gemm256_ragged", mode], outs["all_lds", mode]), mode


def test_fused_rope_random_rowguard(lib, cuda, monkeypatch):
    """(1030, 768, 4096): gemm4w's ragged last row tile (ROWGUARD) against the reference and against gemm256."""
    outs = _rope_random(lib, cuda, monkeypatch, {"gemm4w_rowguard": (_lib.TILE_4W, None), "gemm256": (256, None)}, 1030, 4096, 23)
    for mode in R.rope_modes(1030):
        assert np.array_equal(outs["gemm4w_rowguard", mode], outs["gemm256", mode]), mode


# ================================================================ vstar_op_rope
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S,R0,Lc,B,H", [(33, 0, 0, 2, 3), (288, 128, 100, 2, 2)])
def test_op_rope(lib, cuda, D, S, R0, Lc, B, H):
    """EXACT against rope_apply with the kernel's rounding points; the v third, and the rows behind the buffer, untouched."""
    g0 = np.random.default_rng(D + S)
    mode = R.RopeMode(S, R0=R0, Lc=Lc)
    pos = R.rope_pos(np.arange(B * S), mode)
    n_tab = int(pos.max()) + 1
    table = R.bf(g0.uniform(-1, 1, (n_tab + 64, D)))          # (the door is told n_tab rows)
    x = R.bf(g0.standard_normal((B * S + 2, 3 * H * D)))
    want = x.copy()
    want[: B * S, : 2 * H * D] = R.rope_qk(x[: B * S, : 2 * H * D], table[:n_tab], pos, 2 * H, D)
    dx, dt = up16(cuda, x), up16(cuda, table)
    ok(lib, lib.vstar_op_rope(None, P(dx), B * S, P(dt), n_tab, B, S, H, D, R0, Lc))
    got = host16(dx)
    assert np.array_equal(got[:, 2 * H * D:], R.bits(x[:, 2 * H * D:])) and np.array_equal(got[B * S:], R.bits(x[B * S:]))
    assert np.array_equal(got, R.bits(want))
    assert not np.array_equal(got[: B * S, : 2 * H * D], R.bits(x[: B * S, : 2 * H * D]))


# ================================================================ stats_sum
@pytest.mark.parametrize("name,mapped", [(n, False) for n in R.STATS_CASES] + [(n, True) for n in R.STATS_CMAP],
                         ids=lambda v: v if isinstance(v, str) else ("c_map" if v else "identity"))
def test_stats_sum_exact(lib, cuda, name, mapped, variant=0):
    """Integer-valued C: sums of squares at [0, N/64), sums at [stats_sum, stats_sum + N/64), both equal to the float64 reference
    exactly, nothing else written (the gap column between them included).  Also through a C row map, for the kernels that take one
    (the door refuses the 4-wave kernel with a map: test_gemm_ex_refusals_launch_nothing)."""
    (M, N, K), tile = R.STATS_CASES[name]
    cm = R.STATS_CMAP[name] if mapped else R.IDENT
    A, W = R.int_operands(M, N, K, 3)
    C = (A.astype(np.float64) @ W.astype(np.float64).T).astype(np.float32)
    g = Gemm(lib, cuda, A, W, M, tile, cm=cm, sumsq=True, stats=True, variant=variant)
    assert np.array_equal(g.output(), R.bits(C))
    sm, sq = R.span_sums(C)
    got_sq, got_sm = g.partials()
    assert np.array_equal(got_sq.astype(np.float64), sq) and np.array_equal(got_sm.astype(np.float64), sm)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mapped", [False, True], ids=["identity", "c_map"])
def test_stats_sum_exact_gemm128_variants(lib, cuda, mapped, variant):
    """The g128 statistics case on each of the family's four kernels, requested per call."""
    test_stats_sum_exact(lib, cuda, "g128", mapped, variant)


def test_stats_sum_random_kernel_families_agree(lib, cuda, monkeypatch, dv):
    """(1024, 256, 128), random inputs: the partials of the 128 family, of both gemm256 epilogues and of gemm4w are equal in bits;
    vstar_op_ln_rstd from the partials equals vstar_op_ln_rstd from the stored C in bits; each sum lies within
    64 * 2^-24 * sum |x| (sum x^2 for the squares) of its float64 value — 64 fp32 additions of one rounding each, whatever the tree."""
    M, N, K = 1024, 256, 128
    g0 = np.random.default_rng(31)
    A = R.bf(g0.standard_normal((M, K)) + 0.5)
    W = R.bf(g0.standard_normal((N, K)) / np.sqrt(K))
    runs = {}
    for name, tile, debug in (("g128", 128, None), ("g256_direct", 256, None), ("g256_lds", 256, "4"), ("g4w", _lib.TILE_4W, None)):
        set_debug(monkeypatch, debug)
        g = Gemm(lib, cuda, A, W, M, tile, ldc=N, sumsq=True, stats=True)
        runs[name] = (g, g.output(), *g.partials())
    set_debug(monkeypatch, None)
    g, c, sq, sm = runs["g128"]
    for name, (_, c2, sq2, sm2) in runs.items():
        assert np.array_equal(c, c2), name
        assert np.array_equal(sq.view(np.uint32), sq2.view(np.uint32)) and np.array_equal(sm.view(np.uint32), sm2.view(np.uint32)), name
    stored = as_f32(c)
    ref_sm, ref_sq = R.span_sums(stored)
    err_line("stats_sum (1024,256,128)", np.abs(sm - ref_sm), 64 * 2.0 ** -24 * R.span_abs(stored), ref_sm, "64 * 2^-24 * sum|x|")
    err_line("sumsq (1024,256,128)", np.abs(sq - ref_sq), 64 * 2.0 ** -24 * ref_sq, ref_sq, "64 * 2^-24 * sum x^2")
    # the consumer: 1 / sqrt(var + eps) from the partials (sums of squares | sums, dense) and from the rows themselves
    spans = N // 64
    part = torch.from_numpy(np.ascontiguousarray(np.concatenate([sq, sm], axis=1))).to(cuda)
    r_part, r_rows = (torch.full((M + 2,), float("nan"), dtype=torch.float32, device=cuda) for _ in range(2))
    ok(lib, lib.vstar_op_ln_rstd(None, None, P(part), 2 * spans, M, N, 1e-5, P(r_part)))
    ok(lib, lib.vstar_op_ln_rstd(None, dv(R.to_t(stored)), None, 0, M, N, 1e-5, P(r_rows)))
    a, b = r_part.cpu().numpy(), r_rows.cpu().numpy()
    assert np.isnan(a[M:]).all() and np.isnan(b[M:]).all() and np.isfinite(a[:M]).all()
    assert np.array_equal(a[:M].view(np.uint32), b[:M].view(np.uint32))


# ================================================================ grouped attention
def run_grouped(lib, cuda, qkv, B, S, H, R0, Lc):
    """[B, S, H, 128] float32 of one vstar_op_attention_grouped call; the two rows behind the output must keep the sentinel."""
    dq = up16(cuda, qkv)
    out = sent16(cuda, B * S + 2, H * 128)
    ok(lib, lib.vstar_op_attention_grouped(None, P(dq), B * S, P(out), B * S, B, S, H, R0, Lc))
    got = host16(out)
    assert (got[B * S:] == R.SENT16).all(), "a row behind the output was written"
    assert np.array_equal(host16(dq), R.bits(qkv)), "qkv changed"
    o = as_f32(got[: B * S])
    assert np.isfinite(o).all()
    return o.reshape(B, S, H, 128), out


@pytest.mark.parametrize("geo", R.GROUPED, ids=lambda g: "B%d_S%d_H%d_R%d_Lc%d" % g)
def test_grouped_attention_visibility_probe(lib, cuda, geo):
    """q = 0 and one-hot V columns naming the keys: out[i, h, d] != 0 exactly where grouped_mask[i, key(h, d)] holds — for every row,
    the rows [Lc, R0) included, and both batch entries — and the non-zero values are 1 / n_visible(i) under TIGHT."""
    B, S, H, R0, Lc = geo
    qkv, key = R.visibility_probe(B, S, H)
    m = R.grouped_mask(S, R0, Lc)
    ref = R.masked_attention(qkv, B, S, H, m)
    got, _ = run_grouped(lib, cuda, qkv, B, S, H, R0, Lc)
    for b in range(B):
        for h in range(H):
            vis = np.where(key[b, h][None, :] < S, m[:, np.minimum(key[b, h], S - 1)], False)
            bad = np.argwhere((got[b, :, h] != 0) != vis)
            assert not len(bad), (b, h, "row, d:", bad[:6].tolist(), "keys:", key[b, h][bad[:6, 1]].tolist())
    err_line("grouped probe " + str(geo), np.abs(got - ref.out), ref.tight, ref.out, "TIGHT")


@pytest.mark.parametrize("geo", R.GROUPED, ids=lambda g: "B%d_S%d_H%d_R%d_Lc%d" % g)
def test_grouped_attention_random(lib, cuda, geo):
    """Random inputs with a spiked prefix key and a spiked own-block key (the rescale path): LOOSE against the float64 masked
    attention, and every suffix block's rows against plain vstar_op_attention over [prefix ; block] under LOOSE."""
    B, S, H, R0, Lc = geo
    qkv = R.spiked_qkv(B, S, H, R0, Lc, 5)
    ref = R.masked_attention(qkv, B, S, H, R.grouped_mask(S, R0, Lc))
    got, _ = run_grouped(lib, cuda, qkv, B, S, H, R0, Lc)
    err_line("grouped random " + str(geo), np.abs(got - ref.out), ref.loose, ref.out, "LOOSE")
    seqs, nseq, S2 = R.block_sequences(qkv, B, S, H, R0, Lc)
    dq = up16(cuda, seqs)
    out = sent16(cuda, nseq * S2 + 2, H * 128)
    ws_bytes = lib.vstar_op_attention_workspace(nseq, S2, H, 128)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    ok(lib, lib.vstar_op_attention(None, P(dq), P(out), P(ws), ws_bytes, nseq, S2, H, 128, 1, 0.0))
    plain = as_f32(host16(out)[: nseq * S2]).reshape(nseq, S2, H, 128)
    nb = R.n_blocks(S, R0)
    rows = np.concatenate([R.block_rows(S, R0, blk) for blk in range(nb)])
    mine = got[:, rows].reshape(B * nb, 32, H, 128)
    gate = ref.loose[:, rows].reshape(B * nb, 32, H, 128)
    err_line("grouped vs [prefix;block] " + str(geo), np.abs(mine - plain[:, Lc:]), gate, mine, "LOOSE")


def test_grouped_attention_mx(lib, cuda):
    """Output bytes and scale bytes equal vstar_op_attention_grouped followed by vstar_op_quantize_mx, in bits."""
    B, S, H, R0, Lc = R.GROUPED_MX
    qkv = R.spiked_qkv(B, S, H, R0, Lc, 9)
    _, out = run_grouped(lib, cuda, qkv, B, S, H, R0, Lc)
    nsc = lib.vstar_op_mx_scale_bytes(B * S, H * 128)
    assert nsc > 0
    q_ref = torch.full((B * S + 2, H * 128), 0xA5, dtype=torch.uint8, device=cuda)
    s_ref = torch.full((nsc + 16,), 0xA5, dtype=torch.uint8, device=cuda)
    ok(lib, lib.vstar_op_quantize_mx(None, P(out), P(q_ref), P(s_ref), B * S, H * 128))
    dq = up16(cuda, qkv)
    q_got, s_got = torch.full_like(q_ref, 0xA5), torch.full_like(s_ref, 0xA5)
    ok(lib, lib.vstar_op_attention_mx_grouped(None, P(dq), B * S, P(q_got), B * S, P(s_got), B, S, H, R0, Lc))
    assert torch.equal(q_got, q_ref) and torch.equal(s_got, s_ref)
    assert (q_got[B * S:] == 0xA5).all() and (s_got[nsc:] == 0xA5).all()
    assert (s_got[:nsc] != 0xA5).any()


def test_attention_and_rope_refusals_launch_nothing(lib, cuda):
    qkv = torch.zeros(600, 768, dtype=torch.bfloat16, device=cuda)
    out = sent16(cuda, 600, 256)
    o8 = torch.full((600, 256), 0xA5, dtype=torch.uint8, device=cuda)
    sc = torch.full((4096,), 0xA5, dtype=torch.uint8, device=cuda)
    for name, (qr, orows, B, S, H, R0, Lc), fragment in R.attention_refusals():
        assert lib.vstar_op_attention_grouped(None, P(qkv), qr, P(out), orows, B, S, H, R0, Lc) == ERR_INVALID, name
        assert fragment in lib.vstar_last_error(None).decode(), name
        assert lib.vstar_op_attention_mx_grouped(None, P(qkv), qr, P(o8), orows, P(sc), B, S, H, R0, Lc) == ERR_INVALID, name
    table = torch.zeros(131, 128, dtype=torch.bfloat16, device=cuda)
    assert lib.vstar_op_rope(None, P(qkv), 288, P(table), 131, 1, 288, 2, 128, 128, 100) == ERR_INVALID
    assert "RoPE position 131" in lib.vstar_last_error(None).decode()
    torch.cuda.synchronize()
    assert (host16(out) == R.SENT16).all() and (o8 == 0xA5).all() and (sc == 0xA5).all() and not qkv.any()
