"""The references of tests/_bf16_decode_ref.py pinned on the CPU, and every condition of its input builders asserted for every
parametrisation tests/test_bf16_decode_gpu.py runs: the one-hot probes keep a score gap of 110 and are exactly one-hot ON THE
REFERENCE, the exact-dot inputs have dot products no summation order can change, the GEMV probes change under the fault of the
kernels' geometry each of them is meant to catch."""
import numpy as np
import pytest
import torch

from oracle.vqa_oracle import rope_tables, rotate_half
from tests import _bf16_decode_ref as B
from tests import _decode_ops_ref as R
from tests import _gemm128_ref as G

PATHS_ANC = [(p, a) for p in (0, 1, 2) for a in (False, True)]


def test_storage_type():
    assert B.U == 2.0 ** -8 and B.BF16.u == B.U
    x = B.bf16_codes(20000, 3)
    assert B.is_bf16(x) and np.isfinite(x).all() and (x != 0).all()
    assert len(np.unique(B.bits(x[:15616]))) == 15616                 # 61 binades x 128 significands x 2 signs, each once per run
    assert np.abs(x).max() < 2.0 ** 31 and np.abs(x).min() >= 2.0 ** -30
    assert np.array_equal(B.bits(B.bf(x)), B.bits(x))
    # u: 1 + 2^-8 is a tie (to even: 1), 1 + 3 * 2^-9 rounds up to 1 + 2^-7
    assert B.bf(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -9], np.float32)).tolist() == [1.0, 1 + 2.0 ** -7]
    assert "2^-8" in R.tight_gate.__doc__ and "2^-9" not in R.tight_gate.__doc__


def test_rope_rows_is_the_oracles_rotary_code_in_bf16():
    """Bit for bit q * cos + rotate_half(q) * sin of oracle/vqa_oracle.py in bf16 (each torch op rounds once)."""
    rows = 70
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, 3, 128, generator=g).to(torch.bfloat16)
    cos, sin = rope_tables(rows, 128, 1e4, torch.bfloat16)
    want = x * cos[:, None] + rotate_half(x) * sin[:, None]
    got = R.rope_rows(x.float().numpy(), R.llama_table(rows, st=B.BF16)[:, None], B.BF16)
    assert np.array_equal(B.bits(got), B.bits(want.float().numpy()))
    t = R.grid_table(576, B.BF16)
    assert B.is_bf16(t) and set(np.unique(t.astype(float))) <= {0.0, 0.5, -0.5, 1.0, -1.0}
    x = B.bf16_codes(5 * 128, 1).reshape(5, 128)
    assert np.array_equal(B.bits(R.rope_rows(x, R.identity_table(5, B.BF16), B.BF16)), B.bits(x))


@pytest.mark.parametrize("table", ["llama", "grid"])
@pytest.mark.parametrize("H", [1, 3])
def test_append_case_conditions(H, table):
    c = B.append_case(H, table)
    assert c.st is B.BF16 and c.R == 37 and (c.row_pos < 0).sum() == 5
    assert all(B.is_bf16(a) for a in (c.qkv, c.K, c.V, c.table))
    ref = R.append_ref(c)
    assert ref.written.sum() == 32 * H
    pad = c.row_pos < 0
    assert np.array_equal(B.bits(ref.qkv[pad]), B.bits(c.qkv[pad]))
    live = ~pad
    assert not np.array_equal(B.bits(ref.qkv[live]), B.bits(c.qkv[live]))                  # the rotation is not a no-op
    assert not np.array_equal(B.bits(ref.K[ref.written]), B.bits(c.K[ref.written]))
    v = slice(2 * H * 128, 3 * H * 128)
    assert np.array_equal(B.bits(ref.qkv[:, v]), B.bits(c.qkv[:, v]))                      # v untouched


@pytest.mark.parametrize("path,anc", PATHS_ANC)
def test_probe_conditions(path, anc):
    """Every round of every probe geometry the GPU test runs: the score gap is at least 110 (exp is 0 in fp32 in either denormal
    mode, and in bf16 the rounded probability is 0 as well), p is exactly one-hot, o is V[target] bit for bit."""
    lane_groups = set()
    for g in R.cases_geometry(path, anc=anc):
        want_targets = [set(R.probe_targets(path, int(p), int(g["seq_past"][s]))) for p, s in zip(g["row_pos"], g["row_seq"])]
        hit = [set() for _ in want_targets]
        for t in range(R.probe_rounds(path, g)):
            c = B.probe_case(path, g, t)
            ref = R.attention_ref(c)
            assert B.probe_gap(c, ref) >= B.PROBE_GAP, (c.name, B.probe_gap(c, ref))
            assert R.one_hot(c, ref), c.name
            assert all(B.is_bf16(a) for a in (c.qkv, c.K, c.V, ref.out))
            assert np.isfinite(c.K).all() and np.isfinite(c.V).all() and (c.V != 0).all()
            if path >= 1:
                assert R.fused_reads_clear_of_writes(c), c.name
            for r in range(c.R):
                if c.row_pos[r] < 0:
                    continue
                ks = c.key_slots(r)
                for hh in range(c.H):
                    jt = c.targets[r, hh]
                    hit[r].add(int(jt))
                    Vd = (ref.append.V if path >= 1 else c.V)[ks[jt], hh, jt]
                    assert np.array_equal(B.bits(ref.out[r, hh]), B.bits(Vd))
                    lane_groups.add(int(np.nonzero(c.qkv.reshape(c.R, 3, c.H, 128)[r, 0, hh])[0][0]) // 8)
        for r, w in enumerate(want_targets):
            assert hit[r] == w - {-1}, (r, hit[r], w)
    assert lane_groups == set(range(16))
    # the gap is what makes the probe exact: e^-110 is below half the smallest fp32 subnormal and half the smallest bf16 subnormal
    assert np.exp(-B.PROBE_GAP) < 2.0 ** -150 and np.exp(-B.PROBE_GAP) < 2.0 ** -134
    assert np.float32(np.exp(np.float64(-B.PROBE_GAP))) == 0


def test_fp16_probe_scale_would_not_be_exact_in_bf16():
    """With the fp16 probes' q = k = 16 (gap 22.625) the reference's non-target probabilities are NOT zero in bf16: the reason for the
    new scale."""
    g = R.cases_geometry(0)[0]
    c = R.probe_case(0, 0, g, 0, st=B.BF16, mag=(16, 16))
    assert not R.one_hot(c, R.attention_ref(c))


@pytest.mark.parametrize("path,anc", PATHS_ANC)
def test_exact_dot_conditions(path, anc):
    g = R.cases_geometry(path, which=None if path == 0 else 1, anc=anc)[0]
    c = B.exact_dot_case(path, g)
    ref = R.attention_ref(c)
    assert ref.exact_dots and R.lumpy(ref), c.name
    q = c.qkv.reshape(c.R, 3, c.H, 128).astype(float)
    assert np.all(q[:, :2] * 8 == np.round(q[:, :2] * 8)) and np.abs(q[:, :2]).max() <= 1
    assert all(B.is_bf16(a) for a in (c.qkv, c.K, c.V, c.table))
    Kf = c.K.astype(float)
    assert np.all(Kf * 8 == np.round(Kf * 8)) and np.abs(Kf).max() <= 1                     # the n / 8 grid is representable in bf16
    if path >= 1:
        assert R.fused_reads_clear_of_writes(c)
    err = np.abs(ref.out.astype(float) - ref.f64)[ref.valid]
    assert (err <= ref.loose[ref.valid]).all()
    # TIGHT stays below a tenth of what a lost key with p = 0.05 moves (0.05 |v|, |v| ~ 0.4): a gate that still sees a dropped key
    assert (ref.tight[ref.valid] < 0.05 * (np.abs(ref.out[ref.valid].astype(float)) + 0.5)).all()
    # the gates are the documented formulas with u = 2^-8
    r = int(np.nonzero(ref.valid)[0][0])
    ks = c.key_slots(r)
    K, V = (ref.append.K, ref.append.V) if path >= 1 else (c.K, c.V)
    Vd = V[ks, 0, np.arange(len(ks))].astype(float)
    p = ref.p[r][0].astype(float)
    want = 2 * B.U * np.abs(ref.out[r, 0].astype(float)) + 4 * B.U * (p[:, None] * np.abs(Vd)).sum(0) + 2.0 ** -23 * np.abs(Vd).sum(0)
    assert np.allclose(ref.tight[r, 0], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("path", [0, 1, 2])
def test_random_reference_is_float64_attention_within_loose(path):
    g = R.cases_geometry(path, which=None if path == 0 else 1)[0]
    c = B.random_case(path, g)
    ref = R.attention_ref(c)
    assert np.isfinite(ref.out).all() and B.is_bf16(ref.out)
    err = np.abs(ref.out.astype(float) - ref.f64)[ref.valid]
    assert (err <= ref.loose[ref.valid]).all(), float((err / ref.loose[ref.valid]).max())


@pytest.mark.parametrize("C", [8, 264])
def test_embed_rows_reference(C):
    src, table, feats = R.embed_case(C, st=B.BF16)
    assert B.is_bf16(table) and B.is_bf16(feats)
    got = R.embed_rows(src, table, feats)
    want = np.zeros((len(src), C), np.float32)
    for r, s in enumerate(src.tolist()):
        if 0 <= s < len(table):
            want[r] = table[s]
        elif -len(feats) <= s < 0:
            want[r] = feats[-s - 1]
    assert np.array_equal(B.bits(got), B.bits(want))
    assert len(np.unique(np.concatenate([B.bits(table).ravel(), B.bits(feats).ravel()]))) == table.size + feats.size


@pytest.mark.parametrize("cols", R.ARGMAX_COLS)
def test_argmax_references(cols):
    x, ld = R.argmax_case(cols, st=B.BF16)
    assert B.is_bf16(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)) and ld == cols + 9
    got = R.argmax_rows(x[:, :cols])
    assert got[4] == 0 and got[5] == 0 and got[6] == 0 and got[7] == cols - 1 and got[2] == 0
    assert got[8] == (cols - 2 if cols > 1 else 0)
    # what only bf16 can hold
    assert B.NEG_MAX < B.NEG_AT_OR_BELOW <= -3.0e38 < B.NEG_JUST_ABOVE and np.isfinite(B.NEG_MAX)
    assert B.bits(np.array([B.NEG_AT_OR_BELOW], np.float32))[0] == B.bits(np.array([B.NEG_JUST_ABOVE], np.float32))[0] + 1   # neighbours
    assert np.float32(B.NEG_AT_OR_BELOW) <= np.float32(-3.0e38) < np.float32(B.NEG_JUST_ABOVE)       # ... on both sides of the kernel's -3.0e38f
    x, ld = B.argmax_extreme_case(cols)
    got = R.argmax_rows(x[:, :cols])
    c = cols - 1
    assert got.tolist() == [0, c, c, 0, cols // 2, c]
    assert np.nanmax(x[0, :cols]) == B.NEG_AT_OR_BELOW and int(np.nanargmax(x[0, :cols])) == c


# ================================================================ the GEMV: shapes and faults
def test_gemv_shapes_cover_what_the_issue_lists():
    groups = [B.KSTEP_SHAPES, B.INDEX_SHAPES, B.INT_SHAPES]
    for shapes in groups:
        assert {m for m, _, _ in shapes} == set(B.M_VALUES)
        assert {n for _, n, _ in shapes} == set(B.N_VALUES)
    assert {k for _, _, k in B.KSTEP_SHAPES} == set(B.K_VALUES) and {k for s in groups for _, _, k in s} == set(B.K_VALUES) | {B.RING_LOOP_K}
    # the ring's main loop (slots re-filled behind counted waits) is live only from six stages per wave on: one shape of the integer,
    # SiLU-mul, random and norm groups each
    assert not any(B.wave_steps(k // 64, 0, 8, True, nt)[0] for k in B.K_VALUES if k >= 512 for nt in (1, 2))
    assert B.wave_steps(48, 0, 8, True, 1) == ([0, 8, 16], [24, 32, 40]) and B.wave_steps(48, 7, 7, True, 2) == ([7, 15, 23, 31], [39, 47])
    for shapes in (B.INT_SHAPES, B.SILU_SHAPES, B.RANDOM_SHAPES, B.NORM_SHAPES):
        assert any(k == B.RING_LOOP_K and B.ring_runs(m, k, shapes is B.NORM_SHAPES) for m, _, k in shapes)
    assert {n for _, n, _ in B.SILU_SHAPES} == set(B.SILU_N)
    assert [k // 64 for k in B.K_VALUES] == [1, 7, 8, 9, 17, 24]
    assert sorted({m for m, _, _ in B.NORM_SHAPES}) == [1, 7, 8, 16]
    # both sides of the ring limit, with and without the norm
    assert B.ring_runs(8, 512) and not B.ring_runs(9, 512) and not B.ring_runs(8, 448)
    assert B.ring_runs(7, 512, norm=True) and not B.ring_runs(8, 512, norm=True)
    for shapes in groups + [B.SILU_SHAPES]:
        assert any(B.ring_runs(m, k) for m, _, k in shapes) and any(not B.ring_runs(m, k) for m, _, k in shapes)
    # NT = 1 and NT = 2 tile-major images, on shapes the ring takes (only it reads the image)
    assert {e for *_, e in B.TILED_SHAPES} == {B.EPI_NONE, B.EPI_SILU_MUL}
    assert all(B.ring_runs(m, k) and n % (32 if e == B.EPI_SILU_MUL else 16) == 0 for m, n, k, e in B.TILED_SHAPES)


def test_wave_steps_partition_k():
    for M in B.M_VALUES:
        for K in B.K_VALUES:
            for ring in (False, True):
                if ring and not B.ring_runs(M, K):
                    continue
                for nt in (1, 2):
                    seen = []
                    for w in range(8):
                        main, tail = B.wave_steps(K // 64, w, M, ring, nt)
                        seen += main + tail
                    assert sorted(seen) == list(range(K // 64)), (M, K, ring, nt)
    # K = 576 on the register kernel with two row tiles: wave 0 owns steps 0 and 8 — one unrolled trip, nothing behind it; K = 1088:
    # steps 0, 8, 16 — one trip and a tail step
    assert B.wave_steps(9, 0, 17, False) == ([0, 8], []) and B.wave_steps(17, 0, 17, False) == ([0, 8], [16])
    assert B.wave_steps(9, 1, 17, False) == ([], [1])
    # the ring at K = 1536 (three stages per wave, depth 3): everything in the tail's first phase; NT = 2 (depth 2): two phases
    assert B.wave_steps(24, 0, 8, True, 1) == ([], [0, 8, 16]) and B.wave_steps(24, 0, 8, True, 2) == ([], [0, 8, 16])
    assert B.wave_steps(64, 0, 8, True, 2) == ([0, 8, 16, 24, 32, 40], [48, 56])


@pytest.mark.parametrize("M,N,K", B.KSTEP_SHAPES)
def test_kstep_probe_sees_a_dropped_or_misread_step(M, N, K):
    """2^(K / 64) - 1 everywhere without a fault; any dropped tail step and any wave on its neighbour's steps changes it.  The value
    needs K / 64 <= 24 significant bits: fp32 output."""
    A, W, C = B.ktile_probe(M, N, K)
    assert B.is_bf16(A) and B.is_bf16(W) and G.is_fp32(C) and K // 64 <= 24
    for ring in {False, B.ring_runs(M, K)}:
        assert np.array_equal(B.skinny_acc(A, W, ring=ring), C)
        if B.has_tail(M, K, ring):
            assert (B.skinny_acc(A, W, ring=ring, fault=("drop_tail",)) != C).all()
        if K > 64:
            for w in (0, 7):
                assert (B.skinny_acc(A, W, ring=ring, fault=("neighbour", w)) != C).all(), (ring, w)
    # as a sum of 2^step the wrong value names the steps that entered
    if B.has_tail(M, K, False):
        got = B.skinny_acc(A, W, fault=("drop_tail",))[0, 0]
        assert got < C[0, 0] and float(C[0, 0] - got) == sum(2.0 ** B.wave_steps(K // 64, w, M, False)[1][-1]
                                                                 for w in range(8) if B.wave_steps(K // 64, w, M, False)[1])


def test_some_kstep_shape_has_a_live_tail_on_each_kernel():
    assert any(B.has_tail(m, k, False) for m, _, k in B.KSTEP_SHAPES if not B.ring_runs(m, k))
    assert any(B.has_tail(m, k, True) for m, _, k in B.KSTEP_SHAPES if B.ring_runs(m, k))
    assert any(B.wave_steps(k // 64, 0, m, False)[0] and B.wave_steps(k // 64, 0, m, False)[1] for m, _, k in B.KSTEP_SHAPES if m > 16)


@pytest.mark.parametrize("M,N,K", B.INDEX_SHAPES)
def test_index_probe_sees_a_wrong_row_clamp(M, N, K):
    """Every (row, column) has its own code: C[r, n] = W[n, (37 r) % K] = (n K + (37 r) % K) % 251, a bf16 integer."""
    p = B.index_probe(M, N, K)
    assert B.is_bf16(p.A) and B.is_bf16(p.W) and B.is_bf16(p.C)
    assert np.array_equal(B.skinny_acc(p.A, p.W), p.C[:M])
    if M >= 2:
        bad = B.skinny_acc(p.A, p.W, fault=("row_clamp",))
        assert (bad[M - 1] != p.C[M - 1]).any() and np.array_equal(bad[: M - 1], p.C[: M - 1])
    # neighbouring rows and neighbouring columns differ somewhere: a shifted row tile or column group is visible
    if M >= 2:
        assert all((p.C[r] != p.C[r + 1]).any() for r in range(M - 1))
    assert all((p.C[:, n] != p.C[:, n + 1]).any() for n in range(N - 1))


@pytest.mark.parametrize("M,N,K", B.INT_SHAPES)
def test_int_operand_conditions(M, N, K):
    A, W = B.int_operands(M, N, K, 11)
    assert G.exact_fp32(A, W) and B.is_bf16(A) and B.is_bf16(W)
    acc = G.product(A, W)
    assert np.array_equal(B.skinny_acc(A, W), acc) and np.abs(acc).max() <= 256      # every accumulator a bf16 integer
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    assert B.is_bf16(bias) and B.is_bf16(res)
    for epi in (B.EPI_NONE, B.EPI_RELU):
        for f32 in (False, True):
            out = B.epilogue(acc, epi, f32, bias, res)
            assert G.is_fp32(out) and (f32 or B.is_bf16(out))


@pytest.mark.parametrize("M,N,K", B.SILU_SHAPES)
def test_silu_int_operands_see_a_swapped_tile(M, N, K):
    A, W = B.int_operands(M, N, K, 7)
    acc = G.product(A, W)
    want = B.epilogue(acc, B.EPI_SILU_MUL)
    assert want.shape == (M, N // 2) and B.is_bf16(want)
    ring = B.ring_runs(M, K)
    assert np.array_equal(B.skinny_acc(A, W, nt=2, ring=ring), acc)
    swapped = B.epilogue(B.skinny_acc(A, W, nt=2, ring=ring, fault=("swap_tiles",)), B.EPI_SILU_MUL)
    assert (swapped != want).mean() > 0.3
    if B.has_tail(M, K, ring, 2):
        assert (B.epilogue(B.skinny_acc(A, W, nt=2, ring=ring, fault=("drop_tail",)), B.EPI_SILU_MUL) != want).any()


@pytest.mark.parametrize("M,N,K", B.GELU_SHAPES)
def test_activation_intervals(M, N, K):
    """GELU: the one-rounding reference lies in every interval, most intervals are one point (EXACT), and the quick-GELU formula in
    GELU's place leaves them.  Quick-GELU: the restated rounding points leave one point nearly everywhere, and sigmoid(1.5 t) in place
    of sigmoid(1.702 t) leaves the intervals.
    fp32 forms: float32 arithmetic of the same expressions lies within the gate, and the gate is of fp32 size."""
    assert any(B.ring_runs(m, k) for m, _, k in B.GELU_SHAPES) and any(m > 16 for m, _, _ in B.GELU_SHAPES)
    A, W = B.int_operands(M, N, K, 11)
    acc = G.product(A, W)
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    for b, r in ((True, False), (False, True), (True, True)):
        bb, rr = (bias if b else None), (res if r else None)
        t = B.bf(acc + (bias[None, :] if b else 0)).astype(np.float64)

        def finish(a):
            a = B.bf(a).astype(np.float64)
            return B.bf(a + res).astype(np.float64) if r else a
        lo, hi = B.act16_interval(acc, B.EPI_GELU, bb, rr)
        ref = B.epilogue(acc, B.EPI_GELU, False, bb, rr)
        assert B.is_bf16(lo) and B.is_bf16(hi) and ((lo <= ref) & (ref <= hi)).all()
        assert (lo == hi).mean() > 0.5 and (hi - lo).max() <= 2 * B.ERF_ERR * np.abs(t).max() + 2.0 ** -7 * np.abs(ref).max()
        quick = finish(t / (1 + np.exp(-1.702 * t)))
        assert ((quick < lo) | (quick > hi)).mean() > 0.03
        lo, hi = B.act16_interval(acc, B.EPI_QUICK_GELU, bb, rr)
        assert (lo == hi).mean() > 0.9                        # (two points where the sigmoid leaves the normal fp32 range or a tie is near)
        wrong = finish(t * B.bf(1 / (1 + np.exp(-B.bf(1.5 * t).astype(np.float64)))).astype(np.float64))
        assert ((wrong < lo) | (wrong > hi)).mean() > 0.03
        for epi in (B.EPI_GELU, B.EPI_QUICK_GELU):
            ref32, gate = B.act32_ref(acc, epi, bb, rr)
            t32 = (acc + (bias[None, :] if b else 0)).astype(np.float32)
            if epi == B.EPI_GELU:
                a32 = np.float32(0.5) * t32 * (np.float32(1) + torch.erf(torch.from_numpy(t32 * np.float32(0.70710678))).numpy())
            else:
                with np.errstate(over="ignore"):
                    a32 = t32 * (np.float32(1) / (np.float32(1) + np.exp(-(B.C1702 * t32))))
            a32 = a32 + (res.astype(np.float32) if r else np.float32(0))
            assert (np.abs(a32.astype(np.float64) - ref32) <= gate).all()
            assert (gate <= 2.0 ** -19 * (np.abs(t32) + np.abs(ref32)) + 1e-30).all()       # nothing bf16-sized hides in this gate


def test_silu_sigmoid_flush_is_restated():
    """What the GPU test found on the parent's kernels: with gate = -88 and up = 13 (integer operands, M 8, N 96, K 1536, seed 3,
    output (7, 4)) the kernel stores -0.0 where _gemm128_ref.epilogue has -6.91e-36.  Restated here: the kernel's sigmoid is
    v_rcp_f32(1 + e^88) = v_rcp_f32(1.65e38), a subnormal 6.05e-39 that the instruction flushes to zero."""
    A, W = B.int_operands(8, 96, 1536, 3)
    acc = G.product(A, W)
    gate, up = G.unpack_gate_up(acc)
    assert gate[7, 4] == -88 and up[7, 4] == 13
    ref, restated = B.epilogue(acc, B.EPI_SILU_MUL), B.kernel_silu_mul(acc)
    region = B.silu_flush_region(acc)
    assert region[7, 4] and region.sum() == 1
    assert np.isclose(ref[7, 4], -6.9119e-36, rtol=1e-4) and restated[7, 4] == 0 and np.signbit(restated[7, 4])
    assert np.array_equal(B.bits(restated.astype(np.float32))[~region], B.bits(ref.astype(np.float32))[~region])
    assert abs(restated[7, 4] - ref[7, 4]) <= B.silu_flush_gate(acc)[7, 4] < 1e-34
    # the threshold: sigmoid(-87) is a normal fp32 number with a margin, sigmoid(-88) is not
    assert 1 + np.exp(87.0) < 0.72 * 2.0 ** 126 and 1 + np.exp(88.0) > 2.0 ** 126 and abs(-126 * np.log(2) + 87.34) < 0.01
    # every other SiLU-mul case of the GPU test lies outside the region: EXACT everywhere
    for M, N, K in B.SILU_SHAPES:
        a = G.product(*B.int_operands(M, N, K, 7))
        assert not B.silu_flush_region(a).any()
        assert np.array_equal(B.kernel_silu_mul(a), B.epilogue(a, B.EPI_SILU_MUL))


@pytest.mark.parametrize("M,N,K", B.NORM_SHAPES)
def test_norm_reference(M, N, K):
    """The float64 RMSNorm rows against torch's LlamaRMSNorm arithmetic in bf16, within the gate; the gate is the fp16 prefill gate
    with u = 2^-8."""
    from tests import _small_ops_ref as S
    x, gam = B.norm_inputs(M, K, 5)
    assert B.is_bf16(x) and B.is_bf16(gam)
    y, gate = B.rmsnorm_ref(x, gam, 1e-6)
    stored = S.rmsnorm_bf16(torch.from_numpy(x).bfloat16(), torch.from_numpy(gam).bfloat16(), 1e-6).float().numpy().astype(float)
    assert (np.abs(stored - y) <= gate).all()
    assert (gate >= 2.0 ** -7 * np.abs(y)).all() and (gate <= 2.0 ** -7 * np.abs(y) + np.abs(gam)[None] * B.ulp_bf16(y / gam[None])).all()
    assert B.ulp_bf16(1.0) == 2.0 ** -7 and B.ulp_bf16(3.0) == 2.0 ** -6
    assert B.tie_slack(np.array([1 + 2.0 ** -8]), np.array([1e-9]))[0] == 2.0 ** -7 and B.tie_slack(np.array([1.0]), np.array([1e-9]))[0] == 0
