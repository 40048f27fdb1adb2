"""Pins tests/_prefill_ops_ref.py on the CPU and asserts every condition tests/test_prefill_ops_gpu.py relies on: probe values are
exactly representable, sums are exact in fp32 in any order, every geometry lies inside the doors' domain and the kernels'
eligibility predicates.  The doors' refusals are host-only (nothing is launched), so they are checked here too, with fake pointers:
that also ties the doors' row map and RoPE position rules to the reference's, through the row / position their messages name."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _prefill_ops_ref as R

ERR_INVALID = -1


# ---------------------------------------------------------------- bf16 helpers
def test_bf_and_bits_agree_with_torch():
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 37
    t = torch.from_numpy(x).bfloat16()
    assert np.array_equal(R.bits(R.bf(x)), t.view(torch.int16).numpy().view(np.uint16))
    assert R.is_bf16(R.bf(x)) and not R.is_bf16(np.float32(257.0)) and R.is_bf16(np.float32(256.0))
    assert R.bits(np.float32(1.0)) == 0x3F80


# ---------------------------------------------------------------- row maps
def _map_loop(M, g, s, o):          # the definition, one row at a time
    out = []
    for r in range(M):
        out.append(r if g <= 0 else (r // g) * s + o + (r - (r // g) * g))
    return np.array(out)


@pytest.mark.parametrize("name", list(R.MAP_CASES))
def test_map_cases(name):
    (M, N, K), am, cm, tile = R.MAP_CASES[name]
    for m in (am, cm):
        rows = R.touched_rows(M, m)
        assert np.array_equal(rows, _map_loop(M, m.group, m.gstride, m.off))
        assert len(set(rows.tolist())) == M and rows.min() >= 0           # injective: no two compact rows share a buffer row
        assert R.extent(M, m) > M                                         # there ARE gap rows to keep the sentinel
    assert K % 64 == 0
    if tile == 256:
        assert M >= 1024 and N >= 256 and K % 128 == 0 and M % 256        # gemm256's domain, ragged last row tile
    else:
        assert M < 1024
    if name == "g256_partial":                                            # the partial group lands exactly on the prefix rows
        nseq, Sr, S, Lp = 10, 103, 128, 25
        assert M == nseq * Sr + Lp
        assert np.array_equal(R.touched_rows(M, am)[-Lp:], nseq * S + Lp + np.arange(Lp))
        assert np.array_equal(R.touched_rows(M, am)[:Sr], Lp + np.arange(Sr))


@pytest.mark.parametrize("name", list(R.MAP_CASES))
@pytest.mark.parametrize("scaled", [False, True])
def test_map_probe_is_exact(name, scaled):
    (M, N, K), am, cm, _ = R.MAP_CASES[name]
    p = R.map_probe(M, N, K, am, cm, scaled)
    assert R.is_bf16(p.A) and R.is_bf16(p.W) and R.is_bf16(p.C)
    ar, cr = R.touched_rows(M, am), R.touched_rows(M, cm)
    assert (p.A[ar].sum(axis=1) == 1).all() and (p.A[ar].max(axis=1) == 1).all()         # one-hot compact rows
    gap = np.ones(len(p.A), bool)
    gap[ar] = False
    assert (p.A[gap] == 3).all()
    # asymmetric W: the transpose, a shifted row and a shifted column all differ
    assert not np.array_equal(p.W[:K, :K], p.W[:K, :K].T) and not np.array_equal(p.W[1:], p.W[:-1]) and not np.array_equal(p.W[:, 1:], p.W[:, :-1])
    # float64 product of the buffers through the maps, with the kernel's rounding points
    acc = p.A[ar].astype(np.float64) @ p.W.astype(np.float64).T
    if scaled:
        assert R.is_bf16(p.row_scale) and R.is_bf16(p.res)
        assert set(np.log2(p.row_scale[ar]).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
        scaled_acc = acc * p.row_scale[ar][:, None]
        assert R.is_bf16(scaled_acc)                                     # power-of-two scales: the product stays exact
        want = scaled_acc + p.res[cr]
        assert np.abs(want).max() < 64 and np.array_equal(want * 4, np.round(want * 4))
        assert R.is_bf16(want) and np.array_equal(p.C[cr], want)         # so even the sum needs no rounding
        if p.sumsq is not None:                                          # multiples of 1/16 below 2^18: 22 bits, exact in any order
            assert np.array_equal(p.sumsq * 16, np.round(p.sumsq * 16)) and p.sumsq.max() < 2 ** 18
    else:
        assert np.array_equal(p.C[cr], acc) and np.abs(acc).max() <= 250
    assert p.c_written.sum() == M and not p.c_written.all()


# ---------------------------------------------------------------- RoPE
def test_rope_pos_three_rules():
    for M in (1024, 1030):
        for mode in R.rope_modes(M):
            pos = R.rope_pos(np.arange(M), mode)
            for r in range(M):                                            # kernels.hpp, restated row by row
                q = r % mode.S
                if mode.R0 and q >= mode.R0:
                    q = mode.Lc + ((q - mode.R0) & 31)
                if mode.tail:
                    q = r - mode.tail if r >= mode.tail else r % mode.S + mode.pos0
                assert pos[r] == q
            assert pos.min() == 0 and pos.max() < 1024
            if mode.R0:
                assert mode.R0 % 128 == 0 and 0 < mode.Lc <= mode.R0 and (mode.S - mode.R0) % 32 == 0
                assert mode.Lc % 32, "Lc off the 32 grid: `& 31` vs `& 63`, `Lc +` vs `R0 +` all differ"
                blk = np.arange(mode.R0, mode.S).reshape(-1, 32)
                assert (pos[blk] == mode.Lc + np.arange(32)).all()       # every suffix block restarts at Lc
            if mode.tail:
                assert M == mode.tail + mode.pos0 and mode.tail % mode.S == 0
                assert np.array_equal(pos[mode.tail:], np.arange(mode.pos0))            # the prefix rows: positions 0 .. Lp
                assert np.array_equal(pos[:mode.S], mode.pos0 + np.arange(mode.S))      # a sequence starts at Lp
                m = R.prefix_map(mode)
                rows = R.touched_rows(M, m)
                S = mode.S + mode.pos0
                assert np.array_equal(rows[-mode.pos0:], (mode.tail // mode.S) * S + mode.pos0 + np.arange(mode.pos0))
                assert np.array_equal(rows[:mode.tail] % S, pos[:mode.tail])             # buffer row inside its sequence == position


def test_rope_apply_rounding_points():
    g = np.random.default_rng(1)
    x, y, c, s = (R.bf(g.standard_normal(5000)) for _ in range(4))
    got = R.rope_apply(x, -y, c, s)
    # float64 with the same three roundings: products of two bf16 are exact in float64 AND in float32
    p1, p2 = x.astype(np.float64) * c, -y.astype(np.float64) * s
    assert np.array_equal(p1, (x * c).astype(np.float64)) and np.array_equal(p2, (-y * s).astype(np.float64))
    want = R.bf((R.bf(p1).astype(np.float64) + R.bf(p2)).astype(np.float32))    # sum of two bf16 is exact in float64; one rounding to f32 then bf16
    same = np.array_equal(R.bits(got), R.bits(want))
    # (float64 -> float32 -> bf16 can double-round; where it does not, the two must agree bit for bit)
    exact32 = (R.bf(p1).astype(np.float64) + R.bf(p2)) == (R.bf(p1) + R.bf(p2)).astype(np.float64)
    assert same or np.array_equal(R.bits(got)[exact32], R.bits(want)[exact32])
    assert exact32.mean() > 0.9
    # against torch's bf16 ops, which round after every operation
    t = lambda a: torch.from_numpy(a).bfloat16()  # noqa: E731
    tw = (t(x) * t(c)) + (t(-y) * t(s))
    assert np.array_equal(R.bits(got), tw.view(torch.int16).numpy().view(np.uint16))
    # rotate-half on a head
    h = R.bf(g.standard_normal((7, 128)))
    cs = R.llama_table(7)
    o = R.rope_heads(h, cs)
    assert np.array_equal(o[:, :64], R.rope_apply(h[:, :64], -h[:, 64:], cs[:, :64], cs[:, 64:]))
    assert np.array_equal(o[:, 64:], R.rope_apply(h[:, 64:], h[:, :64], cs[:, :64], cs[:, 64:]))


def test_rope_probe_names_position_and_column():
    t = R.probe_table(1024)
    assert R.is_bf16(t) and t.max() <= 255 and t.min() >= 0
    pos = t[:, 0] + 256 * (t[:, 64] // 64)
    assert np.array_equal(pos, np.arange(1024))                           # (cos, sin) of a row name its position
    assert np.array_equal(t[:, 64:] % 64, np.broadcast_to(np.arange(64), (1024, 64)))      # sin names the column
    assert len({r.tobytes() for r in t}) == 1024
    for M, K in ((1024, 128), (1030, 128), (1030, 4096)):
        A, W = R.rope_probe_operands(M, K)
        pre = A.astype(np.float64) @ W.astype(np.float64).T
        assert np.array_equal(pre, np.broadcast_to(((np.arange(768) % 128) < 64).astype(np.float64), (M, 768)))
        for mode in R.rope_modes(M):
            table = t[: int(R.rope_pos(np.arange(M), mode).max()) + 1]
            want = R.rope_probe_expected(M, mode, table)
            # rotating the exact pre-rotation value reproduces the table entries: cos + (-0 * sin), 0 * cos + 1 * sin
            assert np.array_equal(R.bits(R.rope_qk(pre.astype(np.float32), table, R.rope_pos(np.arange(M), mode), R.ROPE_HEADS)), R.bits(want))
            assert np.array_equal(want[:, R.ROPE_COLS:], pre[:, R.ROPE_COLS:])             # v columns: the raw pattern
        if K == 128:
            break
    assert R.ROPE_COLS % 256 == 0 and R.ROPE_HEADS * 128 == R.ROPE_COLS and R.ROPE_N == R.ROPE_COLS * 3 // 2


# ---------------------------------------------------------------- statistics
@pytest.mark.parametrize("name", list(R.STATS_CASES))
def test_int_operands_give_exact_sums(name):
    (M, N, K), tile = R.STATS_CASES[name]
    A, W = R.int_operands(M, N, K, 3)
    C = A.astype(np.float64) @ W.astype(np.float64).T
    assert R.is_bf16(C) and np.abs(C).max() <= K <= 256 and np.abs(C).max() > 8
    sm, sq = R.span_sums(C)
    assert np.array_equal(sm, np.round(sm)) and np.array_equal(sq, np.round(sq))
    assert np.abs(sm).max() < 2 ** 24 and sq.max() < 2 ** 24 and R.span_abs(C).max() < 2 ** 24          # integers below 2^24: exact in any order
    assert N % 64 == 0 and len({tuple(r) for r in sq.round().astype(int).tolist()}) > M // 2               # rows differ: a row slip shows
    assert (sm != 0).mean() > 0.5
    if tile != 128:
        assert M >= 1024 and N % 256 == 0 and K % 128 == 0
    if tile == 2564:
        assert M % 256 == 0
    if name in R.STATS_CMAP:
        assert len(set(R.touched_rows(M, R.STATS_CMAP[name]).tolist())) == M


def test_span_sums_layout():
    C = np.arange(2 * 128, dtype=np.float64).reshape(2, 128)
    sm, sq = R.span_sums(C)
    assert sm.shape == (2, 2) and sm[1, 1] == C[1, 64:].sum() and sq[0, 1] == (C[0, 64:] ** 2).sum()


# ---------------------------------------------------------------- grouped attention
@pytest.mark.parametrize("geo", R.GROUPED + [R.GROUPED_MX])
def test_grouped_mask_is_the_contract(geo):
    B, S, H, R0, Lc = geo
    assert R.in_domain(S, R0, Lc) and 128 * H >= S
    m = R.grouped_mask(S, R0, Lc)
    assert np.array_equal(m[:R0], R.causal_mask(S)[:R0])                  # rows below R0, the rows [Lc, R0) included: plain causal
    for i in range(R0, S):                                                # kernels.hpp:247-249 restated key by key
        b0 = R0 + 32 * ((i - R0) // 32)
        for j in range(S):
            assert m[i, j] == (j < Lc or b0 <= j <= i), (i, j)
    assert m.diagonal().all()
    # suffix block b under the mask == plain causal attention over [prefix rows 0 .. Lc) ; block b]
    qkv = R.spiked_qkv(B, S, H, R0, Lc, 11)
    full = R.masked_attention(qkv, B, S, H, m).out
    seqs, nseq, S2 = R.block_sequences(qkv, B, S, H, R0, Lc)
    part = R.masked_attention(seqs, nseq, S2, H, R.causal_mask(S2)).out
    nb = R.n_blocks(S, R0)
    assert nb >= 1
    for b in range(B):
        for blk in range(nb):
            rows = R.block_rows(S, R0, blk)
            assert np.array_equal(m[rows][:, np.r_[0:Lc, rows]], R.causal_mask(S2)[Lc:])     # the same visibility, key for key
            assert not m[rows][:, np.setdiff1d(np.arange(S), np.r_[0:Lc, rows])].any()
            np.testing.assert_allclose(full[b, rows], part[b * nb + blk, Lc:], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("geo", R.GROUPED)
def test_visibility_probe(geo):
    B, S, H, R0, Lc = geo
    qkv, key = R.visibility_probe(B, S, H)
    assert R.is_bf16(qkv)
    x = qkv.reshape(B, S, 3, H, 128)
    assert not x[:, :, :2].any()
    for b in range(B):
        covered = np.sort(key[b].ravel())
        assert np.array_equal(covered[covered < S], np.arange(S))       # the heads together name every key exactly once
        assert (x[b, :, 2].sum(axis=0) == (key[b] < S)).all()            # one 1 per named column
    if B > 1:
        assert not np.array_equal(x[0, :, 2], x[1, :, 2])
    m = R.grouped_mask(S, R0, Lc)
    ref = R.masked_attention(qkv, B, S, H, m)
    n = m.sum(axis=1)
    for b in range(B):
        for h in range(H):
            vis = np.where(key[b, h][None, :] < S, m[:, np.minimum(key[b, h], S - 1)], False)
            assert np.array_equal(ref.out[b, :, h] != 0, vis)
            np.testing.assert_allclose(ref.out[b, :, h][vis], np.broadcast_to(1.0 / n[:, None], vis.shape)[vis], rtol=1e-14)
    # what a correct bf16 kernel stores, 1 / n rounded once, passes TIGHT with room: 2^-9 / n against (2^-8 + 2^-7) / n
    assert (np.abs(R.bf(ref.out) - ref.out) <= 0.5 * ref.tight).all()


def test_spiked_inputs_force_the_rescale_path():
    for B, S, H, R0, Lc in R.GROUPED:
        qkv = R.spiked_qkv(B, S, H, R0, Lc, 5)
        assert R.is_bf16(qkv)
        x = qkv.reshape(B, S, 3, H, 128).astype(np.float64)
        log2e = 1.4426950408889634
        m = R.grouped_mask(S, R0, Lc)
        for blk in range(R.n_blocks(S, R0)):
            rows = R.block_rows(S, R0, blk)
            s = (x[0, rows[-1], 0, 0] @ x[0, :, 1, 0].T) / np.sqrt(128.0) * log2e       # the kernel's base-2 score units
            seen = np.flatnonzero(m[rows[-1]])                                            # in the order the kernel walks them
            assert Lc - 1 in seen and rows[5] in seen
            before_own = seen[seen < rows[5]]
            assert s[rows[5]] - s[before_own].max() > 20                  # the own-block key outgrows everything before it by 2^16
            if Lc > 32:                                                   # the prefix key is not in the first sub-tile: a rescale there too
                assert s[Lc - 1] - s[: Lc - 1].max() > 20
    assert any(Lc > 32 for _, _, _, _, Lc in R.GROUPED)


def test_gates_reuse_the_decode_builders():
    from tests import _decode_ops_ref as D
    assert R.tight_gate is D.tight_gate and R.loose_gate is D.loose_gate
    o, pv, va = np.float64(0.5), np.float64(0.75), np.float64(40.0)
    assert D.tight_gate(o, pv, va) == 2.0 ** -10 * o + 2.0 ** -9 * pv + 2.0 ** -23 * va                  # fp16: the decode file's TIGHT
    assert D.tight_gate(o, pv, va, R.U_BF16) == 2.0 ** -8 * o + 2.0 ** -7 * pv + 2.0 ** -23 * va         # bf16: four times the step


# ---------------------------------------------------------------- the doors' refusals (host only)
def _msg(lib):
    return (lib.vstar_last_error(None) or b"").decode()


@pytest.mark.parametrize("case", R.gemm_refusals(), ids=lambda c: c[0])
def test_gemm_ex_refuses_before_any_launch(lib, case):
    _, fields, fragment = case
    g = R.gemm_ex(**fields)
    assert lib.vstar_op_gemm_ex(None, ctypes.byref(g)) == ERR_INVALID
    assert fragment in _msg(lib), _msg(lib)
    assert _msg(lib).startswith("vstar_op_gemm_ex: ")


def test_gemm_ex_extent_messages_name_the_reference_rows(lib):
    """One row short of the reference's extent is refused with the reference's largest row / position in the message, for every
    geometry the GPU file uses: the door's map_row and position rules are the reference's."""
    base = dict(A=True, W=True, C=True, epilogue=R.EPI_NONE)
    for name, ((M, N, K), am, cm, _) in R.MAP_CASES.items():
        f = dict(base, M=M, N=N, K=K, lda=K, ldc=N, w_rows=(N + 255) // 256 * 256, a_group=am.group, a_gstride=am.gstride, a_off=am.off,
                 c_group=cm.group, c_gstride=cm.gstride, c_off=cm.off, a_rows=R.extent(M, am), c_rows=R.extent(M, cm))
        for which, m in (("a", am), ("c", cm)):
            g = R.gemm_ex(**dict(f, **{which + "_rows": R.extent(M, m) - 1}))
            assert lib.vstar_op_gemm_ex(None, ctypes.byref(g)) == ERR_INVALID
            assert f"mapped {which.upper()} row {R.extent(M, m) - 1} outside" in _msg(lib), (name, _msg(lib))
    for M in (1024, 1030):
        for mode in R.rope_modes(M):
            top = int(R.rope_pos(np.arange(M), mode).max())
            g = R.gemm_ex(**dict(base, M=M, N=768, K=128, lda=128, ldc=768, w_rows=768, a_rows=M, c_rows=M, rope_cs=True, rope_rows=top,
                                 rope_S=mode.S, rope_cols=512, rope_R0=mode.R0, rope_Lc=mode.Lc, rope_pos0=mode.pos0, rope_tail=mode.tail))
            assert lib.vstar_op_gemm_ex(None, ctypes.byref(g)) == ERR_INVALID
            assert f"RoPE position {top} outside rope_rows = {top}" in _msg(lib), (mode, _msg(lib))


@pytest.mark.parametrize("case", R.attention_refusals(), ids=lambda c: c[0])
def test_grouped_attention_doors_refuse(lib, case):
    _, (qr, orows, B, S, H, R0, Lc), fragment = case
    fake = ctypes.c_void_p(0x10000)
    assert lib.vstar_op_attention_grouped(None, fake, qr, fake, orows, B, S, H, R0, Lc) == ERR_INVALID
    assert fragment in _msg(lib) and _msg(lib).startswith("vstar_op_attention_grouped: ")
    if (B * S) % 128 == 0:
        assert lib.vstar_op_attention_mx_grouped(None, fake, qr, fake, orows, fake, B, S, H, R0, Lc) == ERR_INVALID
        assert fragment in _msg(lib) and _msg(lib).startswith("vstar_op_attention_mx_grouped: ")


def test_rope_door_refuses(lib):
    fake = ctypes.c_void_p(0x10000)
    for args, fragment in (((288, 131, 1, 288, 2, 128, 128, 100), "RoPE position 131 outside table_rows = 131"),
                           ((33, 32, 1, 33, 2, 64, 0, 0), "RoPE position 32 outside table_rows = 32"),
                           ((287, 288, 1, 288, 2, 128, 0, 0), "qkv_rows < B * S"),
                           ((288, 288, 1, 288, 2, 96, 0, 0), "D must be 64 or 128"),
                           ((288, 288, 1, 288, 2, 128, 128, 129), "0 < grp_Lc <= grp_R0")):
        qkv_rows, table_rows, B, S, H, D, R0, Lc = args
        assert lib.vstar_op_rope(None, fake, qkv_rows, fake, table_rows, B, S, H, D, R0, Lc) == ERR_INVALID
        assert fragment in _msg(lib), _msg(lib)
    assert lib.vstar_op_attention_mx_grouped(None, fake, 160, fake, 160, fake, 1, 160, 2, 128, 100) == ERR_INVALID
    assert "B * S % 128" in _msg(lib)
