"""The references of tests/_decode_ops_ref.py pinned on the CPU, and every condition of its input builders asserted for every
parametrisation tests/test_decode_ops_gpu.py runs: the probes are exactly one-hot ON THE REFERENCE, the exact-dot inputs have dot
products that no summation order can change and lumpy probabilities, the fused cases never read a cache row another row writes."""
import numpy as np
import pytest
import torch

from oracle.vqa_oracle import rope_tables, rotate_half
from tests import _decode_ops_ref as R

PATHS_FMTS_ANC = [(p, f, a) for p in (0, 1, 2) for f in (0, 1, 2) for a in (False, True)]


def test_rope_rows_is_the_oracles_rotary_code():
    """Bit for bit q * cos + rotate_half(q) * sin of oracle/vqa_oracle.py in fp16 (each torch op rounds once)."""
    rows = 70
    g = torch.Generator().manual_seed(0)
    x = torch.randn(rows, 3, 128, generator=g).to(torch.float16)
    cos, sin = rope_tables(rows, 128, 1e4, torch.float16)
    want = x * cos[:, None] + rotate_half(x) * sin[:, None]
    got = R.rope_rows(x.numpy(), R.llama_table(rows)[:, None])
    assert np.array_equal(R.bits(got), R.bits(want.numpy()))


def test_tables():
    t = R.grid_table(576)
    assert set(np.unique(t.astype(float))) <= {0.0, 0.5, -0.5, 1.0, -1.0}
    assert len(np.unique(R.bits(t), axis=0)) > 100                    # varies with the position
    assert np.all((t[:, :64].astype(float) != 0) | (t[:, 64:].astype(float) != 0))
    i = R.identity_table(5)
    x = R.f16_codes(5 * 128, 1).reshape(5, 128)
    assert np.array_equal(R.bits(R.rope_rows(x, i)), R.bits(x))       # the identity table keeps every finite code


def test_split_partitions_cover_the_listed_edges():
    """63 and 255: empty trailing partitions; 512: a full last partition; 513: the span changes from 64 to 128."""
    assert R.split_partitions(63)[0] == (0, 63) and all(lo == hi for lo, hi in R.split_partitions(63)[1:])
    assert R.split_partitions(255)[3] == (192, 255) and R.split_partitions(255)[4] == (255, 255)
    assert R.split_partitions(512)[7] == (448, 512)
    assert R.split_partitions(513)[0] == (0, 128) and R.split_partitions(513)[4] == (512, 513) and R.split_partitions(513)[5] == (513, 513)
    assert R.split_partitions(0) == [(0, 0)] * 8
    for pos in (0, 63, 255, 256, 300, 511, 512, 513):
        parts = R.split_partitions(pos)
        assert parts[0][0] == 0 and parts[-1][1] == pos and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))


def _fixed_point(x, fmt):
    return np.array_equal(R.bits(R.rt(x, fmt)), R.bits(x))


def _rows_distinct(x):
    flat = R.bits(x).reshape(-1, 128)
    return len(np.unique(flat, axis=0)) == len(flat)


@pytest.mark.parametrize("path,fmt,anc", PATHS_FMTS_ANC)
def test_probe_conditions(path, fmt, anc):
    """Every round of every probe geometry: p is exactly one-hot at the target, so o is V[target] bit for bit; V holds distinct,
    finite, non-zero rows; formats 1 and 2 hold fixed points of the round trip."""
    lane_groups = set()
    for g in R.cases_geometry(path, anc=anc):
        want_targets = [set(R.probe_targets(path, int(p), int(g["seq_past"][s]))) for p, s in zip(g["row_pos"], g["row_seq"])]
        hit = [set() for _ in want_targets]
        for t in range(R.probe_rounds(path, g)):
            c = R.probe_case(path, fmt, g, t)
            ref = R.attention_ref(c)
            assert R.one_hot(c, ref), c.name
            assert c.max_keys >= c.row_pos.max() + 1 and c.max_keys <= c.ctx
            assert _fixed_point(c.K, fmt) and _fixed_point(c.V, fmt)
            assert np.isfinite(c.K.astype(float)).all() and np.isfinite(c.V.astype(float)).all() and (c.V != 0).all()
            if t == 0:
                assert _rows_distinct(c.V) and _rows_distinct(c.K)
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
                    assert np.array_equal(R.bits(ref.out[r, hh]), R.bits(Vd))
                    lane_groups.add(int(np.nonzero(c.qkv.reshape(c.R, 3, c.H, 128)[r, 0, hh])[0][0]) // 8)
        for r, w in enumerate(want_targets):
            assert hit[r] == w - {-1}, (r, hit[r], w)
    assert lane_groups == set(range(16))


def test_probe_geometries_hold_what_the_issue_lists():
    g = R.geometry(0)
    assert (g["row_pos"] < 0).sum() == 2 and len(g["row_pos"]) == 9 and len(g["seq_kv"]) == 3 and g["seq_past"][1] == 5
    assert g["seq_prefix"][1] != g["seq_kv"][1] and not np.array_equal(g["seq_kv"], np.arange(3))
    assert sorted(p for tr in R.PATH1_POS for p in tr) == [0, 1, 63, 64, 65, 200]
    assert {p for tr in R.PATH2_POS for p in tr} == {0, 63, 255, 256, 300, 511, 512, 513}
    assert [max(tr) + 1 for tr in R.PATH2_POS] == [256, 514, 514]
    for path in (1, 2):
        for g in R.cases_geometry(path):
            assert g["ctx"] == (576 if path == 2 else 208) and g["slots"] * 2 * g["ctx"] <= 4 * 2 * 576
    a = R.geometry(2, anc=True)["anc"]
    assert (a[3, 0::2] == 3).all() and (a[3, 1::2] == 2).all()


@pytest.mark.parametrize("path,fmt,anc", PATHS_FMTS_ANC)
def test_exact_dot_conditions(path, fmt, anc):
    """Products are multiples of a power of two u with sum |q k| < 2^24 u for every (query, key); at least three keys with p > 0.05
    and none above 0.6 in every row; the inputs lie on the grids."""
    g = R.cases_geometry(path, which=None if path == 0 else 1, anc=anc)[0]
    c = R.exact_dot_case(path, fmt, g)
    ref = R.attention_ref(c)
    assert ref.exact_dots and R.lumpy(ref), c.name
    q = c.qkv.reshape(c.R, 3, c.H, 128).astype(float)
    assert np.all(q[:, :2] * 8 == np.round(q[:, :2] * 8)) and np.abs(q[:, :2]).max() <= 1
    assert set(np.unique(c.table.astype(float))) <= {0.0, 0.5, -0.5, 1.0, -1.0}
    assert _fixed_point(c.K, fmt) and _fixed_point(c.V, fmt)
    if path >= 1:
        assert R.fused_reads_clear_of_writes(c)
    # the reference against plain float64 softmax attention on the same operands, within LOOSE
    err = np.abs(ref.out.astype(float) - ref.f64)[ref.valid]
    assert (err <= ref.loose[ref.valid]).all()
    assert (ref.tight[ref.valid] < 0.01 * (np.abs(ref.out[ref.valid].astype(float)) + 0.5)).all()    # a gate far below a lost key's 0.05 |v|


@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("fmt", [0, 1])
def test_random_reference_is_float64_attention_within_loose(path, fmt):
    g = R.cases_geometry(path, which=None if path == 0 else 1)[0]
    c = R.random_case(path, fmt, g)
    ref = R.attention_ref(c)
    assert np.isfinite(ref.out.astype(float)).all()
    assert _fixed_point(c.K, fmt) and _fixed_point(c.V, fmt)
    err = np.abs(ref.out.astype(float) - ref.f64)[ref.valid]
    assert (err <= ref.loose[ref.valid]).all(), float((err / ref.loose[ref.valid]).max())
    if path >= 1:
        assert R.fused_reads_clear_of_writes(c)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_append_case_conditions(H, fmt):
    c = R.append_case(H, fmt)
    assert c.R == 37 and (c.row_pos < 0).sum() == 5 and len(set(c.row_seq.tolist())) == 3
    assert not np.array_equal(c.seq_kv, np.arange(3))
    live = c.row_pos[c.row_pos >= 0]
    assert (np.diff(live) < 0).any() and (np.diff(live) > 0).any()
    ref = R.append_ref(c)                                             # (asserts that no two rows write the same cache row)
    assert ref.written.sum() == 32 * H
    pad = c.row_pos < 0
    assert np.array_equal(R.bits(ref.qkv[pad]), R.bits(c.qkv[pad]))
    assert _fixed_point(c.K, fmt) and _fixed_point(c.V, fmt)
    if fmt:                                                           # the round trip moves k and v: the in-place rows are not a no-op
        assert not np.array_equal(R.bits(ref.K_raw), R.bits(ref.K))
    assert not np.array_equal(R.bits(ref.K[ref.written]), R.bits(c.K[ref.written]))


@pytest.mark.parametrize("DH", R.PERCEIVER_DH)
@pytest.mark.parametrize("n,H,L,NK", R.PERCEIVER_SHAPES)
def test_perceiver_conditions(n, H, L, NK, DH):
    # probes: exactly one-hot, the output is the target's value row
    q, kv, tg = R.perceiver_probe(n, H, L, NK, DH, 3)
    ref = R.perceiver_ref(q, kv, n, L, NK, H, DH)
    C = H * DH
    v = kv[:, C:].reshape(n, NK, H, DH)
    assert (v != 0).all() and np.isfinite(kv.astype(float)).all()
    for b in range(n):
        for hh in range(H):
            for i in range(L):
                want = np.zeros(NK, np.float16)
                want[tg[b, hh, i]] = 1
                assert np.array_equal(R.bits(ref.p[b, hh, i]), R.bits(want))
                assert np.array_equal(R.bits(ref.out.reshape(n, L, H, DH)[b, i, hh]), R.bits(v[b, tg[b, hh, i], hh]))
    # exact-dot: the kernel's fp32 way to q-hat is the reference's, the dots are exact, the probabilities lumpy
    q, kv = R.perceiver_exact(n, H, L, NK, DH, 4)
    qh = R.perceiver_qhat(q, DH)
    assert np.array_equal(R.bits(qh), R.bits(R.perceiver_qhat(q, DH, kernel_way=True)))
    a = np.abs(qh.astype(float))
    assert ((a >= 2.0 ** -5) & (a < 0.5) | (a == 0)).all()
    k = kv[:, :C].astype(float)
    assert np.all(k * 4 == np.round(k * 4)) and np.abs(k).max() <= 1
    ref = R.perceiver_ref(q, kv, n, L, NK, H, DH)
    assert ref.exact_dots
    if NK >= 3:                                                        # (a single key has p = 1: nothing to misplace)
        p = ref.p.astype(float)
        assert ((p > 0.05).sum(axis=-1) >= 3).all() and p.max() < 0.6, (float(p.max()), int((p > 0.05).sum(axis=-1).min()))
    assert (np.abs(ref.out.astype(float) - ref.f64) <= ref.loose).all()
    # random: the reference is float64 attention within LOOSE
    q, kv = R.perceiver_random(n, H, L, NK, DH, 5)
    assert np.array_equal(R.bits(R.perceiver_qhat(q, DH)), R.bits(R.perceiver_qhat(q, DH, kernel_way=True)))
    ref = R.perceiver_ref(q, kv, n, L, NK, H, DH)
    err = np.abs(ref.out.astype(float) - ref.f64)
    assert (err <= ref.loose).all(), float((err / ref.loose).max())


@pytest.mark.parametrize("C", [8, 264])
def test_embed_rows_reference(C):
    src, table, feats = R.embed_case(C)
    t, f = torch.from_numpy(table), torch.from_numpy(feats)
    want = torch.zeros(len(src), C, dtype=torch.float16)
    for r, s in enumerate(src.tolist()):
        if 0 <= s < len(t):
            want[r] = t[s]
        elif -len(f) <= s < 0:
            want[r] = f[-s - 1]
    got = R.embed_rows(src, table, feats)
    assert np.array_equal(R.bits(got), R.bits(want.numpy()))
    assert len(np.unique(np.concatenate([R.bits(table).ravel(), R.bits(feats).ravel()]))) == table.size + feats.size
    kinds = [(src >= 0) & (src < len(table)), (src < 0) & (src >= -len(feats)), src == R.INT32_MIN, src >= len(table),
             (src < -len(feats)) & (src != R.INT32_MIN)]
    assert all(k.any() for k in kinds)


@pytest.mark.parametrize("cols", R.ARGMAX_COLS)
def test_argmax_reference(cols):
    x, ld = R.argmax_case(cols)
    assert ld > cols and (x[:, cols:].astype(float) > np.nan_to_num(x[:, :cols].astype(float), nan=-1e9).max()).all()
    got = R.argmax_rows(x[:, :cols])
    t = torch.from_numpy(x[:, :cols].astype(np.float32))
    clean = torch.where(torch.isnan(t), torch.full_like(t, -float("inf")), t)
    mx = clean.max(dim=1, keepdim=True).values
    first = (clean == mx).int().argmax(dim=1)
    want = torch.where(torch.isinf(mx[:, 0]) & (mx[:, 0] < 0), torch.zeros_like(first), first)
    assert np.array_equal(got, want.numpy().astype(np.int32))
    assert got[4] == 0 and got[5] == 0 and got[6] == 0 and got[7] == cols - 1 and got[2] == 0
    assert got[8] == (cols - 2 if cols > 1 else 0)
