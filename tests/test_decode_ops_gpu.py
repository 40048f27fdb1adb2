"""Operator-level tests of the decode-side kernels (decode.hip) on the MI355X: rope_kv_append, the three cached-attention kernels
(un-fused, fused, split-KV pair), perceiver_attention, embed_rows and argmax_rows_lp, each driven alone through its vstar_vqa_op_*
door against tests/_decode_ops_ref.py (pinned on the CPU by tests/test_decode_ops_ref.py, which also asserts every condition of the
input builders used here).

Conventions of every test:
  * every index array enters the door as a HOST array and is checked there against the extents; every index a correct kernel touches
    lies inside the allocations made here, which have exactly the extents the door is told;
  * outputs are pre-filled with a sentinel (fp16 NaN); padding rows, the two rows behind the output and every cache row that no row of
    the call writes must come back bit-unchanged;
  * EXACT = equal bits.  One-hot probes: the reference's probabilities are exactly one-hot, so the output IS the target's value row.
  * TIGHT (exact-dot inputs: scores determined bit for bit) = |got - ref| <= 2^-10 |ref| + 2^-9 sum p|v| + 2^-23 sum |v|;
    LOOSE (random inputs) = TIGHT + (e^(2 delta) - 1) sum p|v|, delta from the reference's scores (_decode_ops_ref.attn_row).
    Each prints one `DECODEOP_ERR` line with the measured error and its share of the gate (run with -s to record them).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _decode_ops_ref as R
from vstar_amd._lib import VqaKvRows, VqaKvView

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
HP = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731


def ok(lib, rc):
    assert rc == 0, lib.vstar_vqa_last_error(None)


def refused(lib, rc):
    assert rc == ERR_INVALID, rc
    assert lib.vstar_vqa_last_error(None)


def need_split():
    v = os.environ.get("VSTAR_DECODE_SPLIT_KV")
    if v is not None and v.lstrip("+-").isdigit() and int(v) == 0:
        pytest.skip("VSTAR_DECODE_SPLIT_KV=0 turns the split-KV path off: the door refuses path 2")


def to_dev(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def host(t):
    return None if t is None else t.cpu().numpy()


def sentinel(cuda, rows, cols):
    return torch.full((rows, cols), float("nan"), dtype=torch.float16, device=cuda)


def same(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


class DevCase:
    """A Case on the device: the packed caches, qkv, the table, a sentinel-filled output with two rows behind it, and the door's
    two structs over host index arrays that live as long as this object."""

    def __init__(self, cuda, c: R.Case):
        self.c = c
        self.k0, self.ks0 = R.pack_cache(c.K, c.fmt)
        self.v0, self.vs0 = R.pack_cache(c.V, c.fmt)
        self.k, self.v, self.ks, self.vs = (to_dev(cuda, a) for a in (self.k0, self.v0, self.ks0, self.vs0))
        self.qkv, self.table = to_dev(cuda, c.qkv), to_dev(cuda, c.table)
        self.out = sentinel(cuda, c.R + 2, c.H * 128)
        self.out0 = host(self.out)
        self.view = VqaKvView(c.fmt, c.H, c.ctx, c.slots, P(self.k), P(self.v), P(self.ks), P(self.vs))
        self.idx = {n: np.ascontiguousarray(getattr(c, n), np.int32) for n in ("row_seq", "row_pos", "row_slot", "seq_kv", "seq_prefix", "seq_past")}
        self.idx["anc"] = None if c.anc is None else np.ascontiguousarray(c.anc, np.int32).reshape(-1)
        self.keep = []
        self.rows = self.make_rows()

    def make_rows(self, **over):
        a = dict(self.idx, **over)
        self.keep.append(a)                 # (the struct holds bare pointers)
        n_rows = len(a["row_pos"] if a["row_pos"] is not None else self.idx["row_pos"])
        return VqaKvRows(n_rows, len(a["seq_kv"]), *(HP(a[n]) for n in ("row_seq", "row_pos", "row_slot", "seq_kv", "seq_prefix", "seq_past", "anc")))

    def attention(self, lib, path=None, repeat=1, max_keys=None, rows=None, view=None, table_rows=None):
        ran = ctypes.c_int(-7)
        rc = lib.vstar_vqa_op_cached_attention(P(self.qkv), P(self.table), self.c.ctx if table_rows is None else table_rows,
                                               ctypes.byref(view or self.view), ctypes.byref(rows or self.rows),
                                               self.c.max_keys if max_keys is None else max_keys, self.c.path if path is None else path, repeat,
                                               P(self.out), ctypes.byref(ran))
        return rc, ran.value

    def append(self, lib, rows=None, view=None, table_rows=None):
        return lib.vstar_vqa_op_rope_kv_append(P(self.qkv), P(self.table), self.c.ctx if table_rows is None else table_rows,
                                               ctypes.byref(view or self.view), ctypes.byref(rows or self.rows))

    def output(self):
        """[R, H, 128] after checking that the padding rows and the rows behind the output kept their sentinel."""
        got = host(self.out)
        keep = np.ones(self.c.R + 2, bool)
        keep[: self.c.R] = self.c.row_pos < 0
        assert same(got[keep], self.out0[keep]), "a padding row or a row behind the output was written"
        return got[: self.c.R].reshape(self.c.R, self.c.H, 128)

    def check_caches(self, raw_k=None, raw_v=None, written=None):
        """The caches after the call, bit for bit: the written rows from the quantiser's input rows, everything else unchanged."""
        if written is None:
            written = np.zeros((self.c.slots, self.c.H, self.c.ctx), bool)
            raw_k, raw_v = self.c.K, self.c.V
        for name, dev, dsc, b0, s0, raw in (("K", self.k, self.ks, self.k0, self.ks0, raw_k), ("V", self.v, self.vs, self.v0, self.vs0, raw_v)):
            want, want_s = R.cache_image_after(b0, s0, raw, written, self.c.fmt)
            got = host(dev)
            assert same(got[~written], want[~written]), f"{name}: a cache row no row of the call writes has changed"
            assert same(got, want), f"{name} cache rows"
            if want_s is not None:
                assert same(host(dsc), want_s), f"{name} scale bytes"

    def untouched(self):
        assert same(host(self.out), self.out0) and same(host(self.qkv), self.c.qkv)
        self.check_caches()


def gate_check(name, got, ref, gate, kind):
    """|got - ref| <= gate elementwise; prints the recorded-error line first."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    share = err / gate
    print(f"DECODEOP_ERR {name}: abs {err.max():.3e} rel {err.max() / max(np.abs(ref).max(), 1e-30):.3e} "
          f"worst err/gate {share.max():.3f} [{kind}]")
    assert np.isfinite(got).all()
    assert (err <= gate).all(), float(share.max())


def run_attention_case(lib, cuda, c, ref, path=None, repeat=1):
    """One launch of a case: path_ran, qkv unchanged, caches as the reference leaves them; returns the live rows' output."""
    d = DevCase(cuda, c)
    path = c.path if path is None else path
    rc, ran = d.attention(lib, path=path, repeat=repeat)
    ok(lib, rc)
    assert ran == path
    assert same(host(d.qkv), c.qkv)
    if path >= 1:
        d.check_caches(ref.append.K_raw, ref.append.V_raw, ref.append.written)
    else:
        d.check_caches()
    return d.output()


# ================================================================ rope_kv_append
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_rope_kv_append(lib, cuda, H, fmt):
    """EXACT: q rotated in place; k / v in place as rotated (format 0) or round-tripped (formats 1, 2); the cache rows and, in format
    1, their scale bytes; padding rows of qkv and every cache row the call does not write unchanged.  (This is the test that found
    the fp16 contraction of the rotation: one product fused into the sum, q / k one fp16 step off in some elements.)"""
    c = R.append_case(H, fmt)
    ref = R.append_ref(c)
    d = DevCase(cuda, c)
    ok(lib, d.append(lib))
    assert same(host(d.qkv), ref.qkv)
    d.check_caches(ref.K_raw, ref.V_raw, ref.written)
    assert same(host(d.out), d.out0)


# ================================================================ cached attention
@pytest.mark.parametrize("anc", [False, True])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_cached_attention_probes(lib, cuda, path, fmt, anc):
    """EXACT: every round of the one-hot probes returns the target's value row (first / last key of the prefix, of the own slot, of
    every split partition, the own key); the fused paths leave the own K / V row in the cache; path 2 with repeat = 2 is repeat = 1."""
    if path == 2:
        need_split()
    for gi, g in enumerate(R.cases_geometry(path, anc=anc)):
        for t in range(R.probe_rounds(path, g)):
            c = R.probe_case(path, fmt, g, t)
            ref = R.attention_ref(c)
            got = run_attention_case(lib, cuda, c, ref, repeat=2 if (path == 2 and t % 2) else 1)
            live = ref.valid
            assert same(got[live], ref.out[live]), f"{c.name} geometry {gi}: targets {c.targets.tolist()}"
            if path == 2 and t == 0:
                again = run_attention_case(lib, cuda, c, ref, repeat=2)
                assert same(again, got)


@pytest.mark.parametrize("anc", [False, True])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_cached_attention_exact_dot(lib, cuda, path, anc):
    """TIGHT on inputs whose scores are determined bit for bit; format 1 == format 2 bit for bit; path 2 and path 1 both meet TIGHT on
    the same inputs, and path 2 with repeat = 2 is repeat = 1."""
    if path == 2:
        need_split()
    g = R.cases_geometry(path, which=None if path == 0 else 1, anc=anc)[0]
    outs = {}
    for fmt in (0, 1, 2):
        c = R.exact_dot_case(path, fmt, g)
        ref = R.attention_ref(c)
        live = ref.valid
        outs[fmt] = run_attention_case(lib, cuda, c, ref)[live]
        gate_check(f"exact-dot path {path} fmt {fmt} anc {int(anc)}", outs[fmt], ref.out[live], ref.tight[live], "TIGHT")
        if path == 2:
            assert same(run_attention_case(lib, cuda, c, ref, repeat=2)[live], outs[fmt])
            one = run_attention_case(lib, cuda, c, ref, path=1)[live]
            gate_check(f"exact-dot path 1 on path 2's inputs fmt {fmt} anc {int(anc)}", one, ref.out[live], ref.tight[live], "TIGHT")
    assert same(outs[1], outs[2])


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_cached_attention_random(lib, cuda, path, fmt):
    """LOOSE: the real table, qkv and caches 0.5 x normal; finite outputs."""
    if path == 2:
        need_split()
    g = R.cases_geometry(path, which=None if path == 0 else 1)[0]
    c = R.random_case(path, fmt, g)
    ref = R.attention_ref(c)
    live = ref.valid
    got = run_attention_case(lib, cuda, c, ref)[live]
    gate_check(f"random path {path} fmt {fmt}", got, ref.out[live], ref.loose[live], "LOOSE")


# ================================================================ Perceiver attention
def run_perceiver(lib, cuda, q, kv, n, L, NK, H, DH):
    dq, dkv = to_dev(cuda, q), to_dev(cuda, kv)
    out = sentinel(cuda, n * L + 2, H * DH)
    ok(lib, lib.vstar_vqa_op_perceiver_attention(P(dq), P(dkv), P(out), n, L, NK, H, DH))
    got = host(out)
    assert np.isnan(got[n * L:]).all(), "rows behind the output were written"
    return got[: n * L]


@pytest.mark.parametrize("DH", R.PERCEIVER_DH)
@pytest.mark.parametrize("n,H,L,NK", R.PERCEIVER_SHAPES)
def test_perceiver_attention(lib, cuda, n, H, L, NK, DH):
    """One-hot probes EXACT, exact-dot TIGHT, random LOOSE; n * H * L is no multiple of 4 in four of the five shapes (idle waves in the
    last block)."""
    q, kv, _ = R.perceiver_probe(n, H, L, NK, DH, 3)
    ref = R.perceiver_ref(q, kv, n, L, NK, H, DH)
    assert same(run_perceiver(lib, cuda, q, kv, n, L, NK, H, DH), ref.out)
    shape = f"n {n} H {H} L {L} NK {NK} DH {DH}"
    q, kv = R.perceiver_exact(n, H, L, NK, DH, 4)
    ref = R.perceiver_ref(q, kv, n, L, NK, H, DH)
    gate_check(f"perceiver exact-dot {shape}", run_perceiver(lib, cuda, q, kv, n, L, NK, H, DH), ref.out, ref.tight, "TIGHT")
    q, kv = R.perceiver_random(n, H, L, NK, DH, 5)
    ref = R.perceiver_ref(q, kv, n, L, NK, H, DH)
    gate_check(f"perceiver random {shape}", run_perceiver(lib, cuda, q, kv, n, L, NK, H, DH), ref.out, ref.loose, "LOOSE")


# ================================================================ embed_rows / argmax_rows_lp
@pytest.mark.parametrize("C", [8, 264])
def test_embed_rows(lib, cuda, C):
    """EXACT on distinct codes: token ids, feature rows, INT32_MIN, ids >= vocab and feature indices >= n_feat_rows (zero rows)."""
    src, table, feats = R.embed_case(C)
    dt, df = to_dev(cuda, table), to_dev(cuda, feats)
    out = sentinel(cuda, len(src) + 2, C)
    ok(lib, lib.vstar_vqa_op_embed_rows(HP(src), len(src), P(dt), len(table), P(df), len(feats), P(out), C))
    got = host(out)
    assert np.isnan(got[len(src):]).all()
    assert same(got[: len(src)], R.embed_rows(src, table, feats))


@pytest.mark.parametrize("cols", R.ARGMAX_COLS)
def test_argmax_rows(lib, cuda, cols):
    """EXACT: the first index of the largest number; the padding columns hold the largest value and never win; NaN never wins; rows
    of only NaN and / or -inf return 0."""
    x, ld = R.argmax_case(cols)
    dx = to_dev(cuda, x)
    out = np.full(len(x) + 2, -77, np.int32)
    ok(lib, lib.vstar_vqa_op_argmax_rows(P(dx), len(x), cols, ld, HP(out)))
    assert (out[len(x):] == -77).all()
    assert np.array_equal(out[: len(x)], R.argmax_rows(x[:, :cols]))


# ================================================================ refusals
def test_kv_doors_refuse_bad_index_arrays(lib, cuda):
    """Every rule on the index arrays and extents: VSTAR_ERR_INVALID with a message, output, qkv and caches bit-unchanged (nothing is
    launched)."""
    c = R.random_case(0, 1, R.geometry(0, anc=True))
    d = DevCase(cuda, c)
    live = int(np.nonzero(c.row_pos >= 0)[0][0])
    seq = int(c.row_seq[live])

    def edit(name, i, value):
        a = d.idx[name].copy()
        a[i] = value
        return d.make_rows(**{name: a})

    def view(**over):
        f = dict(fmt=c.fmt, heads=c.H, ctx=c.ctx, slots=c.slots, dev_k=P(d.k), dev_v=P(d.v), dev_ks=P(d.ks), dev_vs=P(d.vs))
        f.update(over)
        return VqaKvView(*(f[n] for n in ("fmt", "heads", "ctx", "slots", "dev_k", "dev_v", "dev_ks", "dev_vs")))

    bad_rows = [edit("row_pos", live, -2), edit("row_pos", live, c.ctx), edit("row_slot", live, c.slots), edit("row_slot", 0, -1),
                edit("row_seq", live, c.n_seq), edit("row_seq", 0, -1), edit("seq_kv", seq, c.slots), edit("seq_kv", 0, -1),
                edit("seq_prefix", seq, c.slots), edit("seq_prefix", 0, -1), edit("seq_past", seq, -1),
                edit("seq_past", seq, int(c.row_pos[live]) + 1), edit("anc", 5, c.slots), edit("anc", c.slots * c.ctx - 1, -1),
                d.make_rows(row_pos=None), d.make_rows(seq_past=None)]
    bad_views = [view(fmt=3), view(fmt=-1), view(dev_ks=None), view(dev_vs=None), view(dev_k=None), view(dev_v=None), view(slots=0),
                 view(heads=0), view(ctx=0)]
    for rows in bad_rows:
        refused(lib, d.attention(lib, rows=rows)[0])
        refused(lib, d.append(lib, rows=rows))
    for v in bad_views:
        refused(lib, d.attention(lib, view=v)[0])
        refused(lib, d.append(lib, view=v))
    top = int(c.row_pos.max())
    refused(lib, d.attention(lib, table_rows=top)[0])                  # row_pos < table_rows
    refused(lib, d.append(lib, table_rows=top))
    refused(lib, d.attention(lib, max_keys=top)[0])                    # row_pos + 1 <= max_keys
    refused(lib, d.attention(lib, max_keys=c.ctx + 1)[0])              # max_keys <= ctx
    refused(lib, d.attention(lib, path=3)[0])
    refused(lib, d.attention(lib, path=-1)[0])
    refused(lib, d.attention(lib, repeat=0)[0])
    ran = ctypes.c_int(-7)
    args = (c.ctx, ctypes.byref(d.view), ctypes.byref(d.make_rows()), c.max_keys, 0, 1)
    refused(lib, lib.vstar_vqa_op_cached_attention(None, P(d.table), *args, P(d.out), ctypes.byref(ran)))
    refused(lib, lib.vstar_vqa_op_cached_attention(P(d.qkv), P(d.table), *args, None, ctypes.byref(ran)))
    refused(lib, lib.vstar_vqa_op_cached_attention(P(d.qkv), P(d.table), *args, P(d.out), None))
    refused(lib, lib.vstar_vqa_op_cached_attention(P(d.qkv), P(d.table), c.ctx, None, ctypes.byref(d.make_rows()), c.max_keys, 0, 1, P(d.out),
                                                   ctypes.byref(ran)))
    refused(lib, lib.vstar_vqa_op_cached_attention(P(d.qkv), P(d.table), c.ctx, ctypes.byref(d.view), None, c.max_keys, 0, 1, P(d.out),
                                                   ctypes.byref(ran)))
    refused(lib, lib.vstar_vqa_op_rope_kv_append(None, P(d.table), c.ctx, ctypes.byref(d.view), ctypes.byref(d.make_rows())))
    refused(lib, lib.vstar_vqa_op_rope_kv_append(P(d.qkv), None, c.ctx, ctypes.byref(d.view), ctypes.byref(d.make_rows())))
    assert ran.value == -7
    d.untouched()


def test_fused_paths_refuse_what_they_cannot_run(lib, cuda):
    """Paths 1 and 2: padding rows, two rows of one sequence, a repeated seq_kv, a row_slot that is not the sequence's slot, a null
    table; path 2 outside the split-KV domain (max_keys < 256, R * heads > 128) is an error, never a fall-back."""
    c = R.random_case(2, 0, R.cases_geometry(2, which=1)[0])
    d = DevCase(cuda, c)

    def edit(**over):
        return d.make_rows(**{n: np.asarray(v, np.int32) for n, v in over.items()})

    other = [s for s in range(c.slots) if s not in c.seq_kv.tolist()][0]
    for path in (1, 2):
        refused(lib, d.attention(lib, path=path, rows=edit(row_pos=[c.row_pos[0], -1, c.row_pos[2]]))[0])
        refused(lib, d.attention(lib, path=path, rows=edit(row_seq=[c.row_seq[0], c.row_seq[0], c.row_seq[2]]))[0])
        refused(lib, d.attention(lib, path=path, rows=edit(row_seq=list(c.row_seq) + [c.row_seq[0]], row_pos=list(c.row_pos) + [7],
                                                           row_slot=list(c.row_slot) + [c.row_slot[0]]))[0])
        dup = c.seq_kv.copy()
        dup[1] = dup[0]
        refused(lib, d.attention(lib, path=path, rows=edit(seq_kv=dup, row_slot=dup[c.row_seq]))[0])
        slot = c.row_slot.copy()
        slot[0] = other
        refused(lib, d.attention(lib, path=path, rows=edit(row_slot=slot))[0])
        ran = ctypes.c_int(-7)
        refused(lib, lib.vstar_vqa_op_cached_attention(P(d.qkv), None, c.ctx, ctypes.byref(d.view), ctypes.byref(d.make_rows()), c.max_keys, path, 1,
                                                       P(d.out), ctypes.byref(ran)))
    low = edit(row_pos=[100, 7, 254])
    refused(lib, d.attention(lib, path=2, rows=low, max_keys=255)[0])  # one key short of the split domain
    d.untouched()
    # R * heads = 129: a cache of 43 heads with exactly the extents the door is told
    H = 43
    big = R.Case(2, 0, H, 256, 4, c.row_seq, np.array([255, 9, 100], np.int32), c.row_slot, c.seq_kv, c.seq_kv.copy(), np.zeros(3, np.int32),
                 R.identity_table(256), np.zeros((3, 3 * H * 128), np.float16), np.ones((4, H, 256, 128), np.float16),
                 np.ones((4, H, 256, 128), np.float16), max_keys=256)
    db = DevCase(cuda, big)
    refused(lib, db.attention(lib, path=2)[0])
    db.untouched()


def test_unsplit_paths_refuse_more_keys_than_lds(lib, cuda):
    """(128 + max_keys) * 4 > 40 KiB on paths 0 and 1: max_keys = 10113 over a cache that really has that many positions."""
    ctx = 10113
    zero = np.zeros(1, np.int32)
    c = R.Case(0, 0, 1, ctx, 1, zero, np.array([5], np.int32), zero, zero, zero, zero, R.identity_table(ctx), np.ones((1, 3 * 128), np.float16),
               np.ones((1, 1, ctx, 128), np.float16), np.ones((1, 1, ctx, 128), np.float16), max_keys=ctx)
    d = DevCase(cuda, c)
    refused(lib, d.attention(lib, path=0)[0])
    refused(lib, d.attention(lib, path=1)[0])
    d.untouched()
    rc, ran = d.attention(lib, path=0, max_keys=ctx - 1)               # the largest call the kernel takes
    ok(lib, rc)
    ref = R.attention_ref(c)
    assert ran == 0 and ref.exact_dots
    gate_check("path 0 at the LDS limit", d.output(), ref.out, ref.tight, "TIGHT")


def test_small_doors_refuse_bad_arguments(lib, cuda):
    """Perceiver: DH outside {32, 64, 96}, NK outside [1, 512]; embed: C % 8 != 0; argmax: ld < cols; null pointers.  Outputs keep
    their sentinel."""
    q, kv = R.perceiver_random(1, 1, 3, 4, 32, 0)
    dq, dkv = to_dev(cuda, q), to_dev(cuda, kv)
    out = sentinel(cuda, 5, 32)
    for DH, NK in ((48, 4), (128, 4), (32, 0), (32, 513), (32, -1)):
        refused(lib, lib.vstar_vqa_op_perceiver_attention(P(dq), P(dkv), P(out), 1, 3, NK, 1, DH))
    refused(lib, lib.vstar_vqa_op_perceiver_attention(None, P(dkv), P(out), 1, 3, 4, 1, 32))
    refused(lib, lib.vstar_vqa_op_perceiver_attention(P(dq), None, P(out), 1, 3, 4, 1, 32))
    refused(lib, lib.vstar_vqa_op_perceiver_attention(P(dq), P(dkv), None, 1, 3, 4, 1, 32))
    refused(lib, lib.vstar_vqa_op_perceiver_attention(P(dq), P(dkv), P(out), 0, 3, 4, 1, 32))
    src, table, feats = R.embed_case(8)
    dt, df = to_dev(cuda, table), to_dev(cuda, feats)
    refused(lib, lib.vstar_vqa_op_embed_rows(HP(src), len(src), P(dt), len(table), P(df), len(feats), P(out), 12))
    refused(lib, lib.vstar_vqa_op_embed_rows(HP(src), len(src), P(dt), len(table), P(df), len(feats), P(out), 0))
    refused(lib, lib.vstar_vqa_op_embed_rows(None, len(src), P(dt), len(table), P(df), len(feats), P(out), 8))
    refused(lib, lib.vstar_vqa_op_embed_rows(HP(src), len(src), None, len(table), P(df), len(feats), P(out), 8))
    refused(lib, lib.vstar_vqa_op_embed_rows(HP(src), len(src), P(dt), len(table), None, len(feats), P(out), 8))
    refused(lib, lib.vstar_vqa_op_embed_rows(HP(src), len(src), P(dt), len(table), P(df), len(feats), None, 8))
    res = np.full(4, -77, np.int32)
    refused(lib, lib.vstar_vqa_op_argmax_rows(P(out), 4, 32, 31, HP(res)))
    refused(lib, lib.vstar_vqa_op_argmax_rows(P(out), 4, 0, 32, HP(res)))
    refused(lib, lib.vstar_vqa_op_argmax_rows(None, 4, 32, 32, HP(res)))
    refused(lib, lib.vstar_vqa_op_argmax_rows(P(out), 4, 32, 32, None))
    assert np.isnan(host(out)).all() and (res == -77).all()
