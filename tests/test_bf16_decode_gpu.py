"""Operator-level tests of the bf16 DECODE kernels on the MI355X — the bf16 build of decode.hip (rope_kv_append, the three
cached-attention paths, embed_rows, argmax_rows_lp) and of skinny.hip (gemm_skinny_kernel, gemm_skinny_ring_kernel; fused RMSNorm,
fp32 output, the tile-major weight image) that vstar_vsm_generate and the batched contextual-cue decode run — each driven alone
through its vstar_op_* door against tests/_bf16_decode_ref.py (pinned on the CPU by tests/test_bf16_decode_ref.py, which also asserts
every condition of the input builders used here).

Conventions of every test:
  * every index array enters a door as a HOST array and is checked there against the extents; every index a correct kernel touches
    lies inside the allocations made here, which have exactly the extents the door is told (W: rows padded to 256, the library's
    contract);
  * outputs are pre-filled with a sentinel NaN pattern; padding rows, the two rows behind every output and every cache row that no
    row of the call writes must come back bit-unchanged;
  * EXACT = equal bits.  TIGHT / LOOSE: the gates of _bf16_decode_ref (u = 2^-8).  Each gated attention case prints one
    `BF16DEC_ERR` line with the measured error and its share of the gate (run with -s to record them);
  * every GEMV call asserts which kernel ran (kernel_ran), every attention call which path (path_ran);
  * VSTAR_SKINNY_RING, VSTAR_DECODE_SPLIT_KV and VSTAR_DECODE_TILED are never set here (they are read once per process).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _bf16_decode_ref as B
from tests import _decode_ops_ref as R
from tests import _gemm128_ref as G
from vstar_amd._lib import VqaKvRows, VqaKvView

pytestmark = pytest.mark.gpu

ERR_INVALID = -1
ATT = "vstar_op_cached_attention"
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
HP = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731


def ok(lib, rc):
    assert rc == 0, lib.vstar_last_error(None)


def refused(lib, rc, door):
    """VSTAR_ERR_INVALID with a message of THIS door: every door prefixes its message with its own name, so a door that returned
    the code without writing a message would show the text of the door refused before it."""
    assert rc == ERR_INVALID, rc
    msg = lib.vstar_last_error(None).decode()
    assert msg.startswith(door + ": ") and len(msg) > len(door) + 2, (door, msg)


def need_split():
    v = os.environ.get("VSTAR_DECODE_SPLIT_KV")
    if v is not None and v.lstrip("+-").isdigit() and int(v) == 0:
        pytest.skip("VSTAR_DECODE_SPLIT_KV=0 turns the split-KV path off: the door refuses path 2")


def nan_bits(x):
    """bits() of float32-held bf16 values that may hold NaN / inf."""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def dev16(cuda, x):
    """float32-held bf16 values -> their 16-bit patterns on the device."""
    return None if x is None else torch.from_numpy(nan_bits(x).view(np.int16)).to(cuda)


def host16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def as_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def sent16(cuda, rows, cols):
    return torch.full((rows, cols), B.SENT16 - 65536 if B.SENT16 >= 32768 else B.SENT16, dtype=torch.int16, device=cuda)


def sent32(cuda, rows, cols):
    return torch.full((rows, cols), B.SENT32, dtype=torch.int32, device=cuda)


class DevCase:
    """A bf16 Case on the device: the caches, qkv, the table, a sentinel-filled output with two rows behind it, and the door's two
    structs over host index arrays that live as long as this object."""

    def __init__(self, cuda, c: R.Case):
        assert c.fmt == 0 and c.st is B.BF16
        self.c = c
        self.k0, self.v0, self.qkv0 = B.bits(c.K), B.bits(c.V), B.bits(c.qkv)
        self.k, self.v, self.table = (dev16(cuda, a) for a in (c.K, c.V, c.table))
        self.qkv = sent16(cuda, c.R + 2, c.qkv.shape[1])          # the in-place output of rope_kv_append: two rows behind it as well
        self.qkv[: c.R] = dev16(cuda, c.qkv)
        self.out = sent16(cuda, c.R + 2, c.H * 128)
        self.view = VqaKvView(0, c.H, c.ctx, c.slots, P(self.k), P(self.v), None, None)
        self.idx = {n: np.ascontiguousarray(getattr(c, n), np.int32) for n in ("row_seq", "row_pos", "row_slot", "seq_kv", "seq_prefix", "seq_past")}
        self.idx["anc"] = None if c.anc is None else np.ascontiguousarray(c.anc, np.int32).reshape(-1)
        self.keep = []
        self.rows = self.make_rows()

    def make_rows(self, **over):
        a = dict(self.idx, **over)
        self.keep.append(a)                 # (the struct holds bare pointers)
        n_rows = len(a["row_pos"] if a["row_pos"] is not None else self.idx["row_pos"])
        return VqaKvRows(n_rows, len(a["seq_kv"]), *(HP(a[n]) for n in ("row_seq", "row_pos", "row_slot", "seq_kv", "seq_prefix", "seq_past", "anc")))

    def make_view(self, **over):
        f = dict(fmt=0, heads=self.c.H, ctx=self.c.ctx, slots=self.c.slots, dev_k=P(self.k), dev_v=P(self.v), dev_ks=None, dev_vs=None)
        f.update(over)
        return VqaKvView(*(f[n] for n in ("fmt", "heads", "ctx", "slots", "dev_k", "dev_v", "dev_ks", "dev_vs")))

    def attention(self, lib, path=None, repeat=1, max_keys=None, rows=None, view=None, table_rows=None):
        ran = ctypes.c_int(-7)
        rc = lib.vstar_op_cached_attention(P(self.qkv), P(self.table), self.c.ctx if table_rows is None else table_rows,
                                           ctypes.byref(view or self.view), ctypes.byref(rows or self.rows),
                                           self.c.max_keys if max_keys is None else max_keys, self.c.path if path is None else path, repeat,
                                           P(self.out), ctypes.byref(ran))
        return rc, ran.value

    def append(self, lib, rows=None, view=None, table_rows=None):
        return lib.vstar_op_rope_kv_append(P(self.qkv), P(self.table), self.c.ctx if table_rows is None else table_rows,
                                           ctypes.byref(view or self.view), ctypes.byref(rows or self.rows))

    def output(self):
        """[R, H, 128] bit patterns after checking that the padding rows and the rows behind the output kept their sentinel."""
        got = host16(self.out)
        keep = np.ones(self.c.R + 2, bool)
        keep[: self.c.R] = self.c.row_pos < 0
        assert (got[keep] == B.SENT16).all(), "a padding row or a row behind the output was written"
        return got[: self.c.R].reshape(self.c.R, self.c.H, 128)

    def check_caches(self, raw_k=None, raw_v=None, written=None):
        """The caches after the call, bit for bit: the written rows hold the reference's rows, everything else is unchanged."""
        if written is None:
            written = np.zeros((self.c.slots, self.c.H, self.c.ctx), bool)
            raw_k, raw_v = self.c.K, self.c.V
        for name, dev, b0, raw in (("K", self.k, self.k0, raw_k), ("V", self.v, self.v0, raw_v)):
            want = b0.copy()
            want[written] = B.bits(raw)[written]
            got = host16(dev)
            assert np.array_equal(got[~written], want[~written]), f"{name}: a cache row no row of the call writes has changed"
            assert np.array_equal(got, want), f"{name} cache rows"

    def qkv_bits(self):
        """[R, 3 H 128] bit patterns after checking that the two rows behind qkv kept their sentinel."""
        got = host16(self.qkv)
        assert (got[self.c.R:] == B.SENT16).all(), "a row behind qkv was written"
        return got[: self.c.R]

    def untouched(self):
        assert (host16(self.out) == B.SENT16).all() and np.array_equal(self.qkv_bits(), self.qkv0)
        self.check_caches()


_worst = {}


def gate_check(family, name, got_bits, ref, gate, kind):
    """|got - ref| <= gate elementwise; prints the recorded-error line first."""
    got, ref = as_f32(got_bits).astype(np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    share = err / gate
    _worst[family] = max(_worst.get(family, 0.0), float(share.max()))
    print(f"BF16DEC_ERR {name}: abs {err.max():.3e} rel {err.max() / max(np.abs(ref).max(), 1e-30):.3e} "
          f"worst err/gate {share.max():.3f} [{kind}] (family {family}: worst so far {_worst[family]:.3f})")
    assert np.isfinite(got).all()
    assert (err <= gate).all(), float(share.max())


def run_attention_case(lib, cuda, c, ref, path=None, repeat=1):
    """One launch of a case: path_ran, qkv unchanged, caches as the reference leaves them; returns the output's bit patterns."""
    d = DevCase(cuda, c)
    path = c.path if path is None else path
    rc, ran = d.attention(lib, path=path, repeat=repeat)
    ok(lib, rc)
    assert ran == path
    assert np.array_equal(d.qkv_bits(), d.qkv0)
    if path >= 1:
        d.check_caches(ref.append.K_raw, ref.append.V_raw, ref.append.written)
    else:
        d.check_caches()
    return d.output()


# ================================================================ rope_kv_append
@pytest.mark.parametrize("table", ["llama", "grid"])
@pytest.mark.parametrize("H", [1, 3])
def test_rope_kv_append(lib, cuda, H, table):
    """EXACT: q and k rotated in place, v untouched, the cache rows written; padding rows of qkv and every cache row the call does
    not write unchanged.  The real LLaMA table in bf16 and the grid table."""
    c = B.append_case(H, table)
    ref = R.append_ref(c)
    d = DevCase(cuda, c)
    ok(lib, d.append(lib))
    assert np.array_equal(d.qkv_bits(), B.bits(ref.qkv))
    d.check_caches(ref.K_raw, ref.V_raw, ref.written)
    assert (host16(d.out) == B.SENT16).all()


# ================================================================ cached attention
@pytest.mark.parametrize("anc", [False, True])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_cached_attention_probes(lib, cuda, path, anc):
    """EXACT: every round of the one-hot probes returns the target's value row (first / last key of the prefix, of the own slot, of
    every split partition, the own key); the fused paths leave the own K / V row in the cache; path 2 with repeat = 2 is repeat = 1."""
    if path == 2:
        need_split()
    for gi, g in enumerate(R.cases_geometry(path, anc=anc)):
        for t in range(R.probe_rounds(path, g)):
            c = B.probe_case(path, g, t)
            ref = R.attention_ref(c)
            got = run_attention_case(lib, cuda, c, ref, repeat=2 if (path == 2 and t % 2) else 1)
            live = ref.valid
            assert np.array_equal(got[live], B.bits(ref.out[live])), f"{c.name} geometry {gi}: targets {c.targets.tolist()}"
            if path == 2 and t == 0:
                again = run_attention_case(lib, cuda, c, ref, repeat=2)
                assert np.array_equal(again, got)


@pytest.mark.parametrize("anc", [False, True])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_cached_attention_exact_dot(lib, cuda, path, anc):
    """TIGHT on inputs whose scores are determined bit for bit; path 2 and path 1 both meet TIGHT on the same inputs, and path 2 with
    repeat = 2 is repeat = 1 bit for bit."""
    if path == 2:
        need_split()
    g = R.cases_geometry(path, which=None if path == 0 else 1, anc=anc)[0]
    c = B.exact_dot_case(path, g)
    ref = R.attention_ref(c)
    live = ref.valid
    out = run_attention_case(lib, cuda, c, ref)[live]
    gate_check(f"exact-dot path {path}", f"exact-dot path {path} anc {int(anc)}", out, ref.out[live], ref.tight[live], "TIGHT")
    if path == 2:
        assert np.array_equal(run_attention_case(lib, cuda, c, ref, repeat=2)[live], out)
        one = run_attention_case(lib, cuda, c, ref, path=1)[live]
        gate_check("exact-dot path 1 on path 2's inputs", f"exact-dot path 1 on path 2's inputs anc {int(anc)}", one, ref.out[live],
                   ref.tight[live], "TIGHT")


@pytest.mark.parametrize("path", [0, 1, 2])
def test_cached_attention_random(lib, cuda, path):
    """LOOSE: the real table, qkv and caches 0.5 x normal; finite outputs."""
    if path == 2:
        need_split()
    g = R.cases_geometry(path, which=None if path == 0 else 1)[0]
    c = B.random_case(path, g)
    ref = R.attention_ref(c)
    live = ref.valid
    got = run_attention_case(lib, cuda, c, ref)[live]
    gate_check(f"random path {path}", f"random path {path}", got, ref.out[live], ref.loose[live], "LOOSE")


# ================================================================ embed_rows / argmax_rows_lp
@pytest.mark.parametrize("C", [8, 264])
def test_embed_rows(lib, cuda, C):
    """EXACT on distinct codes: token ids, feature rows, INT32_MIN, ids >= vocab and feature indices >= n_feat_rows (zero rows)."""
    src, table, feats = R.embed_case(C, st=B.BF16)
    dt, df = dev16(cuda, table), dev16(cuda, feats)
    out = sent16(cuda, len(src) + 2, C)
    ok(lib, lib.vstar_op_embed_rows(HP(src), len(src), P(dt), len(table), P(df), len(feats), P(out), C))
    got = host16(out)
    assert (got[len(src):] == B.SENT16).all()
    assert np.array_equal(got[: len(src)], B.bits(R.embed_rows(src, table, feats)))


@pytest.mark.parametrize("cols", R.ARGMAX_COLS)
def test_argmax_rows(lib, cuda, cols):
    """EXACT.  The fp16 cases in bf16: the first index of the largest number, the padding columns hold the largest value and never
    win, NaN never wins, rows of only NaN and / or -inf return 0.  What only bf16 can hold: a row whose largest value is finite and
    <= -3e38 at a column > 0 returns 0 (kernels.hpp), a row whose largest value is the next bf16 number above -3e38 returns its
    column."""
    for x, ld in (R.argmax_case(cols, st=B.BF16), B.argmax_extreme_case(cols)):
        dx = dev16(cuda, x)
        out = np.full(len(x) + 2, -77, np.int32)
        ok(lib, lib.vstar_op_argmax_rows_lp(P(dx), len(x), cols, ld, HP(out)))
        assert (out[len(x):] == -77).all()
        assert np.array_equal(out[: len(x)], R.argmax_rows(x[:, :cols])), (out[: len(x)].tolist(), R.argmax_rows(x[:, :cols]).tolist())


# ================================================================ the weight-streaming GEMV
def ring_enabled():
    v = os.environ.get("VSTAR_SKINNY_RING")          # (never set here; honoured where it comes from outside: atoi(v) != 0)
    if v is None:
        return True
    try:
        return int(v.strip() or 0) != 0
    except ValueError:
        return False


def pad_w(W):
    n = (len(W) + 255) // 256 * 256
    out = np.zeros((n, W.shape[1]), np.float32)
    out[: len(W)] = W
    return out


class Operands:
    """The device copies of one GEMV case, uploaded once per storage type and shared by the kernels (never written).  `door`:
    "bf16" = vstar_op_gemm_skinny, "fp16" = vstar_vqa_op_gemm on the same values (small integers and quarters: exact in both)."""

    def __init__(self, cuda, A, W, bias=None, res=None, norm_w=None, door="bf16"):
        self.M, self.K = A.shape
        self.N = W.shape[0]
        self.door = door
        if door == "bf16":
            up = lambda x: dev16(cuda, x)  # noqa: E731
        else:
            def up(x):
                if x is None:
                    return None
                hx = np.asarray(x, np.float16)
                assert np.array_equal(hx.astype(np.float64), np.asarray(x, np.float64)), "not an fp16 value"
                return torch.from_numpy(np.ascontiguousarray(hx)).to(cuda)
        self.A, self.W, self.bias, self.res, self.norm_w = up(A), up(pad_w(W)), up(bias), up(res), up(norm_w)


def run_gemv(lib, cuda, ops, kernel, epi=B.EPI_NONE, f32=False, bias=False, res=False, norm=False, layout=0, eps=1e-6):
    """One GEMV call over a freshly sentinel-filled C with two rows behind it -> the [M, n_out] bit patterns (uint32 for fp32 output,
    uint16 else), after checking which kernel ran and that the rows behind the output kept their sentinel."""
    M, N, K = ops.M, ops.N, ops.K
    n_out = N // 2 if epi == B.EPI_SILU_MUL else N
    C = (sent32 if f32 else sent16)(cuda, M + 2, n_out)
    args = (P(ops.A), P(ops.W), P(ops.bias if bias else None), P(ops.res if res else None), P(C), M, N, K, epi, kernel)
    nw = P(ops.norm_w if norm else None)
    if ops.door == "bf16":
        ran = ctypes.c_int(-7)
        rc = lib.vstar_op_gemm_skinny(*args, 1 if f32 else 0, nw, eps, layout, ctypes.byref(ran))
        assert rc == 0, lib.vstar_last_error(None)
        want = 2 if (kernel == 1 and ring_enabled() and B.ring_runs(M, K, norm)) else 1
        assert ran.value == want, (ran.value, want, kernel, M, K, norm)
    else:
        assert not f32 and layout == 0
        rc = lib.vstar_vqa_op_gemm(*args, nw, eps)
        assert rc == 0, lib.vstar_vqa_last_error(None)
    got = C.cpu().numpy().view(np.uint32) if f32 else host16(C)
    assert (got[M:] == (B.SENT32 if f32 else B.SENT16)).all(), "a row behind the output was written"
    return got[:M]


def want_bits(C, f32, door="bf16"):
    C = np.ascontiguousarray(np.asarray(C, np.float32))
    if f32:
        return C.view(np.uint32)
    if door == "fp16":
        hx = C.astype(np.float16)
        assert np.array_equal(hx.astype(np.float32), C), "not an fp16 value"
        return hx.view(np.uint16)
    return B.bits(C)


def same(got, want, what):
    bad = np.argwhere(got != want)
    assert not len(bad), (what, len(bad), "first (row, col):", bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def silu_same(got, acc, res, what):
    """SiLU-mul against _gemm128_ref.epilogue: EXACT wherever the gate is >= -87; below, the kernel's sigmoid (v_rcp_f32 of a value
    above 2^126) may flush to zero and the output may lie anywhere between the reference and its residual-only value
    (_bf16_decode_ref.silu_flush_gate: below 1e-34 here)."""
    ref = B.epilogue(acc, B.EPI_SILU_MUL, False, None, res)
    region = B.silu_flush_region(acc)
    want = want_bits(ref, False)
    same(np.where(region, want, got), want, what)
    if region.any():
        err = np.abs(as_f32(got).astype(np.float64) - ref)[region]
        print(f"BF16DEC_ERR gemv silu flush region {what}: {int(region.sum())} outputs, abs {err.max():.3e}, "
              f"worst err/gate {(err / B.silu_flush_gate(acc)[region]).max():.3f} [sigmoid below 2^-126]")
        assert (err <= B.silu_flush_gate(acc)[region]).all()


_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


doors = pytest.mark.parametrize("door", ["bf16", "fp16"])
KERNELS = (1, 3)


# (the fp16 door takes the probe while 2^(K / 64) - 1 is an fp16 number: up to 11 double steps)
@pytest.mark.parametrize("door,M,N,K", [(d, *s) for d in ("bf16", "fp16") for s in B.KSTEP_SHAPES if d == "bf16" or s[2] // 64 <= 11])
def test_gemv_every_double_step_exactly_once(lib, cuda, M, N, K, door):
    """Double step d of 64 k adds exactly 2^d to every output: C == 2^(K / 64) - 1 everywhere iff every double step entered exactly
    once.  fp32 output (bf16 door: the OUT_F32 instantiations), and 16-bit output while the value fits the significand (bf16: 8
    steps; fp16: 11, the weights 2^d themselves being fp16 numbers up to d = 15)."""
    nd = K // 64
    A, W, C = cached(("kstep", M, N, K), lambda: B.ktile_probe(M, N, K))
    ops = Operands(cuda, A, W, door=door)
    outs = [True] + ([False] if nd <= 8 else []) if door == "bf16" else [False]
    for kernel in KERNELS:
        for f32 in outs:
            got = run_gemv(lib, cuda, ops, kernel, f32=f32)
            bad = np.argwhere(got != want_bits(C, f32, door))
            if len(bad):
                r, c = bad[0]
                val = got.view(np.float32)[r, c] if f32 else (as_f32(got)[r, c] if door == "bf16" else got.view(np.float16)[r, c])
                pytest.fail(f"kernel {kernel} f32 {f32}: {len(bad)} outputs, first at ({r}, {c}): {val} instead of {C[r, c]} — as a sum of "
                            f"2^d it names the double steps that entered")


@doors
@pytest.mark.parametrize("M,N,K", B.INDEX_SHAPES)
def test_gemv_index_probe(lib, cuda, M, N, K, door):
    """Every (row, column) receives its own code W[n, (37 r) % K]: the row clamp of ragged row tiles, the N tail inside a 16-column
    workgroup, the W rows padded to 256."""
    p = cached(("index", M, N, K), lambda: B.index_probe(M, N, K))
    ops = Operands(cuda, p.A, p.W, door=door)
    for kernel in KERNELS:
        for f32 in ((True, False) if door == "bf16" else (False,)):
            same(run_gemv(lib, cuda, ops, kernel, f32=f32), want_bits(p.C[:M], f32, door), (door, kernel, f32))


@doors
@pytest.mark.parametrize("M,N,K", B.INT_SHAPES)
def test_gemv_int_operands(lib, cuda, M, N, K, door):
    """Random {-1, 0, 1} operands, VSTAR_EPI_NONE: the integer result in bits, alone and with a bias of quarters and a residual
    (r + n) % 8 (the reference's rounding points: acc + bias -> round; + residual -> round; fp32: nothing rounded)."""
    A, W = cached(("int", M, N, K), lambda: B.int_operands(M, N, K, 11))
    acc = G.product(A, W)
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    ops = Operands(cuda, A, W, bias, res, door=door)
    for kernel in KERNELS:
        for f32 in ((True, False) if door == "bf16" else (False,)):
            for b, r in ((False, False), (True, True)):
                want = B.epilogue(acc, B.EPI_NONE, f32, bias if b else None, res if r else None)
                if door == "fp16":            # the same rounding points in fp16: quarters below 2^11 are exact, nothing is rounded
                    want = acc + (bias[None, :] if b else 0) + (res if r else 0)
                same(run_gemv(lib, cuda, ops, kernel, f32=f32, bias=b, res=r), want_bits(want, f32, door), (door, kernel, f32, b, r))


@pytest.mark.parametrize("epi", [B.EPI_NONE, B.EPI_RELU], ids=["none", "relu"])
@pytest.mark.parametrize("M,N,K", B.INT_SHAPES)
def test_gemv_exact_epilogues(lib, cuda, M, N, K, epi):
    """Integer operands, a bias of quarters, a residual (r + n) % 8, each with and without the other, bf16 and fp32 output: EXACT
    against _gemm128_ref.epilogue, both kernels."""
    A, W = cached(("int", M, N, K), lambda: B.int_operands(M, N, K, 11))
    acc = G.product(A, W)
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    ops = Operands(cuda, A, W, bias, res)
    for kernel in KERNELS:
        for f32 in (True, False):
            for b, r in ((True, False), (False, True), (True, True)):
                want = want_bits(B.epilogue(acc, epi, f32, bias if b else None, res if r else None), f32)
                same(run_gemv(lib, cuda, ops, kernel, epi=epi, f32=f32, bias=b, res=r), want, (kernel, epi, f32, b, r))


@pytest.mark.parametrize("M,N,K", B.SILU_SHAPES)
def test_gemv_silu_mul_int_operands(lib, cuda, M, N, K):
    """SiLU(gate) x up on integer accumulators, packed N (16 gate rows, then their 16 up rows), with and without the residual: EXACT
    against _gemm128_ref.epilogue (bf(silu(bf(gate))) x bf(up) -> round; + residual -> round), both kernels (silu_same: no gate of
    these cases lies below -87)."""
    A, W = cached(("silu", M, N, K), lambda: B.int_operands(M, N, K, 7))
    acc = G.product(A, W)
    res = G.residual_mod8(M, N // 2)
    ops = Operands(cuda, A, W, None, res)
    for kernel in KERNELS:
        for r in (False, True):
            silu_same(run_gemv(lib, cuda, ops, kernel, epi=B.EPI_SILU_MUL, res=r), acc, res if r else None, (kernel, r))


@pytest.mark.parametrize("epi", [B.EPI_QUICK_GELU, B.EPI_GELU], ids=["quick_gelu", "gelu"])
@pytest.mark.parametrize("M,N,K", B.GELU_SHAPES)
def test_gemv_gelu_int_operands(lib, cuda, M, N, K, epi):
    """GELU and quick-GELU on integer accumulators, a bias of quarters and a residual (r + n) % 8, each with and without the other,
    both kernels.  16-bit output: the stored value lies in _bf16_decode_ref.act16_interval — the kernels' rounding points restated,
    the fp32 activation's error carried through the monotone roundings; EXACT (one point) wherever no rounding tie is that near.
    fp32 output (the OUT_F32 instantiations; quick-GELU takes its un-rounded form there): within act32_ref's gate of float64."""
    A, W = cached(("int", M, N, K), lambda: B.int_operands(M, N, K, 11))
    acc = G.product(A, W)
    bias, res = G.bias_quarters(N), G.residual_mod8(M, N)
    ops = Operands(cuda, A, W, bias, res)
    for b, r in ((True, False), (False, True), (True, True)):
        lo, hi = B.act16_interval(acc, epi, bias if b else None, res if r else None)
        ref32, gate32 = B.act32_ref(acc, epi, bias if b else None, res if r else None)
        for kernel in KERNELS:
            got = as_f32(run_gemv(lib, cuda, ops, kernel, epi=epi, bias=b, res=r)).astype(np.float64)
            bad = np.argwhere(~((lo <= got) & (got <= hi)))
            print(f"BF16DEC_ERR gemv epilogue {epi} int 16-bit ({M},{N},{K}) kernel {kernel} bias {int(b)} res {int(r)}: "
                  f"{float((lo == hi).mean()):.4f} of the outputs EXACT by construction, {len(bad)} outside their interval")
            assert not len(bad), (kernel, b, r, len(bad), bad[:4].tolist(), got[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])])
            out = run_gemv(lib, cuda, ops, kernel, epi=epi, f32=True, bias=b, res=r).view(np.float32).astype(np.float64)
            share = np.abs(out - ref32) / np.where(gate32 > 0, gate32, 1.0)          # (gate 0: t = 0 without a residual, err 0 asserted below)
            print(f"BF16DEC_ERR gemv epilogue {epi} int fp32 ({M},{N},{K}) kernel {kernel} bias {int(b)} res {int(r)}: "
                  f"worst err/gate {np.nanmax(share):.3f} [act32_ref]")
            assert np.isfinite(out).all() and (np.abs(out - ref32) <= gate32).all(), (kernel, b, r, float(np.nanmax(share)))


@pytest.mark.parametrize("operands", ["random", "int"])
@pytest.mark.parametrize("epi", [B.EPI_QUICK_GELU, B.EPI_GELU, B.EPI_SILU_MUL], ids=["quick_gelu", "gelu", "silu_mul"])
@pytest.mark.parametrize("M,K", [(8, 1088), (33, 576)])
def test_gemv_transcendental_epilogues(lib, cuda, M, K, epi, operands):
    """Random bf16 operands, and integer operands with the bias of quarters and the residual (r + n) % 8: ring and register kernel
    agree bit for bit, and stay within the bound tests/test_gemm128_gpu.py uses for these epilogues against the computation with
    exact sums: |ref| 2^-7 + 2e-2 (1e-2 for SILU_MUL) — the check tests/test_gemm128_gpu.py makes on random operands.  (The sharp
    checks of these epilogues are test_gemv_gelu_int_operands and test_gemv_silu_mul_int_operands; _gemm128_ref.epilogue rounds an
    activation once, act_quick_gelu_bf16 keeps the bf16 model's three rounding points, which is why quick-GELU measures 0.57 here.)"""
    g0 = np.random.default_rng(M + K + epi)
    silu = epi == B.EPI_SILU_MUL
    N = 96 if silu else 40
    if operands == "int":
        A, W = B.int_operands(M, N, K, 13)
        bias, res = (None, None) if silu else (G.bias_quarters(N), G.residual_mod8(M, N))
    else:
        A = B.bf(g0.standard_normal((M, K)))
        if silu:
            W = G.pack_gate_up(B.bf(g0.standard_normal((48, K)) / np.sqrt(K)), B.bf(g0.standard_normal((48, K)) / np.sqrt(K)))
            bias = res = None
        else:
            W = B.bf(g0.standard_normal((N, K)) / np.sqrt(K))
            bias, res = B.bf(g0.standard_normal(N)), B.bf(g0.standard_normal((M, N)))
    ops = Operands(cuda, A, W, bias, res)
    got = {k: run_gemv(lib, cuda, ops, k, epi=epi, bias=bias is not None, res=res is not None) for k in KERNELS}
    same(got[1], got[3], "dispatch against the register kernel")
    ref = B.epilogue(G.product(A, W), epi, False, bias, res)
    out = as_f32(got[3]).astype(np.float64)
    assert np.isfinite(out).all()
    err, gate = np.abs(out - ref), B.act_bound(ref, epi)
    print(f"BF16DEC_ERR gemv epilogue {epi} {operands} ({M},{N},{K}): abs {err.max():.3e}, worst err/gate {(err / gate).max():.3f}, "
          f"{int((got[3] != want_bits(ref, False)).sum())} of {ref.size} outputs differ in bits [act_bound]")
    assert (err <= gate).all(), float((err / gate).max())


@pytest.mark.parametrize("M,N,K", B.RANDOM_SHAPES)
def test_gemv_random_f32_kernels_identical_and_bounded(lib, cuda, M, N, K):
    """Random data, fp32 output, three runs per kernel (a misplaced counted wait of the ring shows as a rare wrong tile): all outputs
    equal in bits — ring == register kernel — and each within (K + 2) 2^-24 (|A| |W|^T + |bias|) of the float64 product: K fp32
    additions in any order (the gate of the random case of tests/test_gemm128_gpu.py)."""
    g0 = np.random.default_rng(M + N)
    A, W, bias = B.bf(g0.standard_normal((M, K))), B.bf(g0.standard_normal((N, K)) / np.sqrt(K)), B.bf(g0.standard_normal(N))
    ops = Operands(cuda, A, W, bias)
    ref = G.product(A, W) + bias.astype(np.float64)[None, :]
    bound = B.fp32_sum_bound(A, W, bias)
    first = None
    for rep in range(3):
        for kernel in KERNELS:
            got = run_gemv(lib, cuda, ops, kernel, f32=True, bias=True)
            if first is None:
                first = got
            same(got, first, f"kernel {kernel}, run {rep}, against the dispatch's first run")
            if rep == 0:
                out = got.view(np.float32).astype(np.float64)
                assert np.isfinite(out).all()
                share = np.abs(out - ref) / bound
                print(f"BF16DEC_ERR gemv random f32 ({M},{N},{K}) kernel {kernel}: worst err/gate {share.max():.4f} [fp32_sum_bound]")
                assert (share <= 1).all(), (kernel, float(share.max()))
    # 16-bit output of the same accumulators: ring == register kernel
    same(run_gemv(lib, cuda, ops, 1, bias=True), run_gemv(lib, cuda, ops, 3, bias=True), "16-bit output")


@pytest.mark.parametrize("M,N,K,epi", B.TILED_SHAPES)
def test_gemv_tile_major_image_is_row_major(lib, cuda, M, N, K, epi):
    """layout 1 (the door packs the tile-major image with skinny_pack_tiles, the ring kernel streams it) == layout 0 bit for bit, for
    NT = 1 and NT = 2, 16-bit and fp32 output; integer operands, so both are also the exact result."""
    A, W = B.int_operands(M, N, K, 3)
    ops = Operands(cuda, A, W)
    acc = G.product(A, W)
    for kernel in KERNELS:
        for f32 in ((True, False) if epi == B.EPI_NONE else (False,)):
            row = run_gemv(lib, cuda, ops, kernel, epi=epi, f32=f32, layout=0)
            same(run_gemv(lib, cuda, ops, kernel, epi=epi, f32=f32, layout=1), row, (kernel, f32, "layout 1 against layout 0"))
            if epi == B.EPI_SILU_MUL:
                silu_same(row, acc, None, (kernel, "against the reference"))
            else:
                same(row, want_bits(B.epilogue(acc, epi, f32), f32), (kernel, f32, "against the reference"))
    # random operands: the image holds every weight where the ring expects it (integer operands repeat values)
    g0 = np.random.default_rng(N + K)
    Ar, Wr = B.bf(g0.standard_normal((M, K))), B.bf(g0.standard_normal((N, K)) / np.sqrt(K))
    opr = Operands(cuda, Ar, Wr)
    same(run_gemv(lib, cuda, opr, 1, epi=epi, layout=1), run_gemv(lib, cuda, opr, 1, epi=epi, layout=0), "random operands, ring")
    same(run_gemv(lib, cuda, opr, 1, epi=epi, layout=1), run_gemv(lib, cuda, opr, 3, epi=epi, layout=0), "random operands, ring image against registers")


@pytest.mark.parametrize("M,N,K", B.NORM_SHAPES)
def test_gemv_fused_rmsnorm(lib, cuda, M, N, K):
    """The fused RMSNorm is bit-identical to vstar_op_rmsnorm followed by the same door without norm_w (kernels.hpp), on both sides
    of the ring limit (M = 7 | 8 with the norm) and for both kernels, 16-bit and fp32 output; and the fp32 output lies within the
    RMSNorm gate of tests/_f16_prefill_ref.py with u = 2^-8, carried through the product (_bf16_decode_ref.norm_gemv_ref)."""
    eps = 1e-6
    x, gam = B.norm_inputs(M, K, 5)
    g0 = np.random.default_rng(M + N + K)
    W = B.bf(g0.standard_normal((N, K)) / np.sqrt(K))
    ops = Operands(cuda, x, W, norm_w=gam)
    y = sent16(cuda, M + 2, K)
    ok(lib, lib.vstar_op_rmsnorm(None, P(ops.A), P(ops.norm_w), P(y), M, K, eps))
    yb = host16(y)
    assert (yb[M:] == B.SENT16).all()
    ops2 = Operands(cuda, as_f32(yb[:M]), W)
    ref, gate = B.norm_gemv_ref(x, gam, W, eps)
    for kernel in KERNELS:
        for f32 in (True, False):
            fused = run_gemv(lib, cuda, ops, kernel, f32=f32, norm=True, eps=eps)
            same(fused, run_gemv(lib, cuda, ops2, kernel, f32=f32), (kernel, f32, "fused against rmsnorm + GEMV"))
            if f32:
                out = fused.view(np.float32).astype(np.float64)
                share = np.abs(out - ref) / gate
                print(f"BF16DEC_ERR gemv fused rmsnorm ({M},{N},{K}) kernel {kernel}: worst err/gate {share.max():.3f} [RMSNorm gate]")
                assert np.isfinite(out).all() and (share <= 1).all(), float(share.max())


# ================================================================ refusals
def test_rope_kv_append_refusals(lib, cuda):
    """Every rule on the view and the index arrays: VSTAR_ERR_INVALID with a message, qkv and caches bit-unchanged; fmt != 0 is
    refused (the bf16 build has format 0 only); the next valid call succeeds."""
    c = B.random_case(0, R.geometry(0, anc=True))
    d = DevCase(cuda, c)
    live = int(np.nonzero(c.row_pos >= 0)[0][0])
    seq = int(c.row_seq[live])

    def edit(name, i, value):
        a = d.idx[name].copy()
        a[i] = value
        return d.make_rows(**{name: a})

    for rows in bad_rows(d, c, edit, live, seq):
        refused(lib, d.append(lib, rows=rows), "vstar_op_rope_kv_append")
    for v in bad_views(d):
        refused(lib, d.append(lib, view=v), "vstar_op_rope_kv_append")
    refused(lib, d.append(lib, table_rows=int(c.row_pos.max())), "vstar_op_rope_kv_append")
    refused(lib, lib.vstar_op_rope_kv_append(None, P(d.table), c.ctx, ctypes.byref(d.view), ctypes.byref(d.rows)), "vstar_op_rope_kv_append")
    refused(lib, lib.vstar_op_rope_kv_append(P(d.qkv), None, c.ctx, ctypes.byref(d.view), ctypes.byref(d.rows)), "vstar_op_rope_kv_append")
    refused(lib, lib.vstar_op_rope_kv_append(P(d.qkv), P(d.table), c.ctx, None, ctypes.byref(d.rows)), "vstar_op_rope_kv_append")
    refused(lib, lib.vstar_op_rope_kv_append(P(d.qkv), P(d.table), c.ctx, ctypes.byref(d.view), None), "vstar_op_rope_kv_append")
    d.untouched()
    ok(lib, d.append(lib))
    ref = R.append_ref(c)
    assert np.array_equal(d.qkv_bits(), B.bits(ref.qkv))


def bad_rows(d, c, edit, live, seq):
    return [edit("row_pos", live, -2), edit("row_pos", live, c.ctx), edit("row_slot", live, c.slots), edit("row_slot", 0, -1),
            edit("row_seq", live, c.n_seq), edit("row_seq", 0, -1), edit("seq_kv", seq, c.slots), edit("seq_kv", 0, -1),
            edit("seq_prefix", seq, c.slots), edit("seq_prefix", 0, -1), edit("seq_past", seq, -1),
            edit("seq_past", seq, int(c.row_pos[live]) + 1), edit("anc", 5, c.slots), edit("anc", c.slots * c.ctx - 1, -1),
            d.make_rows(row_pos=None), d.make_rows(seq_past=None)]


def bad_views(d):
    """fmt 1 and 2 come with everything the fp16 build asks of them (scale arrays of the right size): refused for the format alone."""
    spare = torch.zeros(d.c.slots * d.c.H * d.c.ctx * 4, dtype=torch.uint8, device=d.k.device)
    d.keep.append(spare)
    return [d.make_view(fmt=1, dev_ks=P(spare), dev_vs=P(spare)), d.make_view(fmt=2), d.make_view(fmt=3), d.make_view(fmt=-1),
            d.make_view(dev_k=None), d.make_view(dev_v=None), d.make_view(slots=0), d.make_view(heads=0), d.make_view(ctx=0)]


def test_cached_attention_refusals(lib, cuda):
    """The index rules, the view rules (fmt != 0 included), the path rules: VSTAR_ERR_INVALID with a message, *path_ran untouched,
    output, qkv and caches bit-unchanged; paths 1 and 2 refuse what they cannot run (never a re-route); then a valid call succeeds."""
    c = B.random_case(0, R.geometry(0, anc=True))
    d = DevCase(cuda, c)
    live = int(np.nonzero(c.row_pos >= 0)[0][0])
    seq = int(c.row_seq[live])

    def edit(name, i, value):
        a = d.idx[name].copy()
        a[i] = value
        return d.make_rows(**{name: a})

    for rows in bad_rows(d, c, edit, live, seq):
        refused(lib, d.attention(lib, rows=rows)[0], ATT)
    for v in bad_views(d):
        refused(lib, d.attention(lib, view=v)[0], ATT)
    top = int(c.row_pos.max())
    refused(lib, d.attention(lib, table_rows=top)[0], ATT)                  # row_pos < table_rows
    refused(lib, d.attention(lib, max_keys=top)[0], ATT)                    # row_pos + 1 <= max_keys
    refused(lib, d.attention(lib, max_keys=c.ctx + 1)[0], ATT)              # max_keys <= ctx
    for path in (3, -1):
        refused(lib, d.attention(lib, path=path)[0], ATT)
    for rep in (0, 17):
        refused(lib, d.attention(lib, repeat=rep)[0], ATT)
    for path in (1, 2):                                                # this geometry has padding rows and several rows per sequence
        rc, ran = d.attention(lib, path=path)
        refused(lib, rc, ATT)
        assert ran == -7
    ran = ctypes.c_int(-7)
    args = (c.ctx, ctypes.byref(d.view), ctypes.byref(d.rows), c.max_keys, 0, 1)
    refused(lib, lib.vstar_op_cached_attention(None, P(d.table), *args, P(d.out), ctypes.byref(ran)), ATT)
    refused(lib, lib.vstar_op_cached_attention(P(d.qkv), P(d.table), *args, None, ctypes.byref(ran)), ATT)
    refused(lib, lib.vstar_op_cached_attention(P(d.qkv), P(d.table), *args, P(d.out), None), ATT)
    refused(lib, lib.vstar_op_cached_attention(P(d.qkv), P(d.table), c.ctx, None, ctypes.byref(d.rows), c.max_keys, 0, 1, P(d.out), ctypes.byref(ran)), ATT)
    refused(lib, lib.vstar_op_cached_attention(P(d.qkv), P(d.table), c.ctx, ctypes.byref(d.view), None, c.max_keys, 0, 1, P(d.out), ctypes.byref(ran)), ATT)
    assert ran.value == -7
    d.untouched()
    # the fused paths on a geometry they can run: a null table, a row_slot that is not the sequence's slot, one key short of the split domain
    c2 = B.random_case(2, R.cases_geometry(2, which=1)[0])
    d2 = DevCase(cuda, c2)
    for path in (1, 2):
        refused(lib, lib.vstar_op_cached_attention(P(d2.qkv), None, c2.ctx, ctypes.byref(d2.view), ctypes.byref(d2.rows), c2.max_keys, path, 1,
                                                   P(d2.out), ctypes.byref(ran)), ATT)
        other = [s for s in range(c2.slots) if s not in c2.seq_kv.tolist()][0]
        slot = c2.row_slot.copy()
        slot[0] = other
        refused(lib, d2.attention(lib, path=path, rows=d2.make_rows(row_slot=np.asarray(slot, np.int32)))[0], ATT)
    refused(lib, d2.attention(lib, path=2, rows=d2.make_rows(row_pos=np.array([100, 7, 254], np.int32)), max_keys=255)[0], ATT)
    d2.untouched()
    rc, ran = d.attention(lib)
    ok(lib, rc)
    assert ran == 0
    ref = R.attention_ref(c)
    gate_check("random path 0", "random path 0 with anc, after the refusals", d.output()[ref.valid], ref.out[ref.valid], ref.loose[ref.valid], "LOOSE")


def test_embed_rows_refusals(lib, cuda):
    """C % 8 != 0, C = 0, R < 1, vocab < 1, null pointers, feature rows without a table: VSTAR_ERR_INVALID, the output keeps its
    sentinel; the next valid call succeeds."""
    src, table, feats = R.embed_case(8, st=B.BF16)
    dt, df = dev16(cuda, table), dev16(cuda, feats)
    out = sent16(cuda, len(src) + 2, 8)
    n = len(src)
    for args in ((HP(src), n, P(dt), len(table), P(df), len(feats), P(out), 12), (HP(src), n, P(dt), len(table), P(df), len(feats), P(out), 0),
                 (HP(src), 0, P(dt), len(table), P(df), len(feats), P(out), 8), (HP(src), n, P(dt), 0, P(df), len(feats), P(out), 8),
                 (HP(src), n, P(dt), len(table), P(df), -1, P(out), 8),
                 (None, n, P(dt), len(table), P(df), len(feats), P(out), 8), (HP(src), n, None, len(table), P(df), len(feats), P(out), 8),
                 (HP(src), n, P(dt), len(table), None, len(feats), P(out), 8), (HP(src), n, P(dt), len(table), P(df), len(feats), None, 8)):
        refused(lib, lib.vstar_op_embed_rows(*args), "vstar_op_embed_rows")
    assert (host16(out) == B.SENT16).all()
    ok(lib, lib.vstar_op_embed_rows(HP(src), n, P(dt), len(table), P(df), len(feats), P(out), 8))
    assert np.array_equal(host16(out)[:n], B.bits(R.embed_rows(src, table, feats)))


def test_argmax_rows_refusals(lib, cuda):
    """ld < cols, cols < 1, rows < 1, null pointers: VSTAR_ERR_INVALID, the host output untouched; the next valid call succeeds."""
    x, ld = R.argmax_case(255, st=B.BF16)
    dx = dev16(cuda, x)
    res = np.full(len(x), -77, np.int32)
    for args in ((P(dx), len(x), 255, 254, HP(res)), (P(dx), len(x), 0, ld, HP(res)), (P(dx), 0, 255, ld, HP(res)),
                 (None, len(x), 255, ld, HP(res)), (P(dx), len(x), 255, ld, None)):
        refused(lib, lib.vstar_op_argmax_rows_lp(*args), "vstar_op_argmax_rows_lp")
    assert (res == -77).all()
    ok(lib, lib.vstar_op_argmax_rows_lp(P(dx), len(x), 255, ld, HP(res)))
    assert np.array_equal(res, R.argmax_rows(x[:, :255]))


def test_gemm_skinny_refusals(lib, cuda):
    """M outside [1, 64], K % 64 != 0, an odd N under SiLU-mul, the tile-major layout without whole tiles, null operands, values
    outside the door's enumerations: VSTAR_ERR_INVALID with a message, *kernel_ran and C untouched; the next valid call succeeds."""
    M, N, K = 8, 64, 512
    A, W = B.int_operands(64, N, K, 1)
    ops = Operands(cuda, A, W)
    C = sent16(cuda, 66, N)
    ran = ctypes.c_int(-7)

    def call(A_=ops.A, W_=ops.W, C_=C, M_=M, N_=N, K_=K, epi=B.EPI_NONE, kernel=1, f32=0, layout=0, ran_=ctypes.byref(ran)):
        return lib.vstar_op_gemm_skinny(P(A_), P(W_), None, None, P(C_), M_, N_, K_, epi, kernel, f32, None, 1e-6, layout, ran_)

    for kw in (dict(M_=0), dict(M_=65), dict(M_=-1), dict(K_=96), dict(K_=0), dict(K_=32), dict(N_=0), dict(N_=63, epi=B.EPI_SILU_MUL),
               dict(N_=40, layout=1), dict(N_=48, epi=B.EPI_SILU_MUL, layout=1), dict(A_=None), dict(W_=None), dict(C_=None), dict(ran_=None),
               dict(kernel=0), dict(kernel=2), dict(kernel=4), dict(f32=2), dict(layout=2), dict(layout=-1), dict(epi=5), dict(epi=-1)):
        refused(lib, call(**kw), "vstar_op_gemm_skinny")
    assert ran.value == -7 and (host16(C) == B.SENT16).all()
    ok(lib, call())
    assert ran.value == (2 if ring_enabled() else 1)
    got = host16(C)
    assert (got[M:] == B.SENT16).all()
    same(got[:M], B.bits(G.product(A[:M], W).astype(np.float32)), "the valid call after the refusals")
