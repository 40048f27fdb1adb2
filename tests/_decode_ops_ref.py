"""References, input builders and gates of the decode-side op tests (tests/test_decode_ops_gpu.py; pinned on the CPU by
tests/test_decode_ops_ref.py).  Plain numpy: h(x) is round-to-nearest-even to fp16, everything else float64 unless said otherwise.

The pieces the bf16 tests reuse (tests/_bf16_decode_ref.py) take a storage type `st` (a Storage, default FP16): how a value is rounded
to the 16-bit format, which numpy dtype carries it, its unit roundoff and its bit patterns.  A Case carries its own.

Layouts (decode.hip): qkv [R, 3 * H * 128] = q | k | v; the RoPE table [rows, 128] = cos[64] | sin[64]; a cache K / V as
[slots][H][ctx][128] LOGICAL values (what a reader decodes), packed for the device by `pack_cache`.
"""
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from oracle.vsm_oracle import rope_tables
from tests._kv8_oracle import kv8_quantize, kv8_round_trip

D = 128
F16, F32, F64 = np.float16, np.float32, np.float64
SQRT_D = np.sqrt(F32(128.0))           # the kernels' sqrtf(128.0f)
INT32_MIN = -2 ** 31


def h(x):
    return np.asarray(x).astype(F16)


def bits(x):
    return np.ascontiguousarray(x).view({1: np.uint8, 2: np.uint16, 4: np.uint32}[np.asarray(x).dtype.itemsize])


@dataclass(frozen=True)
class Storage:
    """A 16-bit storage type: r rounds to nearest even into arrays of `dtype`, bits gives the 16-bit patterns, u is the unit roundoff,
    codes(n, seed[, emin, emax]) a pool of finite, normal, non-zero values with distinct bit patterns."""
    name: str
    dtype: type
    u: float
    torch_dtype: object
    r: Callable
    bits: Callable
    codes: Callable


def rt(x, fmt, st=None):
    """What the cache of format `fmt` holds for the 16-bit rows x [..., 128]."""
    st = st or FP16
    if fmt == 0:
        return st.r(x)
    assert st is FP16, "formats 1 and 2 exist in the fp16 build only"
    return kv8_round_trip(torch.from_numpy(np.ascontiguousarray(h(x)))).numpy().astype(F16)


# ---------------------------------------------------------------- RoPE
def llama_table(rows, theta=1e4, st=None):
    st = st or FP16
    cos, sin = rope_tables(rows, D, theta, st.torch_dtype)
    return st.r(np.concatenate([cos[:, :64].float().numpy(), sin[:, :64].float().numpy()], axis=1))


def identity_table(rows, st=None):
    t = np.zeros((rows, D), (st or FP16).dtype)
    t[:, :64] = 1
    return t


# (cos, sin) pairs with entries in {0, +-0.5, +-1}; three quarters of them are unit rotations
_GRID_PAIRS = np.array([(1, 0), (0, 1), (-1, 0), (0, -1), (1, 0), (0, -1), (.5, .5), (.5, -.5), (-1, 0), (0, 1), (0, -1), (1, 0),
                        (-.5, .5), (-.5, -.5), (0, 1), (-1, 0)], F16)


def grid_table(rows, st=None):
    """A synthetic table whose entries lie in {0, +-0.5, +-1} and vary with the position and the dimension."""
    p, d = np.arange(rows)[:, None], np.arange(64)[None, :]
    pair = _GRID_PAIRS[(p * 7 + d * 3 + (p * d) % 5 + (p // 16) * (1 + d % 3)) % 16]
    return np.concatenate([pair[..., 0], pair[..., 1]], axis=1).astype((st or FP16).dtype)


def rope_rows(x, cs, st=None):
    """x [..., 128] rotated with cs [..., 128] (cos | sin): o1 = h(h(a c) + h(-b s)), o2 = h(h(b c) + h(a s)), products and
    sums in float32 — every step of the kernel, so the result is the kernel's bit for bit (h = st.r, default fp16)."""
    st = st or FP16
    h = st.r
    x, cs = np.asarray(x, st.dtype), np.asarray(cs, st.dtype)
    a, b = x[..., :64].astype(F32), x[..., 64:].astype(F32)
    c, s = cs[..., :64].astype(F32), cs[..., 64:].astype(F32)
    o1 = h(h(a * c).astype(F32) + h(-b * s).astype(F32))
    o2 = h(h(b * c).astype(F32) + h(a * s).astype(F32))
    return np.concatenate([o1, o2], axis=-1)


# ---------------------------------------------------------------- one call of the cache kernels
@dataclass
class Case:
    path: int                       # -1: rope_kv_append, 0 / 1 / 2: cached attention
    fmt: int
    H: int
    ctx: int
    slots: int
    row_seq: np.ndarray
    row_pos: np.ndarray
    row_slot: np.ndarray
    seq_kv: np.ndarray
    seq_prefix: np.ndarray
    seq_past: np.ndarray
    table: np.ndarray               # [ctx, 128] fp16
    qkv: np.ndarray                 # [R, 3 H 128] fp16
    K: np.ndarray                   # [slots, H, ctx, 128] fp16, logical
    V: np.ndarray
    max_keys: int = 0
    anc: Optional[np.ndarray] = None
    targets: Optional[np.ndarray] = None      # probes: [R, H] the key that must win (-1: padding row)
    name: str = ""
    st: Optional[Storage] = None              # the storage type of table, qkv, K and V (None: fp16)

    def __post_init__(self):
        self.st = self.st or FP16

    @property
    def R(self):
        return len(self.row_pos)

    @property
    def n_seq(self):
        return len(self.seq_kv)

    def key_slots(self, r):
        """The slot that holds key j of row r, j = 0 .. pos."""
        seq = self.row_seq[r]
        nk = self.row_pos[r] + 1
        if self.anc is not None:
            return self.anc.reshape(self.slots, self.ctx)[self.seq_kv[seq], :nk].copy()
        return np.where(np.arange(nk) < self.seq_past[seq], self.seq_prefix[seq], self.seq_kv[seq])


def pack_cache(x, fmt, st=None):
    """Logical rows -> the device image: 16-bit cells (formats 0, 2) or (code bytes, E8M0 bytes [..., 4]) (format 1)."""
    if fmt != 1:
        return np.ascontiguousarray(x, (st or FP16).dtype), None
    codes, e, dec = kv8_quantize(np.ascontiguousarray(x, F16).reshape(-1, D))
    assert np.array_equal(bits(dec), bits(x.reshape(-1, D))), "format 1 caches are built from fixed points of the round trip"
    return codes.reshape(x.shape), e.reshape(x.shape[:-1] + (4,))


@dataclass
class AppendRef:
    qkv: np.ndarray                 # the in-place result
    K: np.ndarray                   # logical caches after the call
    V: np.ndarray
    K_raw: np.ndarray               # the rows as they were BEFORE the round trip (format 1: what the codes / scale bytes come from)
    V_raw: np.ndarray
    written: np.ndarray             # [slots, H, ctx] bool


def append_ref(c: Case, rows=None) -> AppendRef:
    """rope_kv_append of the rows (default: all): q, k rotated in place, k and v replaced by what the cache holds, cache rows written."""
    H = c.H
    qkv = c.qkv.copy().reshape(c.R, 3, H, D)
    K, V, Kr, Vr = c.K.copy(), c.V.copy(), c.K.copy(), c.V.copy()
    written = np.zeros((c.slots, H, c.ctx), bool)
    for r in (range(c.R) if rows is None else rows):
        pos = c.row_pos[r]
        if pos < 0:
            continue
        cs = c.table[pos]
        qkv[r, 0] = rope_rows(qkv[r, 0], cs, c.st)
        k, v = rope_rows(qkv[r, 1], cs, c.st), qkv[r, 2].copy()
        qkv[r, 1], qkv[r, 2] = rt(k, c.fmt, c.st), rt(v, c.fmt, c.st)
        s = c.row_slot[r]
        assert not written[s, :, pos].any(), "two rows of a call write the same cache row"
        Kr[s, :, pos], Vr[s, :, pos] = k, v
        K[s, :, pos], V[s, :, pos] = qkv[r, 1], qkv[r, 2]
        written[s, :, pos] = True
    return AppendRef(qkv.reshape(c.R, 3 * H * D), K, V, Kr, Vr, written)


def cache_image_after(before_cells, before_scales, raw, written, fmt, st=None):
    """Device image after a call: `before` everywhere but on the written rows, which hold pack(raw row)."""
    cells = before_cells.copy()
    scales = None if before_scales is None else before_scales.copy()
    idx = np.nonzero(written)
    rows = np.ascontiguousarray(raw[idx], (st or FP16).dtype)        # [n, 128]
    if len(rows) == 0:
        return cells, scales
    if fmt == 0:
        cells[idx] = rows
    elif fmt == 2:
        cells[idx] = rt(rows, 2)
    else:
        codes, e, _ = kv8_quantize(rows)
        cells[idx] = codes
        scales[idx] = e
    return cells, scales


@dataclass
class AttnRef:
    out: np.ndarray                 # [R, H, 128] fp16 (padding rows: zeros, not compared)
    valid: np.ndarray               # [R] bool
    tight: np.ndarray               # [R, H, 128] float64 gates
    loose: np.ndarray
    p: List[List[np.ndarray]]       # [R][H] fp16 probabilities
    exact_dots: bool                # the exact-dot condition holds for every (query, key)
    append: Optional[AppendRef] = None
    f64: Optional[np.ndarray] = None   # plain float64 softmax attention on the same decoded operands


def lsb_exponent(x):
    """Exponent of the lowest set bit of every non-zero float64 (x = odd * 2^e -> e); +inf exponent for zeros."""
    m, e = np.frexp(np.asarray(x, F64))
    i = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = i & -i
    tz = np.where(i != 0, np.log2(np.maximum(low, 1).astype(F64)), 0).astype(np.int64)
    return np.where(i != 0, e - 53 + tz, 10 ** 6)


def dots_exact(qh, Kd):
    """The exact-dot condition for one query: per key, all products are multiples of a power of two u and sum |q k| < 2^24 u —
    every summation order and FMA contraction then gives the same fp32 dot."""
    prod = Kd.astype(F64) * qh.astype(F64)[None, :]                  # exact: fp16 x fp16
    u = np.ldexp(1.0, lsb_exponent(prod).min(axis=1).clip(-900, 900))
    ok = np.abs(prod).sum(axis=1) < 2.0 ** 24 * u
    return bool(np.all(ok | (np.abs(prod).sum(axis=1) == 0)))


def tight_gate(o, pv, vabs, u=2.0 ** -11):
    """TIGHT for a 16-bit format of unit roundoff u (fp16: 2^-11, bf16: 2^-8): 2u |o| (the output's rounding, with slack for the
    reference's own) + 4u sum p|v| (every probability rounded, the normaliser) + 2^-23 sum |v| (fp32 accumulation)."""
    return 2 * u * np.abs(o) + 4 * u * pv + 2.0 ** -23 * vabs


def loose_gate(tight, delta, pv):
    """LOOSE = TIGHT + (e^(2 delta) - 1) sum p|v|: every score off by at most delta moves a probability by e^(+-2 delta)."""
    return tight + np.expm1(2 * delta) * pv


def attn_row(qh, Kd, Vd, st=None):
    """One (row, head) of cached attention on the decoded operands: qh [128], Kd / Vd [nk, 128] in the storage type st (default fp16,
    h = st.r, u = st.u).  a_j = sum q k_j; s_j = h(float32(h(a_j)) / float32(sqrt(128))); p_j = h(exp(s_j - max) / sum);
    o = h(sum p_j v_j).  delta = 4u |s| + 2^-17 sum |q||k| / sqrt(128).
    Returns o, p, the TIGHT and LOOSE gates [128] and the plain float64 attention."""
    st = st or FP16
    h = st.r
    q, Kf, Vf = qh.astype(F64), Kd.astype(F64), Vd.astype(F64)
    a = Kf @ q
    s = h(h(a).astype(F32) / SQRT_D)
    e = np.exp(s.astype(F64) - s.astype(F64).max())
    p = h(e / e.sum())
    o = h((p.astype(F64)[:, None] * Vf).sum(axis=0))
    pv = (p.astype(F64)[:, None] * np.abs(Vf)).sum(axis=0)
    tight = tight_gate(o.astype(F64), pv, np.abs(Vf).sum(axis=0), st.u)
    delta = (4 * st.u * np.abs(s.astype(F64)) + 2.0 ** -17 * (np.abs(Kf) @ np.abs(q)) / float(SQRT_D)).max()
    loose = loose_gate(tight, delta, pv)
    s64 = a / np.sqrt(128.0)
    e64 = np.exp(s64 - s64.max())
    f64 = (e64 / e64.sum()) @ Vf
    return o, p, tight, loose, f64


def attention_ref(c: Case) -> AttnRef:
    H = c.H
    app = None
    K, V = c.K, c.V
    qkv = c.qkv.reshape(c.R, 3, H, D)
    if c.path >= 1:                 # fused: the row is rotated and appended first, then read like any other key
        app = append_ref(c)
        K, V, qkv = app.K, app.V, app.qkv.reshape(c.R, 3, H, D)
    out = np.zeros((c.R, H, D), c.st.dtype)
    tight, loose, f64 = np.zeros((c.R, H, D)), np.zeros((c.R, H, D)), np.zeros((c.R, H, D))
    ps, exact = [], True
    for r in range(c.R):
        ps.append([])
        if c.row_pos[r] < 0:
            continue
        ks = c.key_slots(r)
        j = np.arange(len(ks))
        for hh in range(H):
            Kd, Vd = K[ks, hh, j], V[ks, hh, j]
            o, p, t, lo, f = attn_row(qkv[r, 0, hh], Kd, Vd, c.st)
            out[r, hh], tight[r, hh], loose[r, hh], f64[r, hh] = o, t, lo, f
            ps[r].append(p)
            exact = exact and dots_exact(qkv[r, 0, hh], Kd)
    return AttnRef(out, c.row_pos >= 0, tight, loose, ps, exact, app, f64)


def fused_reads_clear_of_writes(c: Case) -> bool:
    """No row of a fused call reads a cache row that ANOTHER row of the call writes, and (anc) every row finds its own key in its own slot."""
    writes = {(int(c.row_slot[r]), int(c.row_pos[r])): r for r in range(c.R)}
    if len(writes) != c.R:
        return False
    for r in range(c.R):
        ks = c.key_slots(r)
        if ks[c.row_pos[r]] != c.row_slot[r]:
            return False
        for j, s in enumerate(ks):
            if writes.get((int(s), j), r) != r:
                return False
    return True


# ---------------------------------------------------------------- value pools
def f16_codes(n, seed, emin=1, emax=30):
    """n fp16 values, finite, normal, non-zero, biased exponent in [emin, emax]; pairwise distinct bit patterns within every run of
    the pool's size."""
    c = np.arange(65536, dtype=np.int64)
    e = (c >> 10) & 0x1F
    c = c[(e >= emin) & (e <= emax)]
    g = np.random.default_rng(seed)
    out = np.concatenate([g.permutation(c) for _ in range((n + len(c) - 1) // len(c))])[:n]
    return out.astype(np.uint16).view(F16)


FP16 = Storage("fp16", F16, 2.0 ** -11, torch.float16, h, bits, f16_codes)


def cache_values(shape, seed, fmt, st=None):
    """A cache full of distinct codes; formats 1 / 2: of round-trip fixed points none of which is zero (magnitudes in [2^-4, 4): no
    element of a block lies 2^17 below its largest)."""
    n = int(np.prod(shape))
    if fmt == 0:
        return (st or FP16).codes(n, seed).reshape(shape)
    return rt(f16_codes(n, seed, 11, 16).reshape(shape), fmt)


def make_anc(slots, ctx, spare):
    """Ancestry rows that interleave every slot with the slot `spare` position by position (row s: s, spare, s, ...); `spare` is a slot no
    row of the call writes, so a fused call never reads what it writes."""
    anc = np.repeat(np.arange(slots, dtype=np.int32)[:, None], ctx, axis=1)
    anc[:, 1::2] = spare
    return anc


def own_anc(c: Case):
    """The caller's part of the contract: the entries of the rows a call writes point at the writing slot."""
    if c.anc is not None:
        c.anc = c.anc.copy()
        a = c.anc.reshape(c.slots, c.ctx)
        for r in range(c.R):
            if c.row_pos[r] >= 0:
                a[c.row_slot[r], c.row_pos[r]] = c.row_slot[r]
    return c


# ---------------------------------------------------------------- scenarios of the attention tests
def geometry(path, anc=False, big=False):
    """Index arrays of the attention cases.  Slots differ from sequence ids everywhere.
    path 0: 9 rows of 3 sequences (two padding rows); sequence 1 reads its first 5 keys from slot 0 (= sequence 2's own slot).
    path 1: 3 sequences, one row each.  path 2: 3 rows, ctx 576.  Returns a dict of Case fields; positions are set by the caller for
    paths 1 and 2."""
    if path == 0:
        ctx, slots = 48, 4
        row_seq = np.array([0, 0, 1, 2, 1, 0, 1, 2, 2], np.int32)
        row_pos = np.array([3, 4, 9, 11, 10, -1, 12, -1, 12], np.int32)
        seq_kv = np.array([3, 2, 0], np.int32)
        seq_prefix = np.array([3, 0, 0], np.int32)
        seq_past = np.array([0, 5, 0], np.int32)
    else:
        ctx, slots = (576, 4) if (path == 2 or big) else (208, 4)
        row_seq = np.array([2, 0, 1], np.int32)
        row_pos = np.zeros(3, np.int32)
        seq_kv = np.array([3, 1, 0], np.int32)
        seq_prefix = np.array([3, 1, 2], np.int32)
        seq_past = np.zeros(3, np.int32)
    g = dict(ctx=ctx, slots=slots, row_seq=row_seq, row_pos=row_pos, row_slot=seq_kv[row_seq].copy(), seq_kv=seq_kv, seq_prefix=seq_prefix,
             seq_past=seq_past, anc=None)
    if anc:
        g["anc"] = make_anc(slots, ctx, 1 if path == 0 else 2)
        g["seq_past"] = np.zeros_like(seq_past)
        g["seq_prefix"] = seq_kv.copy()
    return g


def with_positions(g, pos, past_of_seq1=0):
    """Paths 1 / 2: the three rows' positions; sequence 1 (row 2) reads keys [0, past) from slot 2, which no row writes."""
    g = dict(g)
    g["row_pos"] = np.array(pos, np.int32)
    if g["anc"] is None:
        sp = g["seq_past"].copy()
        sp[1] = min(past_of_seq1, pos[2])
        g["seq_past"] = sp
    return g


def split_partitions(pos):
    """[lo, hi) of the 8 partitions of the `pos` cached keys of a split-KV row (decode.hip split_range)."""
    span = (((pos + 7) // 8) + 63) & ~63
    out = []
    for p in range(8):
        lo = min(p * span, pos)
        out.append((lo, min(lo + span, pos)))
    return out


def probe_targets(c_path, pos, past):
    """The keys a probe aims at, for one row."""
    if pos < 0:
        return [-1]
    if c_path == 0:
        t = [0, past - 1, past, pos - 1, pos]
    elif c_path == 1:
        t = [0, 15, 16, 63, 64, pos - 1, pos, past - 1, past]
    else:
        t = [pos, past - 1, past]
        for lo, hi in split_partitions(pos):
            if hi > lo:
                t += [lo, hi - 1]
    seen = []
    for j in t:
        if 0 <= j <= pos and j not in seen:
            seen.append(j)
    return seen


def probe_dq(r, hh, t):
    """The one dimension at which a probe's q is non-zero: distinct 8-element lane groups across the rows of a call (r < 16), all 16
    groups over rows, heads and rounds."""
    return 8 * ((r * 5 + hh * 3 + t) % 16) + (r + 2 * hh + t) % 8


def probe_case(path, fmt, g, t, H=2, seed=0, st=None, mag=(16, 16)) -> Case:
    """Round t of the one-hot probes on the geometry g: row r aims at its (t mod n)-th target.  q = mag[0] e_dq; the target key holds
    mag[1] at dq, every other key of the row 0; identity table.  fp16 (16, 16): scores 256 -> h(256 / sqrt(128)) = 22.625 against 0."""
    st = st or FP16
    ctx, slots = g["ctx"], g["slots"]
    R = len(g["row_pos"])
    K = cache_values((slots, H, ctx, D), 100 + seed, fmt, st)
    V = cache_values((slots, H, ctx, D), 200 + seed, fmt, st)
    qkv = (st.codes(R * 3 * H * D, 300 + seed) if fmt == 0 else f16_codes(R * 3 * H * D, 300 + seed, 11, 16)).reshape(R, 3, H, D).copy()
    qkv[:, 0] = 0
    c = own_anc(Case(path, fmt, H, table=identity_table(ctx, st), qkv=qkv.reshape(R, -1), K=K, V=V, st=st, **g))
    c.max_keys = int(max(c.row_pos.max() + 1, 256 if path == 2 else 1))
    qkv = c.qkv.reshape(R, 3, H, D)
    targets = np.full((R, H), -1, np.int64)
    for r in range(R):
        pos = c.row_pos[r]
        if pos < 0:
            continue
        tl = probe_targets(path, pos, c.seq_past[c.row_seq[r]])
        ks = c.key_slots(r)
        j = np.arange(pos + 1)
        for hh in range(H):
            dq = probe_dq(r, hh, t)
            jt = tl[(t + hh) % len(tl)]
            targets[r, hh] = jt
            qkv[r, 0, hh, dq] = mag[0]
            K[ks, hh, j, dq] = 0
            if path >= 1:
                qkv[r, 1, hh, dq] = mag[1] if jt == pos else 0
            if not (path >= 1 and jt == pos):
                K[ks[jt], hh, jt, dq] = mag[1]
    c.K = rt(K, fmt, st)                                # (formats 1 / 2: the edited blocks, made fixed points again)
    c.targets = targets
    c.name = f"probe path {path} fmt {fmt} round {t}"
    return c


def probe_rounds(path, g):
    return max(len(probe_targets(path, int(p), int(g["seq_past"][s]))) for p, s in zip(g["row_pos"], g["row_seq"]))


def _grid(g, shape, lo=1, st=None):
    """Random non-zero multiples of 1/8 in [-1, 1] with |x| >= lo / 8."""
    return (g.integers(lo, 9, shape) * g.choice([-1, 1], shape) / 8.0).astype((st or FP16).dtype)


def exact_dot_case(path, fmt, g, H=2, seed=0, st=None) -> Case:
    """Exact-dot inputs: q, k multiples of 1/8 in [-1, 1], table entries in {0, +-0.5, +-1}, so the rotated rows lie on a grid of
    1/16 and every dot product is exact in fp32 in any order.  Lumpy probabilities: the keys at the edges of every mechanism (0,
    past - 1, past, the partition edges, pos - 1 and the rows' own keys) are aligned with the sign of the (rotated) query, everything
    else is random."""
    st = st or FP16
    h = st.r
    rng = np.random.default_rng(seed)
    ctx, slots = g["ctx"], g["slots"]
    R = len(g["row_pos"])
    table = grid_table(ctx, st)
    K = _grid(rng, (slots, H, ctx, D), st=st)
    V = rt(h(0.5 * rng.standard_normal((slots, H, ctx, D))), fmt, st)
    qkv = np.zeros((R, 3, H, D), st.dtype)
    qkv[:, 2] = h(0.5 * rng.standard_normal((R, H, D)))
    c = own_anc(Case(path, fmt, H, table=table, qkv=qkv.reshape(R, -1), K=K, V=V, st=st, **g))
    c.max_keys = int(max(c.row_pos.max() + 1, 256 if path == 2 else 1))
    qkv = c.qkv.reshape(R, 3, H, D)
    for s in range(c.n_seq):
        rows = [r for r in range(R) if c.row_seq[r] == s and c.row_pos[r] >= 0]
        sign = rng.choice([-1.0, 1.0], (H, D))          # of the sequence's ROTATED queries
        for r in rows:
            pos = c.row_pos[r]
            mag = rng.integers(5, 9, (H, D)) / 8.0
            if path == 0:                                # q is given rotated; the own key lies in the cache
                qkv[r, 0] = h(sign * mag)
            else:                                        # raw q and k share signs: rotations keep their dot product, (c^2 + s^2) sum |q||k|
                raw_sign = rng.choice([-1.0, 1.0], (H, D))
                qkv[r, 0] = h(raw_sign * mag)
                qkv[r, 1] = h(raw_sign * rng.integers(6, 9, (H, D)) / 8.0)
        for r in rows:
            pos, past = c.row_pos[r], c.seq_past[s]
            ks = c.key_slots(r)
            hot = [j for j in probe_targets(path, pos, past) if not (path >= 1 and j == pos)]
            if path == 0:
                hot += [int(c.row_pos[r2]) for r2 in rows if c.row_pos[r2] <= pos]
            qh = sign if path == 0 else np.sign(rope_rows(qkv[r, 0], table[pos], st).astype(F64))
            for j in set(hot):
                al = np.where(qh != 0, qh, 1.0) * rng.integers(6, 9, (H, D)) / 8.0
                K[ks[j], :, j] = h(al)
    c.K = rt(K, fmt, st)
    c.name = f"exact-dot path {path} fmt {fmt}"
    return c


def random_case(path, fmt, g, H=2, seed=0, st=None) -> Case:
    """The real LLaMA table; qkv and the caches 0.5 x normal."""
    st = st or FP16
    h = st.r
    rng = np.random.default_rng(1000 + seed)
    ctx, slots = g["ctx"], g["slots"]
    R = len(g["row_pos"])
    K = rt(h(0.5 * rng.standard_normal((slots, H, ctx, D))), fmt, st)
    V = rt(h(0.5 * rng.standard_normal((slots, H, ctx, D))), fmt, st)
    qkv = h(0.5 * rng.standard_normal((R, 3 * H * D)))
    c = own_anc(Case(path, fmt, H, table=llama_table(ctx, st=st), qkv=qkv, K=K, V=V, st=st, **g))
    c.max_keys = int(max(c.row_pos.max() + 1, 256 if path == 2 else 1))
    c.name = f"random path {path} fmt {fmt}"
    return c


def lumpy(ref: AttnRef) -> bool:
    """In every row at least three keys have p > 0.05 and the largest p is below 0.6."""
    return all((p.astype(F64) > 0.05).sum() >= 3 and p.astype(F64).max() < 0.6 for row in ref.p for p in row)


def one_hot(c: Case, ref: AttnRef) -> bool:
    """Every probability vector is exactly one-hot at the target."""
    for r in range(c.R):
        for hh, p in enumerate(ref.p[r]):
            want = np.zeros(len(p), c.st.dtype)
            want[c.targets[r, hh]] = 1
            if not np.array_equal(c.st.bits(p), c.st.bits(want)):
                return False
    return True


# the positions of the fused cases (tests/test_decode_ops_gpu.py and the CPU conditions use the same lists)
PATH1_POS = [(0, 1, 63), (64, 65, 200)]
PATH2_POS = [(255, 63, 0), (513, 256, 300), (511, 512, 513)]
PATH1_EXACT_POS, PATH2_EXACT_POS = (64, 65, 200), (513, 256, 300)
PATH1_PAST, PATH2_PAST = 40, 200


def cases_geometry(path, which=None, anc=False, big=False):
    """The geometries the tests run: path 0 one; paths 1 / 2 one per position triple (`which` picks one)."""
    if path == 0:
        return [geometry(0, anc)]
    pos = PATH1_POS if path == 1 else PATH2_POS
    past = PATH1_PAST if path == 1 else PATH2_PAST
    out = [with_positions(geometry(path, anc, big), p, past) for p in pos]
    return out if which is None else [out[which]]


# ---------------------------------------------------------------- Perceiver attention
PERCEIVER_SHAPES = [(1, 1, 3, 1), (2, 2, 5, 64), (1, 2, 7, 65), (1, 1, 4, 288), (1, 1, 2, 512)]     # (n, H, L, NK)
PERCEIVER_DH = [32, 64, 96]


def perceiver_qhat(q, DH, kernel_way=False):
    """h(q / sqrt(DH)); kernel_way: h(float32(q) * (1.0f / sqrtf(DH))) — the builders' condition is that both agree."""
    if kernel_way:
        return h(q.astype(F32) * (F32(1.0) / np.sqrt(F32(DH))))
    return h(q.astype(F64) / np.sqrt(float(DH)))


@dataclass
class PcvRef:
    out: np.ndarray                 # [n * L, H * DH] fp16
    tight: np.ndarray
    loose: np.ndarray
    p: np.ndarray                   # [n, H, L, NK] fp16
    exact_dots: bool
    f64: np.ndarray


def perceiver_ref(q, kv, n, L, NK, H, DH) -> PcvRef:
    """q [n L, H DH], kv [n NK, 2 H DH] = k | v.  qh = h(q / sqrt(DH)); sim = h(sum qh k); x = h(sim - max); p = h(exp(x) / sum);
    o = h(sum p v).  TIGHT as for cached attention.  LOOSE adds (e^(2 delta) - 1) sum p |v| with
    delta = max_j 2^-10 (|sim_j| + |max| + |x_j|) + 2^-16 sum_e |qh_e k_je|: one fp16 step of sim_j, of the maximum and of x_j, and twice
    the bound DH * 2^-24 <= 2^-17 of an fp32 accumulation (the key's and the maximum's)."""
    C = H * DH
    qh = perceiver_qhat(q, DH).astype(F64).reshape(n, L, H, DH)
    k = kv[:, :C].astype(F64).reshape(n, NK, H, DH)
    v = kv[:, C:].astype(F64).reshape(n, NK, H, DH)
    out, tight, loose, f64 = np.zeros((n, L, H, DH), F16), np.zeros((n, L, H, DH)), np.zeros((n, L, H, DH)), np.zeros((n, L, H, DH))
    ps = np.zeros((n, H, L, NK), F16)
    exact = True
    for b in range(n):
        for hh in range(H):
            for i in range(L):
                qv, kk, vv = qh[b, i, hh], k[b, :, hh], v[b, :, hh]
                a = kk @ qv
                sim = h(a).astype(F64)
                x = h(sim - sim.max()).astype(F64)
                e = np.exp(x)
                p = h(e / e.sum())
                o = h((p.astype(F64)[:, None] * vv).sum(axis=0))
                pv = (p.astype(F64)[:, None] * np.abs(vv)).sum(axis=0)
                t = 2.0 ** -10 * np.abs(o.astype(F64)) + 2.0 ** -9 * pv + 2.0 ** -23 * np.abs(vv).sum(axis=0)
                delta = (2.0 ** -10 * (np.abs(sim) + np.abs(sim).max() + np.abs(x)) + 2.0 ** -16 * (np.abs(kk) @ np.abs(qv))).max()
                out[b, i, hh], tight[b, i, hh], loose[b, i, hh], ps[b, hh, i] = o, t, t + np.expm1(2 * delta) * pv, p
                s64 = kk @ (q.astype(F64).reshape(n, L, H, DH)[b, i, hh] / np.sqrt(float(DH)))
                e64 = np.exp(s64 - s64.max())
                f64[b, i, hh] = (e64 / e64.sum()) @ vv
                exact = exact and dots_exact(h(qv), h(kk))
    sh = (n * L, C)
    return PcvRef(out.reshape(sh), tight.reshape(sh), loose.reshape(sh), ps, exact, f64.reshape(sh))


def perceiver_probe(n, H, L, NK, DH, seed):
    """One-hot probes: q = 64 e_dq, the target key 16 at dq, every other key 0 there: sim = h(h(64 / sqrt(DH)) * 16) >= 104 against 0.
    Targets walk over key 0, the last key and the keys next to the 64-key lane passes.  Returns q, kv, targets [n, H, L]."""
    C = H * DH
    q = np.zeros((n, L, H, DH), F16)
    kv = f16_codes(n * NK * 2 * C, seed).reshape(n, NK, 2, H, DH).copy()
    edge = [j for j in (0, NK - 1, 63, 64, NK // 2, 255, 256, NK - 2) if 0 <= j < NK]
    tg = np.zeros((n, H, L), np.int64)
    for b in range(n):
        for hh in range(H):
            for i in range(L):
                dq = (7 * i + 3 * hh + 11 * b + seed) % DH
                jt = edge[(i + hh + b) % len(edge)]
                q[b, i, hh, dq] = 64
                tg[b, hh, i] = jt
    for b in range(n):          # the keys: zero at every dq some query of this (image, head) uses, 16 at its target
        for hh in range(H):
            for i in range(L):
                dq = (7 * i + 3 * hh + 11 * b + seed) % DH
                kv[b, :, 0, hh, dq] = 0
            used = {}
            for i in range(L):
                dq = (7 * i + 3 * hh + 11 * b + seed) % DH
                assert used.setdefault(dq, i) == i, "two queries of a head share their probe dimension"
                kv[b, tg[b, hh, i], 0, hh, dq] = 16
    return q.reshape(n * L, C), kv.reshape(n * NK, 2 * C), tg


def perceiver_exact(n, H, L, NK, DH, seed):
    """Exact-dot inputs: qh = h(q / sqrt(DH)) with |qh| in [2^-5, 2^-1) (or 0), k multiples of 1/4 in [-1, 1]: products are multiples
    of 2^-17 and sum |qh k| < 48 < 2^24 2^-17.  Lumpy: up to four keys are aligned with the sign of the query."""
    rng = np.random.default_rng(seed)
    C = H * DH
    lim = np.sqrt(float(DH))
    sign = rng.choice([-1.0, 1.0], (n, 1, H, DH))
    q = h(sign * rng.uniform(0.26, 0.48, (n, L, H, DH)) * lim)
    k = (rng.integers(-4, 5, (n, NK, H, DH)) / 4.0).astype(F16)
    hot = sorted({0, NK - 1, NK // 2, NK // 3, min(64, NK - 1), min(63, NK - 1)})
    for j in hot:
        k[:, j] = h(sign[:, 0] * rng.integers(3, 5, (n, H, DH)) / 4.0)
    v = h(0.5 * rng.standard_normal((n, NK, H, DH)))
    return q.reshape(n * L, C), np.concatenate([k.reshape(n * NK, C), v.reshape(n * NK, C)], axis=1)


def perceiver_random(n, H, L, NK, DH, seed):
    rng = np.random.default_rng(seed)
    C = H * DH
    return h(rng.standard_normal((n * L, C))), h(rng.standard_normal((n * NK, 2 * C)))


# ---------------------------------------------------------------- embed_rows / argmax_rows_lp (contracts: kernels.hpp)
def embed_rows(src, table, feats):
    """x[r] = table[src] for 0 <= src < vocab, feats[-(src + 1)] for a feature index in range, zero for INT32_MIN and out-of-range."""
    out = np.zeros((len(src), table.shape[1]), table.dtype)          # (the storage type's carrier: float16, or float32 for bf16)
    for r, s in enumerate(np.asarray(src, np.int64)):
        if 0 <= s < len(table):
            out[r] = table[s]
        elif s < 0 and s != INT32_MIN and -(s + 1) < len(feats):
            out[r] = feats[-(s + 1)]
    return out


def argmax_rows(x):
    """The first column holding the largest NUMBER; NaN never wins; a row of only NaN and / or -inf returns 0."""
    out = np.zeros(len(x), np.int32)
    for r, row in enumerate(np.asarray(x, F64)):
        best, idx = -3.0e38, 0
        for c, v in enumerate(row):
            if v > best:
                best, idx = v, c
        out[r] = idx
    return out


# ---------------------------------------------------------------- builders of the remaining cases
def append_case(H, fmt, seed=0, st=None, table=None) -> Case:
    """rope_kv_append: 37 rows over 3 sequences, 5 of them padding, positions in no order, slots (2, 0, 3) for sequences (0, 1, 2);
    the real LLaMA table, random qkv; the caches full of distinct codes (the sentinel of every row the call does not write)."""
    rng = np.random.default_rng(50 + seed)
    ctx, slots, R = 40, 4, 37
    seq_kv = np.array([2, 0, 3], np.int32)
    row_seq = rng.integers(0, 3, R).astype(np.int32)
    row_pos = np.zeros(R, np.int32)
    for s in range(3):
        idx = np.nonzero(row_seq == s)[0]
        row_pos[idx] = rng.permutation(ctx)[: len(idx)]
    row_pos[[4, 11, 12, 30, 36]] = -1
    st = st or FP16
    qkv = st.r(rng.standard_normal((R, 3 * H * D)))
    return Case(-1, fmt, H, ctx, slots, row_seq, row_pos, seq_kv[row_seq].copy(), seq_kv, seq_kv.copy(), np.zeros(3, np.int32),
                llama_table(ctx, st=st) if table is None else table(ctx, st), qkv, cache_values((slots, H, ctx, D), 7, fmt, st),
                cache_values((slots, H, ctx, D), 8, fmt, st), name=f"append H {H} fmt {fmt}", st=st)


def embed_case(C, seed=0, st=None):
    """Distinct codes; sources: token ids, feature rows, INT32_MIN, an id >= vocab, a feature index >= n_feat_rows."""
    vocab, nf = 37, 9
    pool = (st or FP16).codes((vocab + nf) * C, 60 + seed)
    table, feats = pool[: vocab * C].reshape(vocab, C), pool[vocab * C:].reshape(nf, C)
    src = np.array([0, vocab - 1, -1, -nf, INT32_MIN, vocab, vocab + 1000, -(nf + 1), -(nf + 500), 5, -3, 2 ** 31 - 1, INT32_MIN + 1, 17, 5],
                   np.int32)
    return src, table, feats


ARGMAX_COLS = [1, 255, 257, 1000]


def argmax_case(cols, seed=0, st=None):
    """Rows [9, ld] with ld = cols + 9: random values; the padding columns hold the largest value of all; rows with ties (the
    first wins), NaN (never wins), only NaN, only -inf, NaN and -inf."""
    rng = np.random.default_rng(70 + seed)
    ld = cols + 9
    st = st or FP16
    x = st.r(rng.standard_normal((9, ld)))
    x[:, cols:] = 1000.0
    x[1, rng.integers(0, cols, 3)] = 7.0                            # a tie of up to three columns
    x[2, :] = 3.0                                                    # every column ties: 0
    x[2, cols:] = 1000.0
    x[3, rng.integers(0, cols, max(1, cols // 3))] = np.nan
    x[4, :cols] = np.nan
    x[5, :cols] = -np.inf
    x[6, :cols] = np.where(np.arange(cols) % 2 == 0, np.nan, -np.inf)
    x[7, :cols] = -np.inf
    x[7, cols - 1] = -60000.0                                        # one number among -inf, in the last column
    x[8, 0] = np.nan
    x[8, cols - 1] = 9.0
    if cols > 1:
        x[8, cols - 2] = 9.0                                         # a tie in the last two columns
    return st.r(x), ld
