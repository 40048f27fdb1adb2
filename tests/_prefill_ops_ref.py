"""References, input builders and geometries of the prefill-side op tests (tests/test_prefill_ops_gpu.py; pinned on the CPU by
tests/test_prefill_ops_ref.py): GEMM row maps, the RoPE fused into the GEMM epilogue, the LayerNorm sums, grouped attention.

Plain numpy / torch.  bf16 values travel as float32 arrays whose low 16 bits are zero (`bf` rounds to nearest even, `bits` gives the
16-bit patterns); references are float64 or exact integer / bit arithmetic.  Layouts: a GEMM computes C [M, N] = A [M, K] . W [N, K]^T;
the fused-RoPE table is [rows, 128] = cos(64) | sin(64); qkv is [B * S, 3 * H * D] = q | k | v.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from tests._decode_ops_ref import loose_gate, tight_gate

F32, F64 = np.float32, np.float64
U_BF16 = 2.0 ** -9                     # unit roundoff of bf16 (8 significant bits)
SENT16 = 0x7FC5                        # a quiet bf16 NaN no kernel produces
SENT32 = 0x7FC00123                    # its fp32 twin, for the statistics buffers


# ---------------------------------------------------------------- bf16
def bf(x):
    """Round to nearest even to bf16; returned as float32."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, F32))).bfloat16().float().numpy()


def bits(x):
    """The 16-bit patterns of bf16 values held as float32."""
    x = np.ascontiguousarray(np.asarray(x, F32))
    u = x.view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def is_bf16(x):
    """Whether every value survives the trip float64 -> float32 -> bf16 unchanged."""
    x32 = np.ascontiguousarray(np.asarray(x, F32))
    return bool(np.array_equal(np.atleast_1d(np.asarray(x, F64)), np.atleast_1d(x32).astype(F64)) and not (x32.view(np.uint32) & 0xFFFF).any())


def to_t(x):
    """float32-held bf16 values -> a torch.bfloat16 tensor (exact)."""
    assert is_bf16(x)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, F32))).bfloat16()


def from_t(t):
    return t.float().cpu().numpy()


# ---------------------------------------------------------------- row maps (kernels.hpp: GemmParams)
@dataclass(frozen=True)
class RowMap:
    group: int = 0
    gstride: int = 0
    off: int = 0


IDENT = RowMap()


def map_row(r, group, gstride, off):
    """mapped(r) = (r / group) * gstride + off + r % group; group <= 0: identity."""
    r = np.asarray(r, np.int64)
    if group <= 0:
        return r
    return (r // group) * gstride + off + r % group


def touched_rows(M, m: RowMap):
    """The mapped rows of a call over rows [0, M), in call order."""
    return map_row(np.arange(M), m.group, m.gstride, m.off)


def extent(M, m: RowMap):
    """Rows a buffer addressed through `m` must hold."""
    return int(touched_rows(M, m).max()) + 1


# ---------------------------------------------------------------- RoPE positions and rotation
@dataclass(frozen=True)
class RopeMode:
    """plain: position = row % S.  grouped (R0 > 0): q = row % S; q >= R0 -> Lc + ((q - R0) & 31).  shared prefix (tail > 0):
    row >= tail -> row - tail, else row % S + pos0 (rows [0, tail) are sequences of S rows that start at position pos0)."""
    S: int
    R0: int = 0
    Lc: int = 0
    pos0: int = 0
    tail: int = 0

    @property
    def name(self):
        return "grouped" if self.R0 else "prefix" if self.tail else "plain"


def rope_pos(row, mode: RopeMode):
    row = np.asarray(row, np.int64)
    pos = row % mode.S
    if mode.R0 > 0:
        pos = np.where(pos >= mode.R0, mode.Lc + ((pos - mode.R0) % 32), pos)
    if mode.tail > 0:
        pos = np.where(row >= mode.tail, row - mode.tail, pos + mode.pos0)
    return pos


def rope_apply(x, partner, cos, sin):
    """bf(bf(x * cos) + bf(partner * sin)), float32 arithmetic on bf16 inputs: both products are exact in fp32 (8 x 8 significant
    bits) and the sum is one correctly rounded add, so every step is deterministic and the result is the kernels' bit for bit.
    `partner` carries the sign: -second half for the first half of a head, +first half for the second."""
    x, partner, cos, sin = (np.asarray(a, F32) for a in (x, partner, cos, sin))
    return bf(bf(x * cos) + bf(partner * sin))


def rope_heads(x, cs):
    """x [..., D] (one head) rotated with cs [..., D] = cos(D / 2) | sin(D / 2) (rotate-half)."""
    hd = x.shape[-1] // 2
    a, b, c, s = x[..., :hd], x[..., hd:], cs[..., :hd], cs[..., hd:]
    return np.concatenate([rope_apply(a, -b, c, s), rope_apply(b, a, c, s)], axis=-1)


def rope_qk(C, table, pos, n_heads, D=128):
    """C [M, >= n_heads * D]: the first n_heads heads of every row rotated at position pos[row]; the other columns unchanged."""
    out = np.array(C, F32, copy=True)
    cs = table[pos]
    for h in range(n_heads):
        out[:, h * D:(h + 1) * D] = rope_heads(out[:, h * D:(h + 1) * D], cs)
    return out


def probe_table(rows):
    """cos[pos, i] = pos % 256, sin[pos, i] = 64 * (pos // 256) + i: small integers naming the position and the column."""
    assert rows <= 1024, "64 * (pos // 256) + i must stay below 256 to be a bf16 integer"
    p, i = np.arange(rows)[:, None], np.arange(64)[None, :]
    t = np.concatenate([np.broadcast_to(p % 256, (rows, 64)), 64 * (p // 256) + i], axis=1).astype(F32)
    return t


def llama_table(rows, D=128, theta=1e4):
    i = np.arange(D // 2, dtype=F64)
    ang = np.arange(rows, dtype=F64)[:, None] / theta ** (2 * i / D)[None, :]
    return bf(np.concatenate([np.cos(ang), np.sin(ang)], axis=1))


# fused RoPE: N = 768 = q | k | v of H = 2 heads of 128, the q | k columns rotated
ROPE_N, ROPE_COLS, ROPE_HEADS = 768, 512, 4


def rope_probe_operands(M, K):
    """A [M, K] and W [768, K] whose product is exactly 1 in the first half of every head of 128 columns and 0 in the second."""
    A = np.zeros((M, K), F32)
    A[:, 0] = 1
    W = np.zeros((ROPE_N, K), F32)
    W[(np.arange(ROPE_N) % 128) < 64, 0] = 1
    return A, W


def rope_probe_expected(M, mode: RopeMode, table):
    """What the fused call must store: the table row of each position in every q | k head, the raw 1 | 0 pattern in the v heads."""
    pre = np.tile(np.concatenate([np.ones(64, F32), np.zeros(64, F32)]), ROPE_N // 128)
    out = np.broadcast_to(pre, (M, ROPE_N)).copy()
    cs = table[rope_pos(np.arange(M), mode)]
    for h in range(ROPE_HEADS):
        out[:, h * 128:(h + 1) * 128] = cs
    return out


# the modes of the probe per M; every position stays below 1024 (probe_table)
def rope_modes(M):
    plain = {1024: RopeMode(512), 1030: RopeMode(515)}[M]
    nseq, Sr, Lp = {1024: (9, 111, 25), 1030: (5, 201, 25)}[M]
    return [plain, RopeMode(288, R0=128, Lc=100), RopeMode(544, R0=256, Lc=129), RopeMode(Sr, pos0=Lp, tail=nseq * Sr)]


def prefix_map(mode: RopeMode):
    """The row map that goes with a shared-prefix mode: the compact rows are rows [Lp, S) of every sequence of S = Sr + Lp buffer
    rows, and the partial last group — the Lp prefix rows — lands on rows [Lp, 2 Lp) of the slot behind the last sequence."""
    assert mode.tail > 0
    return RowMap(mode.S, mode.S + mode.pos0, mode.pos0)


# ---------------------------------------------------------------- row-map probes
@dataclass
class MapProbe:
    A: np.ndarray                       # [a_rows, K] buffer
    W: np.ndarray                       # [N, K]
    C: np.ndarray                       # [c_rows, N] expected, sentinel rows excluded (see c_written)
    c_written: np.ndarray               # [c_rows] bool
    row_scale: Optional[np.ndarray] = None      # [a_rows]
    res: Optional[np.ndarray] = None            # [c_rows, N]
    sumsq: Optional[np.ndarray] = None          # [c_rows, N / 64] float64, exact


def map_probe(M, N, K, am: RowMap, cm: RowMap, scaled=False, col=None) -> MapProbe:
    """Compact row r of A is one-hot at column col[r] (default r % K), so C[crow(r), n] = W[n, col[r]]; W is asymmetric.  Buffer rows
    no compact row maps to hold 3.0 everywhere (A) / a scale of 3 / a residual of 100: reading one of them changes every output of the row.
    scaled: row_scale[arow(r)] = 2^(r % 5 - 2) and res[crow(r), n] = (r + n) % 8, W entries below 13 so that every stored value is
    a multiple of 1/4 below 64 and the sums of squares of 64 of them are exact in fp32 in any order."""
    ar, cr = touched_rows(M, am), touched_rows(M, cm)
    a_rows, c_rows = int(ar.max()) + 1, int(cr.max()) + 1
    A = np.full((a_rows, K), 3.0, F32)
    col = np.arange(M) % K if col is None else np.asarray(col, np.int64)
    assert col.shape == (M,) and (0 <= col).all() and (col < K).all()
    A[ar] = 0
    A[ar, col] = 1
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    W = ((n * K + k) % (13 if scaled else 251)).astype(F32)
    acc = W[:, col].T                                                # [M, N], exact
    written = np.zeros(c_rows, bool)
    written[cr] = True
    C = np.zeros((c_rows, N), F32)
    p = MapProbe(A, W, C, written)
    if scaled:
        p.row_scale = np.full(a_rows, 3.0, F32)
        p.row_scale[ar] = 2.0 ** (np.arange(M) % 5 - 2)
        p.res = np.full((c_rows, N), 100.0, F32)
        p.res[cr] = ((np.arange(M)[:, None] + np.arange(N)[None, :]) % 8).astype(F32)
        C[cr] = bf(bf(acc * p.row_scale[ar][:, None]) + p.res[cr])
        if N % 64 == 0:
            p.sumsq = (C.astype(F64) ** 2).reshape(c_rows, N // 64, 64).sum(axis=2)
    else:
        C[cr] = acc
    return p


# (M, N, K), A map, C map, the kernel gemm_last_tile() must name
MAP_CASES = {
    "g128": ((70, 130, 64), RowMap(7, 12, 3), RowMap(7, 9, 2), 128),
    "g128_stats": ((70, 192, 64), RowMap(7, 12, 3), RowMap(7, 9, 2), 128),
    "g256": ((1030, 256, 128), RowMap(103, 128, 25), RowMap(103, 128, 25), 256),
    # the shared-prefix pattern proper: M = nseq * Sr + Lp, whose partial last group (25 rows) lands on rows [Lp, 2 Lp) behind the sequences
    "g256_partial": ((10 * 103 + 25, 256, 128), RowMap(103, 128, 25), RowMap(103, 128, 25), 256),
}


# ---------------------------------------------------------------- 64-column statistics
def span_sums(C):
    """Per row and 64 columns: (sum, sum of squares) of the stored bf16 values, float64."""
    C = np.asarray(C, F64)
    s = C.reshape(C.shape[0], -1, 64)
    return s.sum(axis=2), (s * s).sum(axis=2)


def span_abs(C):
    C = np.abs(np.asarray(C, F64)).reshape(C.shape[0], -1, 64)
    return C.sum(axis=2)


def int_operands(M, N, K, seed):
    """A, W with entries in {-1, 0, 1}: C is an integer of magnitude <= K <= 256 (a bf16 value), its span sums (<= 2^14) and
    sums of squares (<= 2^22) are exact in fp32 in any order."""
    g = np.random.default_rng(seed)
    A = g.integers(-1, 2, (M, K)).astype(F32)
    W = g.integers(-1, 2, (N, K)).astype(F32)
    return A, W


STATS_CASES = {"g128": ((70, 192, 64), 128), "g256": ((1030, 256, 128), 256), "g4w": ((1024, 256, 128), 2564)}
STATS_CMAP = {"g128": RowMap(7, 9, 2), "g256": RowMap(103, 128, 25)}


# ---------------------------------------------------------------- grouped attention
# (B, S, H, R0, Lc)
GROUPED = [(2, 288, 3, 128, 100), (1, 160, 2, 128, 128), (1, 544, 5, 256, 129), (1, 160, 2, 128, 1)]
GROUPED_MX = (1, 256, 2, 128, 100)


def causal_mask(S):
    return np.tril(np.ones((S, S), bool))


def grouped_mask(S, R0, Lc):
    """[S, S] (query, key).  kernels.hpp: rows [0, Lc) of a sequence are a shared prefix, rows [R0, S) independent 32-row suffix
    blocks that attend to the prefix and causally to themselves.  So a row < R0 is plain causal; a row i >= R0 sees the keys < Lc
    and the keys [R0 + 32 ((i - R0) // 32), i]."""
    i, j = np.arange(S)[:, None], np.arange(S)[None, :]
    m = j <= i
    if R0 > 0:
        start = R0 + 32 * ((i - R0) // 32)
        m = np.where(i >= R0, (j < Lc) | ((j >= start) & (j <= i)), m)
    return m


def block_rows(S, R0, b):
    return np.arange(R0 + 32 * b, R0 + 32 * b + 32)


def n_blocks(S, R0):
    return (S - R0) // 32


def in_domain(S, R0, Lc):
    return R0 % 128 == 0 and 0 < Lc <= R0 <= S and (S - R0) % 32 == 0


@dataclass
class AttnRef:
    out: np.ndarray                     # [B, S, H, 128] float64
    tight: np.ndarray
    loose: np.ndarray


def masked_attention(qkv, B, S, H, mask, D=128) -> AttnRef:
    """Float64 softmax(q k^T / sqrt(D)) v under `mask`, with the gates of a bf16 kernel that rounds q * scale * log2(e) to bf16
    once, keeps scores, row maximum and row sum in fp32, rounds the probabilities to bf16 for the PV product and stores bf16:
      TIGHT = tight_gate(o, sum p|v|, sum |v|, u = 2^-9)   (output and probability roundings, fp32 accumulation);
      LOOSE = TIGHT + (e^(2 delta) - 1) sum p|v|, delta = max over the visible keys of (2^-9 + 2^-17) sum_d |q_d k_d| / sqrt(D):
              each element of the pre-scaled q is off by at most 2^-9 relative, and fp32 accumulation of D products adds 2^-17."""
    x = np.asarray(qkv, F64).reshape(B, S, 3, H, D)
    out, tight, loose = (np.zeros((B, S, H, D)) for _ in range(3))
    sc = 1.0 / np.sqrt(float(D))
    for b in range(B):
        for h in range(H):
            q, k, v = x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h]
            s = np.where(mask, (q @ k.T) * sc, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            p /= p.sum(axis=1, keepdims=True)
            o = p @ v
            pv = p @ np.abs(v)
            vabs = np.where(mask, 1.0, 0.0) @ np.abs(v)
            delta = (np.where(mask, (np.abs(q) @ np.abs(k).T) * sc, 0.0)).max(axis=1) * (U_BF16 + 2.0 ** -17)
            t = tight_gate(o, pv, vabs, U_BF16)
            out[b, :, h], tight[b, :, h], loose[b, :, h] = o, t, loose_gate(t, delta[:, None], pv)
    return AttnRef(out, tight, loose)


def visibility_probe(B, S, H):
    """q = k = 0 (every visible score equal) and, in head h of batch entry b, V[j, d] = 1 iff j == (128 h + d + 37 b) % (128 H):
    the heads together name every key (128 H >= S), so out[i, h, d] != 0 exactly where the key of (h, d) is visible to row i, and
    then it is 1 / n_visible(i).  The two batch entries carry different V."""
    assert 128 * H >= S
    x = np.zeros((B, S, 3, H, 128), F32)
    key = np.zeros((B, H, 128), np.int64)
    for b in range(B):
        for h in range(H):
            key[b, h] = (128 * h + np.arange(128) + 37 * b) % (128 * H)
            ok = key[b, h] < S
            x[b, key[b, h][ok], 2, h, np.arange(128)[ok]] = 1
    return x.reshape(B * S, 3 * H * 128), key


def spiked_qkv(B, S, H, R0, Lc, seed):
    """Random q, k (sigma 1/2), v (sigma 1), plus — in head 0 of batch entry 0 — the last query of every suffix block set to 1.0
    everywhere, one prefix key (the last one the block sees, Lc - 1) to 1.5 and the block's sixth key to 3.0.  In the kernel's
    base-2 score units (x log2(e) / sqrt(128) = 0.1275 per unit of q . k) that query scores 24.5 at the prefix key and 49 at its
    own block's key, against a few units elsewhere: each outgrows the running maximum by more than the 2^16 that triggers the
    online-softmax rescale (the prefix key only when it is not in the first 32-key sub-tile, Lc > 32)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, H, 128, generator=g)
    x[:, :, :2] *= 0.5
    x = x.bfloat16().float().numpy()
    for blk in range(n_blocks(S, R0)):
        rows = block_rows(S, R0, blk)
        x[0, rows[-1], 0, 0] = 1.0
        x[0, rows[5], 1, 0] = 3.0
    x[0, Lc - 1, 1, 0] = 1.5
    return x.reshape(B * S, 3 * H * 128)


def block_sequences(qkv, B, S, H, R0, Lc):
    """Every suffix block as a sequence of its own, [prefix rows 0 .. Lc) ; block]: qkv2 [B * nb * (Lc + 32), 3 H 128]."""
    x = np.asarray(qkv, F32).reshape(B, S, -1)
    nb = n_blocks(S, R0)
    seqs = [np.concatenate([x[b, :Lc], x[b, block_rows(S, R0, blk)]]) for b in range(B) for blk in range(nb)]
    return np.concatenate(seqs), B * nb, Lc + 32


# ---------------------------------------------------------------- the doors' refusals (host only: nothing is launched)
EPI_NONE, EPI_RELU = 0, 3
TILE128, TILE256, TILE4W = 0x200, 0x400, 0x800
_FAKE = 0x10000                         # an aligned non-null pointer for calls that must be refused before any launch


def gemm_ex(ptr=None, **kw):
    """A vstar_gemm_ex.  Scalar fields by name; the pointer fields A, W, C, bias, residual, row_scale, sumsq_out, rope_cs take a
    device pointer, or True for `ptr(name)` (default: a fake aligned pointer — only for calls the door must refuse)."""
    from vstar_amd._lib import GemmEx
    g = GemmEx()
    for k, v in kw.items():
        if k in ("A", "W", "C", "bias", "residual", "row_scale", "sumsq_out", "rope_cs"):
            v = None if v is None or v is False else ((ptr(k) if ptr else _FAKE) if v is True else v)
        assert hasattr(g, k), k
        setattr(g, k, v)
    return g


def gemm_refusals():
    """(name, fields, fragment of the message): one violated precondition each, everything else valid."""
    b = dict(A=True, W=True, C=True, M=1024, N=768, K=128, lda=128, ldc=768, a_rows=1024, c_rows=1024, w_rows=768, epilogue=EPI_NONE)
    rope = dict(b, rope_cs=True, rope_rows=512, rope_S=512, rope_cols=512)
    amap = dict(a_group=103, a_gstride=128, a_off=25)
    cmap = dict(c_group=103, c_gstride=128, c_off=25)
    ext = extent(1024, RowMap(103, 128, 25))
    stats = dict(b, sumsq_out=True, sumsq_ld=24, stats_sum=12)
    return [
        ("tile4w_a_map", dict(b, **amap, a_rows=ext, epilogue=TILE4W), "VSTAR_EPI_TILE4W with a row map"),
        ("tile4w_c_map", dict(b, **cmap, c_rows=ext, epilogue=TILE4W), "VSTAR_EPI_TILE4W with a row map"),
        ("a_map_leaves_extent", dict(b, **amap, a_rows=ext - 1), f"mapped A row {ext - 1} outside a_rows"),
        ("c_map_leaves_extent", dict(b, **cmap, c_rows=ext - 1), f"mapped C row {ext - 1} outside c_rows"),
        ("identity_a_extent", dict(b, a_rows=1023), "mapped A row 1023"),
        ("identity_c_extent", dict(b, c_rows=1023), "mapped C row 1023"),
        ("c_map_overlaps", dict(b, c_group=103, c_gstride=100, c_off=0, c_rows=2048), "two rows to one"),
        ("w_rows", dict(b, w_rows=767), "W needs"),
        ("both_tiles", dict(b, epilogue=TILE128 | TILE256), "more than one tile override"),
        ("nosync", dict(b, epilogue=0x100), "unknown bits"),
        ("rope_tile128", dict(rope, epilogue=TILE128), "rope_cs with VSTAR_EPI_TILE128"),
        ("rope_epilogue", dict(rope, epilogue=EPI_RELU), "epilogue other than VSTAR_EPI_NONE"),
        ("rope_R0_and_tail", dict(rope, rope_R0=128, rope_Lc=100, rope_pos0=25, rope_tail=512), "rope_R0 together with rope_tail"),
        ("rope_table_short", dict(rope, rope_rows=511), "RoPE position 511 outside rope_rows"),
        ("rope_table_short_grouped", dict(rope, rope_S=288, rope_R0=128, rope_Lc=100, rope_rows=131), "RoPE position 131 outside rope_rows"),
        ("rope_table_short_prefix", dict(rope, rope_S=111, rope_pos0=25, rope_tail=999, rope_rows=135), "RoPE position 135 outside rope_rows"),
        ("rope_small_M", dict(rope, M=1000), "outside the 256 x 256 kernels' domain"),
        ("rope_cols", dict(rope, rope_cols=384), "rope_cols % 256"),
        ("rope_Lc_range", dict(rope, rope_R0=128, rope_Lc=129), "0 < rope_Lc <= rope_R0"),
        ("rope_with_sumsq", dict(rope, sumsq_out=True, sumsq_ld=12), "rope_cs with sumsq_out"),
        ("rope_fields_without_table", dict(b, rope_S=512), "without rope_cs"),
        ("stats_without_sumsq", dict(b, stats_sum=12), "stats_sum without sumsq_out"),
        ("stats_overlap", dict(stats, stats_sum=11), "stats_sum must be 0 or >= N / 64"),
        ("stats_ld", dict(stats, sumsq_ld=23), "sumsq_ld shorter"),
        ("sumsq_epilogue", dict(stats, epilogue=EPI_RELU), "sumsq_out: VSTAR_EPI_NONE"),
        ("tile256_domain", dict(b, M=1000, a_rows=1000, c_rows=1000, epilogue=TILE256), "VSTAR_EPI_TILE256"),
        ("tile4w_domain", dict(b, M=1030, a_rows=1030, c_rows=1030, epilogue=TILE4W), "VSTAR_EPI_TILE4W: call outside"),
    ]


def attention_refusals():
    """(name, (qkv_rows, out_rows, B, S, H, R0, Lc), fragment): the domain of grouped sequences and the extents."""
    return [
        ("R0_not_128", (288, 288, 1, 288, 2, 64, 32), "grp_R0 % 128"),
        ("Lc_zero", (288, 288, 1, 288, 2, 128, 0), "0 < grp_Lc <= grp_R0"),
        ("Lc_above_R0", (288, 288, 1, 288, 2, 128, 129), "0 < grp_Lc <= grp_R0"),
        ("suffix_not_32", (300, 300, 1, 300, 2, 128, 100), "(S - grp_R0) % 32"),
        ("R0_above_S", (96, 96, 1, 96, 2, 128, 100), "grp_R0 > S"),
        ("Lc_without_R0", (288, 288, 1, 288, 2, 0, 100), "grp_Lc without grp_R0"),
        ("qkv_extent", (575, 576, 2, 288, 2, 128, 100), "< B * S"),
        ("out_extent", (576, 575, 2, 288, 2, 128, 100), "< B * S"),
    ]
