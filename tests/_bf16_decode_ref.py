"""References, input builders and gates of the op tests of the bf16 DECODE kernels (tests/test_bf16_decode_gpu.py; pinned on the CPU by
tests/test_bf16_decode_ref.py): the bf16 build of decode.hip (rope_kv_append, the three cached-attention paths, embed_rows,
argmax_rows_lp) and of skinny.hip (gemm_skinny_kernel, gemm_skinny_ring_kernel, with and without the fused RMSNorm, 16-bit and fp32
output, the tile-major weight image).

Plain numpy.  bf16 values travel as float32 arrays whose low 16 bits are zero (tests/_prefill_ops_ref.py: bf, bits, is_bf16).  The
decode references are the ones of tests/_decode_ops_ref.py with the storage type BF16 in place of fp16; the GEMV probes and the
epilogue are the ones of tests/_gemm128_ref.py.  Unit roundoff: bf16 has 8 significand bits, u = 2^-8.

Gates (derived, not measured):
  TIGHT = 2u |o| + 4u sum p|v| + 2^-23 sum |v|            (tight_gate, u = 2^-8)
  LOOSE = TIGHT + (e^(2 delta) - 1) sum p|v|,  delta = 4u |s| + 2^-17 sum |q||k| / sqrt(128)      (the fp16 derivation, u substituted)

One-hot probes.  In bf16 a small probability does not flush to zero at 2^-25 as it does in fp16: the smallest bf16 subnormal is 2^-133.
Reference (float64 exp) and kernel (fp32 __expf, whatever its denormal mode) agree bit for bit only where exp(s_j - max) is 0 in fp32
for every non-target key, i.e. below 2^-150 = e^-103.97.  The probes therefore use q = 64 e_dq against a target key of 32 e_dq: the
target's score is bf(bf(2048) / sqrt(128)) = 181 against 0, a gap >= PROBE_GAP = 110 (checked by the CPU pin for every probe case).

`skinny_acc` restates the GEMV kernels' geometry — double steps of 64 k interleaved over 8 waves, the unrolled main loop and the tail
loop of the register kernel, the ring's main loop and two-phase tail, 16 columns (SiLU-mul: 16 gate + 16 up) per workgroup, row tiles
of 16 — only so that a FAULT of that geometry can be applied to the reference: the CPU test shows that every probe of the GPU test
changes under the fault it is meant to catch."""
import numpy as np
import torch

from tests import _decode_ops_ref as D
from tests._f16_prefill_ref import n_add, tie_slack as _tie_slack  # noqa: F401
from tests._gemm128_ref import act_bound, epilogue, fp32_sum_bound, index_probe, ktile_probe, unpack_gate_up  # noqa: F401  (re-exported)
from tests._prefill_ops_ref import F32, F64, SENT16, SENT32, bf, bits, int_operands, is_bf16  # noqa: F401  (re-exported)

U = 2.0 ** -8
PROBE_MAG = (64, 32)                   # q and target-key magnitude of the one-hot probes
PROBE_GAP = 110.0


def bf16_codes(n, seed, emin=97, emax=157):
    """n bf16 values, finite, normal, non-zero, biased exponent in [emin, emax] (default 2^-30 .. 2^30: sixty-one binades, so that
    no sum of two of them overflows); pairwise distinct bit patterns within every run of the pool's size."""
    c = np.arange(65536, dtype=np.int64)
    e = (c >> 7) & 0xFF
    c = c[(e >= emin) & (e <= emax)]
    g = np.random.default_rng(seed)
    out = np.concatenate([g.permutation(c) for _ in range((n + len(c) - 1) // len(c))])[:n]
    return (out.astype(np.uint32) << 16).view(F32)


BF16 = D.Storage("bf16", F32, U, torch.bfloat16, bf, bits, bf16_codes)


# ---------------------------------------------------------------- decode cases in bf16 (format 0 only)
def append_case(H, table="llama"):
    return D.append_case(H, 0, st=BF16, table=None if table == "llama" else (lambda rows, st: D.grid_table(rows, st)))


def probe_case(path, g, t):
    return D.probe_case(path, 0, g, t, st=BF16, mag=PROBE_MAG)


def exact_dot_case(path, g):
    return D.exact_dot_case(path, 0, g, st=BF16)


def random_case(path, g):
    return D.random_case(path, 0, g, st=BF16)


def probe_gap(c, ref):
    """The smallest s_target - s_j over the non-target keys of every (row, head) of a probe case (+inf where a row has one key)."""
    H = c.H
    K, qkv = c.K, c.qkv.reshape(c.R, 3, H, D.D)
    if c.path >= 1:
        K, qkv = ref.append.K, ref.append.qkv.reshape(c.R, 3, H, D.D)
    gap = np.inf
    for r in range(c.R):
        if c.row_pos[r] < 0:
            continue
        ks = c.key_slots(r)
        j = np.arange(len(ks))
        for hh in range(H):
            a = K[ks, hh, j].astype(F64) @ qkv[r, 0, hh].astype(F64)
            s = bf(bf(a).astype(F32) / D.SQRT_D).astype(F64)
            t = c.targets[r, hh]
            others = np.delete(s, t)
            if len(others):
                gap = min(gap, float(s[t] - others.max()))
    return gap


# ---------------------------------------------------------------- argmax_rows_lp: what only bf16 can hold
def _code(c):
    return float(np.array([c << 16], np.uint32).view(F32)[0])


NEG_AT_OR_BELOW = _code(0xFF62)        # -3.0041e38: the largest bf16 number <= -3e38 (the kernel's `best` starts at -3.0e38f)
NEG_JUST_ABOVE = _code(0xFF61)         # -2.9908e38: the next bf16 number above -3e38
NEG_MAX = _code(0xFF7F)                # -3.3895e38: the most negative finite bf16


def argmax_extreme_case(cols):
    """Rows [6, ld], ld = cols + 9, padding columns 1000.  With c = the last column (> 0 where cols > 1):
      0  every value NEG_MAX, NEG_AT_OR_BELOW at c: the largest value is finite and <= -3e38 -> 0 (kernels.hpp)
      1  every value NEG_MAX, NEG_JUST_ABOVE at c -> c
      2  -inf everywhere, NEG_JUST_ABOVE at c, NaN at 0 -> c
      3  NEG_AT_OR_BELOW everywhere, NaN at c -> 0 (NaN never wins)
      4  NEG_JUST_ABOVE at the middle column and at c, NEG_AT_OR_BELOW elsewhere -> the middle column (the first of a tie)
      5  NaN everywhere, NEG_JUST_ABOVE at c -> c"""
    ld = cols + 9
    c, mid = cols - 1, cols // 2
    x = np.full((6, ld), 1000.0, F32)
    x[0, :cols] = NEG_MAX
    x[0, c] = NEG_AT_OR_BELOW
    x[1, :cols] = NEG_MAX
    x[1, c] = NEG_JUST_ABOVE
    x[2, :cols] = -np.inf
    x[2, c] = NEG_JUST_ABOVE
    if cols > 1:
        x[2, 0] = np.nan
    x[3, :cols] = NEG_AT_OR_BELOW
    if cols > 1:
        x[3, c] = np.nan
    x[4, :cols] = NEG_AT_OR_BELOW
    x[4, mid] = x[4, c] = NEG_JUST_ABOVE
    x[5, :cols] = np.nan
    x[5, c] = NEG_JUST_ABOVE
    return x, ld


# ---------------------------------------------------------------- the weight-streaming GEMV (skinny.hip)
WAVES, STEP, COLS, ROWS = 8, 64, 16, 16
EPI_NONE, EPI_QUICK_GELU, EPI_GELU, EPI_RELU, EPI_SILU_MUL = range(5)
# the smallest shapes at which each mechanism is live.  M: one row, the ring's limit with (7) and without (8) the norm, the first
# register-only M (9), one full row tile and the first row of the second (16, 17), three row tiles (33), the largest M (64).
# N: one workgroup, an 8-column tail inside the third workgroup (40), seventeen workgroups past one 256-row block of W (272);
# packed SiLU-mul N: two and three gate | up workgroups.  K: 1, 7, 8, 9, 17 and 24 double steps — a wave without work, every wave
# one step, wave 0 two (the ring's threshold K = 512), a tail step behind the unrolled main loop, three ring stages, two ring rounds.
M_VALUES, N_VALUES, SILU_N, K_VALUES = (1, 7, 8, 9, 16, 17, 33, 64), (16, 40, 272), (64, 96), (64, 448, 512, 576, 1088, 1536)
# One K more, outside the k-step probe (2^48 - 1 is no fp32 number): up to K = 1536 a wave of the ring kernel has at most three stages
# and never enters its main loop (`i0 + 2 RD <= n`: six stages at depth 3, four at depth 2), the only place a ring slot is re-filled
# behind a counted wait.  K = 3072 = 48 double steps, six per wave: one trip (NT = 1) or two (NT = 2), then the tail.
RING_LOOP_K = 3072
KSTEP_SHAPES = [(1, 16, 64), (7, 40, 448), (8, 16, 512), (9, 40, 576), (16, 16, 1088), (17, 272, 1536), (33, 40, 1088), (64, 16, 1536),
                (1, 272, 1536), (8, 40, 1088), (7, 16, 576)]
INDEX_SHAPES = [(1, 40, 64), (7, 272, 512), (8, 40, 576), (9, 16, 448), (16, 40, 512), (17, 40, 1088), (33, 272, 64), (64, 40, 576)]
INT_SHAPES = [(1, 16, 512), (7, 40, 576), (8, 272, 64), (9, 40, 1088), (16, 16, 1536), (17, 16, 448), (33, 40, 512), (64, 272, 576),
              (8, 40, 3072)]
SILU_SHAPES = [(1, 64, 512), (8, 96, 576), (9, 64, 448), (33, 96, 1088), (7, 64, 3072)]
RANDOM_SHAPES = [(8, 272, 3072), (33, 40, 1088)]
NORM_SHAPES = [(1, 40, 512), (7, 16, 576), (8, 40, 1088), (16, 272, 512), (7, 40, 3072)]
TILED_SHAPES = [(1, 16, 512, EPI_NONE), (8, 272, 1088, EPI_NONE), (7, 64, 576, EPI_SILU_MUL), (8, 96, 1536, EPI_SILU_MUL)]


def ring_runs(M, K, norm=False):
    """Whether the dispatch takes gemm_skinny_ring_kernel (launch_skinny; VSTAR_SKINNY_RING unset)."""
    return M <= (7 if norm else 8) and K >= 512


def ring_depth(nt):
    return 3 if nt == 1 else 2


def wave_steps(nd, w, M, ring, nt=1):
    """(main, tail): the double steps wave w enters in the kernel's main loop and behind it.
    register kernel: UH double steps per main-loop trip (1 for one row tile, else 2), the tail loop takes what is left one by one.
    ring kernel: trips of RD stages while two full rounds are left, then up to 2 RD stages in two phases."""
    own = list(range(w, nd, WAVES))
    if ring:
        rd, n, i0 = ring_depth(nt), len(own), 0
        while i0 + 2 * rd <= n:
            i0 += rd
        return own[:i0], own[i0:]
    uh = 1 if (M + ROWS - 1) // ROWS == 1 else 2
    n_main = len(own) // uh * uh
    return own[:n_main], own[n_main:]


def skinny_acc(A, W, nt=1, ring=False, fault=None):
    """A . W^T in float64, [M, N], assembled the way the GEMV kernels do.  fault (None = none):
      ("drop_tail",)       every wave leaves out the last double step it takes behind its main loop
      ("neighbour", w)     wave w reads the double steps of wave (w + 1) % 8 instead of its own
      ("swap_tiles",)      nt = 2: the gate tile of every workgroup reads the up tile's W rows and the other way round
      ("row_clamp",)       row tiles clamp rows >= M - 1 to row M - 2 instead of rows >= M to row M - 1"""
    A, W = np.asarray(A, F64), np.asarray(W, F64)
    M, K = A.shape
    N, nd = W.shape[0], K // STEP
    kind = fault[0] if fault else None
    src = np.arange(M)
    if kind == "row_clamp" and M >= 2:
        src = np.minimum(src, M - 2)
    wrow = np.arange(N)
    if kind == "swap_tiles":
        assert nt == 2 and N % 32 == 0
        wrow = wrow.reshape(N // 32, 2, 16)[:, ::-1].reshape(N)
    C = np.zeros((M, N), F64)
    for w in range(WAVES):
        main, tail = wave_steps(nd, w, M, ring, nt)
        if kind == "neighbour" and w == fault[1]:
            main, tail = wave_steps(nd, (w + 1) % WAVES, M, ring, nt)
        if kind == "drop_tail":
            tail = tail[:-1]
        for ds in main + tail:
            k = slice(ds * STEP, (ds + 1) * STEP)
            C += A[src][:, k] @ W[wrow][:, k].T
    return C


def has_tail(M, K, ring, nt=1):
    return any(wave_steps(K // STEP, w, M, ring, nt)[1] for w in range(WAVES))


# ---------------------------------------------------------------- SiLU-mul where the sigmoid leaves the normal fp32 range
# The epilogue's sigmoid is v_rcp_f32(1 + v_exp_f32(-g)) (common.hpp: fast_sigmoid), and v_rcp_f32 has no subnormal results: for
# 1 + e^-g > 2^126, i.e. g < -126 ln 2 = -87.34, the kernel's sigmoid is 0 and SiLU(g) is -0, where float64 (and an IEEE fp32
# g / (1 + e^-g)) gives a value of magnitude |g| / (1 + e^-g) < |g| 2^-126 — a NORMAL bf16 number, because bf16 has fp32's exponent
# range; in fp16 the same value is below half the smallest subnormal and rounds to zero either way.  _gemm128_ref.epilogue does not
# model the flush, so EXACT holds for gate >= -87 only (e^87 = 0.71 x 2^126: a margin of 29 % against the error of v_exp_f32);
# below, the kernel may return anything between the reference and zero.
SIGMOID_NORMAL_FROM = -87.0


def silu_flush_region(acc):
    """[M, N / 2] bool: the outputs whose gate accumulator lies where the kernel's sigmoid may flush to zero."""
    gate, _ = unpack_gate_up(np.asarray(acc, F64))
    return bf(gate).astype(F64) < SIGMOID_NORMAL_FROM


def silu_flush_gate(acc):
    """|got - ref| in the flush region: at most the reference's own magnitude before the residual, |g| 2^-126 |bf(up)|, with one bf16
    rounding of each of the two factors' product (1 + 2^-7).  A residual only adds a common term, rounded the same way on both
    sides when the SiLU term vanishes against it; where it does not (residual 0) the difference is the term itself."""
    gate, up = unpack_gate_up(np.asarray(acc, F64))
    return 2.0 ** -126 * np.abs(bf(gate).astype(F64)) * np.abs(bf(up).astype(F64)) * (1 + 2.0 ** -7)


def kernel_silu_mul(acc, res=None):
    """The epilogue of VSTAR_EPI_SILU_MUL restated with the kernel's sigmoid: 0 where 1 + e^-g > 2^126 (fp32), else as float64."""
    gate, up = unpack_gate_up(np.asarray(acc, F64))
    g = bf(gate).astype(F64)
    with np.errstate(over="ignore"):
        d = (F32(1.0) + np.exp(-g).astype(F32)).astype(F64)
    sig = np.where(d > 2.0 ** 126, 0.0, 1.0 / (1.0 + np.exp(-g)))
    t = bf(g * sig).astype(F64) * bf(up).astype(F64)
    if res is not None:
        t = bf(t).astype(F64) + np.asarray(res, F64)
    return bf(t).astype(F64)


# ---------------------------------------------------------------- GELU and quick-GELU on integer operands
# The kernels' rounding points (gemm_epilogue.hpp, common.hpp), restated.  16-bit output:
#   t = bf(acc + bias)                                   exact accumulators and quarters: one deterministic rounding
#   GELU        a = 0.5 t (1 + erff(t / sqrt 2))         fp32, within ERF_ERR |t| of the float64 value (the bound
#                                                        tests/_f16_prefill_ref.py uses for the same expression: erff, two products, one add)
#   quick-GELU  u = bf(1.702f t); s = bf(sigmoid(u)); a = t s      1.702f t is ONE fp32 product, restated exactly; the sigmoid is
#               v_rcp_f32(1 + v_exp_f32(-u)): 1 ulp each and one add, within SIG_REL of the float64 value, and 0 where that value lies
#               below the normal fp32 range (see the SiLU section); t s is exact in fp32 (8 x 8 significant bits)
#   out = bf(a), or bf(bf(a) + residual)
# Rounding is monotone, so a kernel whose a (or sigmoid) lies in [x - e, x + e] stores a value in [round(x - e), round(x + e)]:
# `act16_interval` returns that interval.  It is ONE point — EXACT — wherever no rounding tie lies within e, and two neighbouring bf16
# numbers where one does; only where the activation underflows (|a| << e: GELU of t < -5) is it wider, by e itself.
# fp32 output (nothing rounded): t = acc + bias exactly; GELU as above; quick-GELU is t sigmoid(1.702f t) with the un-rounded
# argument — against float64 sigmoid(1.702 t) the argument is off by 2^-23 |x| (the constant and the product), which moves the sigmoid by
# at most |x| s (1 - s) 2^-23 <= 0.23 x 2^-23, and the sigmoid itself by SIG_REL s; the product and the residual add round once each.
ERF_ERR = 2.0 ** -20
SIG_REL = 2.0 ** -21
C1702 = F32(1.702)


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(t, F64)) / np.sqrt(2.0)).numpy())


def _sig64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, F64)))


def _bf64(x):
    return bf(x).astype(F64)


def act16_interval(acc, epi, bias=None, res=None):
    """(lo, hi), float64 arrays of bf16 values: what a kernel with the rounding points above may store."""
    t = _bf64(np.asarray(acc, F64) + (0 if bias is None else np.asarray(bias, F64)[None, :]))
    if epi == EPI_GELU:
        a, e = _gelu64(t), ERF_ERR * np.abs(t)
        ends = [a - e, a + e]
    else:
        assert epi == EPI_QUICK_GELU
        u = bf((C1702 * t.astype(F32)).astype(F32)).astype(F64)
        s = _sig64(u)
        s_lo = np.where(s * (1 + SIG_REL) < 2.0 ** -126 * 1.5, 0.0, s * (1 - SIG_REL))       # v_rcp_f32 has no subnormal results
        ends = [t * _bf64(s_lo), t * _bf64(s * (1 + SIG_REL))]
    outs = []
    for x in ends:
        x = _bf64(x)
        if res is not None:
            x = _bf64(x + np.asarray(res, F64))
        outs.append(x)
    return np.minimum(*outs), np.maximum(*outs)


def act32_ref(acc, epi, bias=None, res=None):
    """(reference, gate) of the fp32-output forms, float64."""
    t = np.asarray(acc, F64) + (0 if bias is None else np.asarray(bias, F64)[None, :])
    r = 0 if res is None else np.asarray(res, F64)
    if epi == EPI_GELU:
        a, e = _gelu64(t), ERF_ERR * np.abs(t)
    else:
        assert epi == EPI_QUICK_GELU
        s = _sig64(1.702 * t)
        a = t * s
        e = np.abs(t) * (SIG_REL * s + 0.23 * 2.0 ** -23 + 2.0 ** -126) + 2.0 ** -24 * np.abs(a)
    return a + r, e + 2.0 ** -24 * (np.abs(a) + np.abs(r))


GELU_SHAPES = [(8, 40, 1088), (33, 272, 576), (64, 16, 1536), (7, 40, 3072)]


# ---------------------------------------------------------------- the fused RMSNorm of the GEMV
def ulp_bf16(t):
    """Spacing of bf16 at |t| (float64 in and out; subnormal spacing 2^-133)."""
    a = np.abs(np.asarray(t, F64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.exp2(e - 7)


def tie_slack(t, err):
    """tests/_f16_prefill_ref.py::tie_slack with the bf16 spacing."""
    return _tie_slack(t, err, ulp_bf16)


def rmsnorm_ref(x, gamma, eps):
    """LlamaRMSNorm rows BEFORE the store rounding, float64: y = gamma * bf(x rstd), and the gate of tests/_f16_prefill_ref.py's
    rmsnorm_ref with u = 2^-8: 2u |y| + |gamma| tie_slack(t, (n_add / 2 + 4) 2^-24 |t|), t = x rstd."""
    x, gamma = np.asarray(x, F64), np.asarray(gamma, F64)
    t = x / np.sqrt((x ** 2).mean(axis=1, keepdims=True) + eps)
    y = gamma[None, :] * bf(t).astype(F64)
    err = (n_add(x.shape[1]) / 2 + 4) * 2.0 ** -24 * np.abs(t)
    return y, 2 * U * np.abs(y) + np.abs(gamma)[None, :] * tie_slack(t, err)


def norm_gemv_ref(x, gamma, W, eps):
    """The norm-fused GEMV with fp32 output against float64: C = y . W^T with y the un-rounded norm rows.  The gate: every operand
    y_k the kernel feeds the MFMA lies within the RMSNorm gate g_k of y_k, so the exact product moves by at most g . |W|^T; the fp32
    accumulation of K exact products in any order adds fp32_sum_bound on the operands' magnitudes |y| + g."""
    y, g = rmsnorm_ref(x, gamma, eps)
    Wd = np.asarray(W, F64)
    return y @ Wd.T, g @ np.abs(Wd).T + fp32_sum_bound(np.abs(y) + g, Wd)


def norm_inputs(M, K, seed):
    """Rows 0.3 + 2 N(0, 1) (even) and 50 + N(0, 1) (odd: mean >> std), a weight 1 + 0.1 N(0, 1): tests/_f16_prefill_ref.py::norm_inputs."""
    g = np.random.default_rng(seed)
    x = 0.3 + 2 * g.standard_normal((M, K))
    x[1::2] = 50 + g.standard_normal((len(x[1::2]), K))
    return bf(x), bf(1 + 0.1 * g.standard_normal(K))
