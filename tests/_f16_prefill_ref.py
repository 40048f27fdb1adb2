"""References, input builders and gates of the fp16 PREFILL op tests (tests/test_f16_prefill_gpu.py; pinned on the CPU by
tests/test_f16_prefill_ref.py): the -DVSTAR_LP_F16 build of attn2_kernel, layernorm_lp, rmsnorm_lp, add_bcast, vit_assemble_tokens
and the tile GEMMs above the weight-streaming domain.  Plain numpy / torch: h(x) is round-to-nearest-even to fp16, everything else
float64 unless said otherwise.  Every gate comes from the unit roundoff u = 2^-11 and the kernels' rounding points, never from
measured output.

Attention.  Reference: float64 softmax attention on the fp16 operands.  Gate per output element:
    loose_gate(tight_gate(o, sum p|v|, sum |v|, u), delta, sum p|v|) + 2^-24 sum_j |v_j|
(the two functions of _decode_ops_ref.py), delta = 2^-11 scale max_j sum_d |q_d k_jd|: the kernel rounds the pre-scaled query
q' = h(float32(q) scale log2e) ONCE, which moves a score by at most that; the last term covers probabilities that are fp16
subnormals (absolute error 2^-25 each, in units of a row sum that the first sub-tile's anchoring keeps >= 1).

Norms.  Reference: _small_ops_ref.layernorm_ex / rmsnorm_ex with rnd = rf16, the value BEFORE the store rounding.  Gate
2^-10 |ref| + atol (u for the store rounding, u of slack for every relative fp32 error), atol per element:
  * LayerNorm: the kernel's fp32 mean is a sum of `cols` numbers — per lane 8 ceil(cols / 512) sequential adds, then 6 butterfly levels —
    so its error is at most n_add 2^-24 mean|x|, n_add = 8 ceil(cols / 512) + 6; every (x - mean) is off by that, the output by
    A = n_add 2^-24 mean|x| rstd |gamma|.  On the "mean >> std" rows (50 + N(0, 1), 4096 columns) A = 70 * 6e-8 * 50 * 1 * 1.3 =
    2.7e-4; on the centred rows it is 1e-5.  (The bf16 tests' scalar 1e-2 is 37 x that: it also has to hold the bf16 ties below.)
    Plus 2^-22 (|a| + |beta|) for the affine's own fp32 operations where a + beta cancels.
  * A rounding INSIDE the kernel (RMSNorm's h(x rstd); act = 1: h(affine) before the GELU; the GEMM's h(silu(g))) can fall to the
    other side than the reference's where the exact value lies within the kernel's fp32 error of a rounding tie: `tie_slack`
    allows one fp16 step of the inner value THERE and nothing elsewhere (well under 1 % of the elements).
"""
import math

import numpy as np
import torch

from tests import _small_ops_ref as S
from tests._decode_ops_ref import F16, F32, F64, bits, h, loose_gate, tight_gate  # noqa: F401  (bits, h: re-exported)

U = 2.0 ** -11
BIG_BF16, BIG_F16 = 65536.0, 65504.0      # attn2's re-centre thresholds (attention.hip); fp16: every p <= rs <= BIG rounds to a finite value
F16_MAX_ROUNDS_FINITE = 65520.0           # the smallest value h() sends to +inf


def ulp16(t):
    """Spacing of fp16 at |t| (float64 in and out; subnormal spacing 2^-24)."""
    a = np.abs(np.asarray(t, F64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10)


def tie_slack(t, err, spacing=ulp16):
    """One step of the storage type (default fp16; `spacing` gives another format's) at t where t lies within err of a rounding tie
    (a kernel whose value of t is off by up to err may round to the other neighbour), 0 elsewhere."""
    t, err = np.asarray(t, F64), np.asarray(err, F64)
    sp = spacing(t)
    frac = np.abs(t) / sp
    dist = np.abs(frac - np.floor(frac) - 0.5) * sp
    return np.where(dist <= err, sp, 0.0)


# ================================================================ attention
ATTN_SHAPES = [(3, 33, 1, 128, 1), (1, 100, 2, 64, 1), (2, 257, 2, 64, 0), (1, 577, 2, 64, 0), (2, 320, 2, 128, 1), (1, 64, 1, 128, 0)]
RANGE_SHAPES = [(577, 2, 64, 0), (200, 1, 128, 1)]                         # (S, H, D, causal)
RANGE_PROFILES = ["ascending", "descending", "all_very_negative", "sawtooth"]
WINDOW_SHAPES = [(64, 0), (128, 1)]                                        # (D, causal)
WINDOW_S, WINDOW_H, WINDOW_SPIKES = 160, 2, (40, 100)


def attention_ref(qkv, B, S, H, D, causal):
    """qkv [B * S, 3 H D] fp16 -> (float64 attention [B * S, H * D], gate of the same shape)."""
    x = np.asarray(qkv, F16).reshape(B, S, 3, H, D).astype(F64)
    scale = 1.0 / math.sqrt(D)
    out, gate = np.zeros((B, S, H, D)), np.zeros((B, S, H, D))
    vis = np.tril(np.ones((S, S), bool)) if causal else np.ones((S, S), bool)
    for b in range(B):
        for hh in range(H):
            q, k, v = x[b, :, 0, hh], x[b, :, 1, hh], x[b, :, 2, hh]
            s = np.where(vis, (q @ k.T) * scale, -np.inf)
            e = np.exp(s - s.max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
            o = p @ v
            pv = p @ np.abs(v)
            vabs = vis.astype(F64) @ np.abs(v)
            delta = U * scale * np.where(vis, np.abs(q) @ np.abs(k).T, 0.0).max(axis=1)
            out[b, :, hh] = o
            gate[b, :, hh] = loose_gate(tight_gate(o, pv, vabs, U), delta[:, None], pv) + 2.0 ** -24 * vabs
    return out.reshape(B * S, H * D), gate.reshape(B * S, H * D)


def scale_log2e(D):
    """The kernel's fp32 constant: (1.0f / sqrtf(D)) * 1.4426950408889634f."""
    return F32(F32(1.0) / np.sqrt(F32(D))) * F32(1.4426950408889634)


def prescaled_q(q, D):
    """q' = h(float32(q) scale log2e)."""
    return h(np.asarray(q, F16).astype(F32) * scale_log2e(D))


def attn2_restated(qkv, B, S, H, D, causal, big=BIG_F16):
    """attn2_kernel's documented rounding points, restated: q' = h(float32(q) scale log2e); per wave (32 query rows) and 32-key
    sub-tile p = exp2(s - m) against the STALE reference m, re-centred on the wave's first sub-tile and whenever a lane's partial row
    sum (its 16 keys of the 32: those with bit 2 of the key offset equal) exceeds `big`; l sums the unrounded p, O sums h(p) v;
    o = h(O / l).  Scores in float64 rounded to fp32 (the MFMA accumulates in fp32 in an order this does not model).  fp16 out."""
    x = np.asarray(qkv, F16).reshape(B, S, 3, H, D)
    out = np.zeros((B, S, H, D), F16)
    half = (np.arange(32) >> 2) & 1
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for b in range(B):
            for hh in range(H):
                q = prescaled_q(x[b, :, 0, hh], D).astype(F64)
                k, v = x[b, :, 1, hh].astype(F64), x[b, :, 2, hh].astype(F64)
                for q0 in range(0, S, 32):
                    rows = np.arange(q0, min(q0 + 32, S))
                    n = len(rows)
                    m, l, O, first = np.zeros(n), np.zeros(n), np.zeros((n, D)), True
                    kend = min(S, (q0 // 128) * 128 + 128) if causal else S
                    for kt0 in range(0, kend, 32):
                        if causal and kt0 > q0 + 31:
                            break
                        keys = np.arange(kt0, kt0 + 32)
                        kc = np.minimum(keys, S - 1)
                        masked = (keys >= S)[None, :] | ((keys[None, :] > rows[:, None]) if causal else False)
                        s = np.where(masked, -1e30, (q[rows] @ k[kc].T).astype(F32).astype(F64) - m[:, None])
                        p = np.exp2(s.astype(F32)).astype(F64)
                        rs = np.stack([p[:, half == 0].sum(axis=1), p[:, half == 1].sum(axis=1)]).astype(F32)
                        if first or not (rs <= big).all():
                            mx = s.max(axis=1)
                            delta = np.maximum(mx, -1e4 if first else 0.0)
                            alpha = np.ones(n) if first else np.exp2(-delta)
                            l, O, m = l * alpha, O * alpha[:, None], m + delta
                            p = np.exp2((s - delta[:, None]).astype(F32)).astype(F64)
                            first = False
                        l = l + p.sum(axis=1)
                        O = O + h(p.astype(F32)).astype(F64) @ v[kc]
                    out[b, rows, hh] = h(O / l[:, None])
    return out.reshape(B * S, H * D)


def random_qkv(B, S, H, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * S, 3 * H * D, generator=g).numpy().astype(F16)


def spiked(qkv, B, S, H, D):
    """The spiked-key variant of test_ops_gpu.py::test_attention: one huge q.k at a late tile (forces the re-centring branch)."""
    x = qkv.copy().reshape(B, S, 3, H, D)
    x[0, S - 1, 0, 0] = 4.0
    x[0, S - 2, 1, 0] = 4.0
    return x.reshape(B * S, -1)


def range_qkv(S, H, D, profile):
    """The score profiles of test_ops_gpu.py::test_attention_softmax_dynamic_range: q[:, 0] = sqrt(D), so score(i, j) = k[j, 0] + noise."""
    g = torch.Generator().manual_seed(S + D + len(profile))
    x = 0.1 * torch.randn(1, S, 3, H, D, generator=g)
    j = torch.arange(S, dtype=torch.float32)
    ramp = {"ascending": 90.0 * j / S, "descending": 90.0 * (1 - j / S), "all_very_negative": torch.full((S,), -300.0),
            "sawtooth": 40.0 * ((j % 97) / 97.0) + 30.0 * (j // 97 % 2)}[profile]
    x[0, :, 0, :, 0] = math.sqrt(D)
    x[0, :, 1, :, 0] = ramp[:, None]
    x[0, :, 2] = torch.randn(S, H, D, generator=g)
    return x.view(S, -1).numpy().astype(F16)


# ---------------------------------------------------------------- the fp16 overflow window
def window_score(D, k0, k1):
    """The fp32 score of the spike key, in exp2 units, for q = (sqrt(D), 1, 0, ...): q'_0 k0 + q'_1 k1 (fp16 x fp16 products are exact
    in fp32; the sum is rounded once).  Returns (score as float32, q'_0, q'_1)."""
    qp = prescaled_q(np.array([math.sqrt(D), 1.0], F32).astype(F16), D).astype(F32)
    return F32(qp[0] * F32(k0)) + F32(qp[1] * F32(k1)), float(qp[0]), float(qp[1])


def window_spike_key(D, margin=1e-4):
    """Searches fp16 (k0, k1) so that the score lies in [log2 65520 + margin, 16 - margin]: exp2 of it is at most 65536 — the stale-m
    fast path of the bf16 threshold — and rounds to +inf in fp16.  k0 walks down from 16 / q'_0 in fp16 steps, k1 over [0.5, 1)."""
    lo, hi = math.log2(F16_MAX_ROUNDS_FINITE) + margin, 16.0 - margin
    _, q0, q1 = window_score(D, 0, 0)
    k0 = F16(16.0 / q0)
    k1s = (np.arange(1024, 2048) / 2048.0).astype(F16)            # every fp16 in [0.5, 1)
    for _ in range(64):
        k0 = np.nextafter(k0, F16(0))
        s = np.array([float(window_score(D, k0, k1)[0]) for k1 in k1s])
        okay = np.nonzero((s >= lo) & (s <= hi))[0]
        if len(okay):
            return F16(k0), F16(k1s[okay[0]])
    raise AssertionError("no spike key found")


def window_qkv(D, spike_at, seed=0):
    """S = 160, H = 2: q = (sqrt(D), 1, 0, ...) in every row; keys 0..31 are zero (scores exactly 0: the first sub-tile anchors m = 0
    in every wave); every other key has k_0 = -20 (p underflows to 0) but the spike key, which holds window_spike_key(D); V ~ N(0, 1)."""
    S, H = WINDOW_S, WINDOW_H
    g = torch.Generator().manual_seed(1000 + D + spike_at + seed)
    x = np.zeros((S, 3, H, D), F16)
    x[:, 0, :, 0], x[:, 0, :, 1] = math.sqrt(D), 1.0
    x[32:, 1, :, 0] = -20.0
    k0, k1 = window_spike_key(D)
    x[spike_at, 1, :, 0], x[spike_at, 1, :, 1] = k0, k1
    x[:, 2] = torch.randn(S, H, D, generator=g).numpy().astype(F16)
    return x.reshape(S, -1)


# ================================================================ norms
NORM_SHAPES = [(5, 8), (7, 72), (6, 256), (5, 4096)]                  # tests/test_small_ops_gpu.py::NORM_SHAPES
NORM_VARIANTS = [(0, True), (0, False), (1, True), (1, False)]        # (act, use_beta)


def norm_inputs(rows, cols, seed):
    """tests/test_small_ops_gpu.py::_norm_inputs in fp16: a source of rows + 4 rows — even ones 0.3 + 2 N(0, 1), odd ones
    50 + N(0, 1) (mean >> std) — and a row index into it (a permutation with one repeat)."""
    g = torch.Generator().manual_seed(seed)
    n_src = rows + 4
    x = 0.3 + 2 * torch.randn(n_src, cols, generator=g)
    x[1::2] = 50 + torch.randn(n_src // 2, cols, generator=g)
    idx = torch.randperm(n_src, generator=g)[:rows].to(torch.int32)
    idx[2] = idx[0]
    gam = (1 + 0.1 * torch.randn(cols, generator=g)).half()
    bet = (0.1 * torch.randn(cols, generator=g)).half()
    return x.half(), idx, gam, bet


def n_add(cols):
    """fp32 additions on the longest path of the kernels' row sums: 8 per 512 columns in a lane, then 6 butterfly levels."""
    return 8 * ((cols + 511) // 512) + 6


def layernorm_ref(x, gamma, beta, eps, idx, act):
    """(reference before the store rounding, gate), both float64 torch tensors [rows, cols]."""
    ref = S.layernorm_ex(x, gamma, beta, eps, idx, act, rnd=S.rf16)
    xs = x.double()[idx.long()]
    cols = xs.shape[-1]
    mean = xs.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + eps)
    a = (xs - mean) * rstd * gamma.double()
    b = beta.double().abs() if beta is not None else torch.zeros(cols, dtype=torch.float64)
    atol = n_add(cols) * 2.0 ** -24 * xs.abs().mean(-1, keepdim=True) * rstd * gamma.double().abs() + 2.0 ** -22 * (a.abs() + b)
    if act == 1:      # |gelu'| <= 1.13; the kernel's affine value is off by atol + the relative fp32 errors; erff: 2^-20 |t|
        t = S.layernorm_ex(x, gamma, beta, eps, idx, 0)
        err = atol + 2.0 ** -20 * t.abs()
        atol = 1.13 * (err + torch.from_numpy(tie_slack(t.numpy(), err.numpy()))) + 2.0 ** -20 * t.abs()
    return ref, 2.0 ** -10 * ref.abs() + atol


def rmsnorm_ref(x, gamma, eps, idx):
    """(reference before the store rounding, gate).  t = x rstd is off by (n_add / 2 + 4) 2^-24 |t| in the kernel (the sum of squares
    has only positive terms: a RELATIVE error of n_add 2^-24, halved by the square root; the divide, the rsqrt and the product)."""
    ref = S.rmsnorm_ex(x, gamma, eps, idx, rnd=S.rf16)
    xs = x.double()[idx.long()]
    t = xs / torch.sqrt((xs ** 2).mean(-1, keepdim=True) + eps)
    err = (n_add(xs.shape[-1]) / 2 + 4) * 2.0 ** -24 * t.abs()
    atol = gamma.double().abs() * torch.from_numpy(tie_slack(t.numpy(), err.numpy()))
    return ref, 2.0 ** -10 * ref.abs() + atol


# ================================================================ add_bcast / vit_assemble_tokens (EXACT)
LAYOUT_SHAPES = [(5, 8), (5, 72), (5, 768), (577, 8), (577, 72), (577, 768)]      # tests/test_small_ops_gpu.py::LAYOUT_SHAPES
ADD_BCAST_CASES = [(r, c, b) for r, c in LAYOUT_SHAPES + [(580, 72)] for b in (1, 5) if r % b == 0]
ASSEMBLE_CASES = [(3, 4, 72), (2, 256, 1024)]                                     # (B, P, C)


def f16_mid_codes(n, seed):
    """n fp16 values with pairwise distinct bit patterns within every run of the pool's size: finite, normal, magnitudes in
    [2^-8, 2^8) (biased exponent 7 .. 22: no overflow and no denormal result of one add)."""
    c = torch.arange(65536, dtype=torch.int64)
    e = (c >> 10) & 0x1F
    c = c[(e >= 7) & (e <= 22)]
    g = torch.Generator().manual_seed(seed)
    out = torch.cat([c[torch.randperm(len(c), generator=g)] for _ in range((n + len(c) - 1) // len(c))])[:n]
    return torch.where(out >= 32768, out - 65536, out).to(torch.int16).view(torch.float16)


def add_bcast(a, b):
    """out[r] = h(float32(a[r]) + float32(b[r % b_rows])): one fp32 add (exact or rounded once), one rounding."""
    idx = torch.arange(a.shape[0]) % b.shape[0]
    return (a.float() + b.float()[idx]).half()


def vit_assemble_tokens(patch, cls, pos):
    B = patch.shape[0]
    seq = torch.cat([cls.view(1, 1, -1).expand(B, 1, -1), patch], 1)
    return (seq.float() + pos.float()[None]).half()


# ================================================================ fp16 tile GEMM above the weight-streaming domain
GEMM_CASES = [(65, 320, 256, 2), (200, 130, 192, 2), (577, 1024, 640, 2), (1030, 300, 384, 5)]      # (M, N, K, kernel)
EPI_NONE, EPI_SILU_MUL = 0, 4


def gemm_inputs(M, N, K, epi, operands="exact", seed=0):
    """A [M, K], W [ceil(N / 256) 256, K] (rows >= N zero), bias [that many] (None for SILU_MUL), res [M, n_out] = h(0.5 N(0, 1)) (None
    for SILU_MUL) — numpy fp16.
    "exact": A and W are multiples of 1/8 in [-1, 1] and the bias a multiple of 1/64 in [-2, 2]: every product is a multiple of 1/64
    and |acc + bias| <= K + 2 < 2^24 / 64, so the fp32 accumulator and the bias add are EXACT in any order — the epilogue's roundings
    h(acc + bias), h(gate), h(up) are the reference's bit for bit and the gate is the issue's 2^-10 |ref| + 2^-22 sum |a w| as it
    stands.  |acc| reaches past 16, where multiples of 1/64 are no fp16 values: the roundings do round.
    "random": the operands of tests/test_vqa_gpu.py::test_weight_streaming_gemm (A = 0.5 N(0, 1), W = N(0, 1) / sqrt(K), bias =
    0.1 N(0, 1)).  The accumulator is then off by up to the gate's own 2^-22 sum |a w|, and where acc + bias (gate, up) lies within
    that of a rounding tie the kernel's h() may land one fp16 step from the reference's — which 2^-10 |ref| cannot hold once the
    residual cancels or the final rounding adds to it (measured on the MI355X: 1 .. 54 elements per case, 1e-4 of them, up to 33 x
    the plain gate).  gemm_ref(acc_err=True) allows that one step THERE (tie_slack) and nothing elsewhere, plus 2^-25 everywhere: random
    SiLU products reach below 2^-14, where the store rounds to an fp16 SUBNORMAL (half a step is 2^-25, not 2^-11 |ref|)."""
    rng = np.random.default_rng(7000 + M + N + K + epi + seed)
    Npad = (N + 255) // 256 * 256
    n_out = N // 2 if epi == EPI_SILU_MUL else N
    W, bias = np.zeros((Npad, K), F16), None
    if operands == "exact":
        A = (rng.integers(-8, 9, (M, K)) / 8.0).astype(F16)
        W[:N] = (rng.integers(-8, 9, (N, K)) / 8.0).astype(F16)
    else:
        A = h(0.5 * rng.standard_normal((M, K)))
        W[:N] = h(rng.standard_normal((N, K)) / math.sqrt(K))
    if epi == EPI_NONE:
        bias = np.zeros(Npad, F16)
        bias[:N] = (rng.integers(-128, 129, N) / 64.0).astype(F16) if operands == "exact" else h(0.1 * rng.standard_normal(N))
    res = None if epi == EPI_SILU_MUL else h(0.5 * rng.standard_normal((M, n_out)))
    return A, W, bias, res


def gemm_ref(A, W, bias, res, N, epi, acc_err=False):
    """float64 with the epilogue's rounding points (tests/test_vqa_gpu.py::test_weight_streaming_gemm): NONE = h(acc + bias) + res;
    SILU_MUL (W rows packed gate | up in blocks of 16 | 16, output N / 2 columns) = h(silu(h(gate))) * h(up).  Returns (reference
    before the store rounding [M, n_out], gate = 2^-10 |ref| + 2^-22 sum_k |a_k w_k| + tie slack).  The tie slack: always that of
    h(silu(g)) (the kernel's silu is fp32 with v_exp_f32 / v_rcp_f32, 1 ulp each, and two more fp32 operations: 2^-21 relative);
    acc_err: also that of the roundings of the accumulators, which are off by up to e = 2^-22 sum |a w| —
    one step of h(acc + bias); one step of h(gate) through |silu'| <= 1.1 plus one of h(silu); one step of h(up) — and 2^-25 for a
    store that rounds to an fp16 subnormal."""
    Af, Wf = A.astype(F64), W.astype(F64)
    acc = Af @ Wf.T
    aw = np.abs(Af) @ np.abs(Wf).T
    e = 2.0 ** -22 * aw
    if epi == EPI_NONE:
        t = acc[:, :N] + bias[:N].astype(F64)
        ref = h(t).astype(F64)
        if res is not None:
            ref = ref + res.astype(F64)
        slack = tie_slack(t, e[:, :N]) + 2.0 ** -25 if acc_err else 0.0
        return ref, 2.0 ** -10 * np.abs(ref) + e[:, :N] + slack
    n_out = N // 2
    c = np.arange(n_out)
    gi, ui = (c // 16) * 32 + c % 16, (c // 16) * 32 + 16 + c % 16
    g, u = h(acc[:, gi]).astype(F64), h(acc[:, ui]).astype(F64)
    silu = g / (1.0 + np.exp(-g))
    s = h(silu).astype(F64)
    ref = s * u
    slack = tie_slack(silu, 2.0 ** -21 * np.abs(silu)) * np.abs(u)
    if acc_err:
        g_tie = tie_slack(acc[:, gi], e[:, gi])
        slack = slack + np.where(g_tie > 0, 1.1 * g_tie + ulp16(silu), 0.0) * np.abs(u) + tie_slack(acc[:, ui], e[:, ui]) * np.abs(s) + 2.0 ** -25
    return ref, 2.0 ** -10 * np.abs(ref) + (np.abs(u) * e[:, gi] + np.abs(s) * e[:, ui]) + slack
