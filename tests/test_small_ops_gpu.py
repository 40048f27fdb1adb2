"""Operator-level parity of the small kernels on the MI355X — the OWL-ViT head finishers and the mask head's non-GEMM pieces
(heads.hip), the layout / broadcast / gather kernels (elementwise.hip), LayerNorm / RMSNorm with a row index and the fused GELU,
the LayerNorm statistics, scale_cols / fill (norm.hip), the fp8 row quantisers (quant.hip) and the SAM-head attention
(attention.hip) — each driven alone through its vstar_op_* door against tests/_small_ops_ref.py.

Conventions of every test:
  * inputs of pure data-movement kernels are DISTINCT bf16 codes, so any index error changes bits;
  * element counts are no multiples of 256 and row counts no multiples of 4: the last block is partly idle;
  * every output is allocated with padding rows / columns pre-filled with a sentinel that must come back bit-unchanged; every
    index a correct kernel touches lies inside the allocation;
  * EXACT = torch.equal on the raw bits.  STEP = |got - ref| <= 2^-7 |ref| + atol (one bf16 step, the gate of test_ops_gpu.py),
    atol derived per kernel in its docstring — from the reference and the rounding analysis, never from measured output.
    STEP tests print one `SMALLOP_ERR` line with the measured error and its share of the gate (run with -s to record them).
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _small_ops_ref as R

pytestmark = pytest.mark.gpu

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
NAN = float("nan")


class _Dev:
    """Copies host tensors to the device and keeps them alive until the test ends (a temporary's block would be handed to the next
    allocation of the same call)."""

    def __init__(self, dev):
        self.dev, self.keep = dev, []

    def __call__(self, t):
        self.keep.append(t.to(self.dev))
        return P(self.keep[-1])


@pytest.fixture
def dv(cuda):
    return _Dev(cuda)


def ok(lib, rc):
    assert rc == 0, lib.vstar_last_error(None)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def bf_codes(n, seed, emin=1, emax=254):
    """n bf16 values with pairwise distinct bit patterns (distinct within every run of 65024 when n is larger): finite, normal,
    non-zero, biased exponent in [emin, emax].  Arithmetic kernels get [119, 134] (2^-8 .. 2^7: no overflow, no denormal result)."""
    c = torch.arange(65536, dtype=torch.int64)
    e = (c >> 7) & 0xFF
    c = c[(e >= emin) & (e <= emax)]
    g = torch.Generator().manual_seed(seed)
    out = torch.cat([c[torch.randperm(len(c), generator=g)] for _ in range((n + len(c) - 1) // len(c))])[:n]
    return torch.where(out >= 32768, out - 65536, out).to(torch.int16).view(torch.bfloat16)


def mid_codes(n, seed):
    return bf_codes(n, seed, 119, 134)


class Out:
    """An output buffer [rows + pad_rows, ld] filled with a sentinel; `payload` marks what the kernel may write."""

    def __init__(self, dev, rows, cols, dtype, ld=None, pad_rows=2, sentinel=NAN, payload=None):
        ld = ld or cols
        self.full = torch.full((rows + pad_rows, ld), sentinel, dtype=dtype, device=dev)
        self.before = self.full.cpu().clone()
        if payload is None:
            payload = torch.zeros(rows + pad_rows, ld, dtype=torch.bool)
            payload[:rows, :cols] = True
        self.payload, self.rows, self.cols = payload, rows, cols

    def get(self):
        """The payload block on the CPU, after checking that everything else is bit-unchanged."""
        got = self.full.cpu()
        assert torch.equal(bits(got)[~self.payload], bits(self.before)[~self.payload]), "the kernel wrote outside its output"
        return got[: self.rows, : self.cols]


def step_check(name, shape, got, ref, atol, gate):
    """STEP gate; atol a float or a tensor like ref.  Prints the recorded-error line first."""
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    lim = ref.abs() * 2 ** -7 + atol
    print(f"SMALLOP_ERR {name} {shape}: abs {err.max().item():.3e} rel {(err.max() / ref.abs().max().clamp_min(1e-30)).item():.3e} "
          f"worst err/gate {(err / lim).max().item():.3f} [gate 2^-7|ref| + {gate}]")
    assert torch.isfinite(got).all()
    assert (err <= lim).all(), float((err / lim).max())


# ================================================================ elementwise.hip
@pytest.mark.parametrize("B,I,ps,kpad", [(2, 28, 14, 640), (1, 32, 16, 768), (3, 28, 14, 588)])
def test_im2col_patch(lib, cuda, dv, B, I, ps, kpad):
    """EXACT, pad columns zero.  (B * P * kpad = 5120 / 3072 / 7056 elements; P = 4: 8 / 4 / 12 rows.)"""
    pix = bf_codes(B * 3 * I * I, I + B).view(B, 3, I, I)
    rows = B * (I // ps) ** 2
    out = Out(cuda, rows, kpad, torch.bfloat16)
    ok(lib, lib.vstar_op_im2col_patch(None, dv(pix), P(out.full), B, I, ps, kpad))
    assert torch.equal(bits(out.get()), bits(R.im2col_patch(pix, ps, kpad)))


@pytest.mark.parametrize("B,Pn,C", [(3, 4, 72), (2, 256, 1024)])
def test_vit_assemble_tokens(lib, cuda, dv, B, Pn, C):
    """EXACT vs (a.float() + pos.float()).bfloat16(), the class row of every batch included."""
    patch, cls, pos = mid_codes(B * Pn * C, 1).view(B, Pn, C), mid_codes(C, 2), mid_codes((Pn + 1) * C, 3).view(Pn + 1, C)
    out = Out(cuda, B * (Pn + 1), C, torch.bfloat16)
    ok(lib, lib.vstar_op_vit_assemble_tokens(None, dv(patch), dv(cls), dv(pos), P(out.full), B, Pn, C))
    assert torch.equal(bits(out.get()), bits(R.vit_assemble_tokens(patch, cls, pos).view(-1, C)))


@pytest.mark.parametrize("img_col", [0, 3, 8])
def test_llm_embed_text(lib, cuda, dv, img_col):
    """EXACT; the P image rows keep their sentinel; ids < 0 clamp to 0, ids >= vocab to vocab - 1."""
    L, Pn, B, C, vocab = 9, 4, 2, 72, 50
    g = torch.Generator().manual_seed(img_col)
    ids = torch.randint(0, vocab, (B, L), generator=g, dtype=torch.int32)
    ids[:, img_col] = -200
    ids[0, (img_col + 2) % L], ids[1, (img_col + 4) % L], ids[1, (img_col + 5) % L] = -7, vocab, vocab + 1000
    table = bf_codes(vocab * C, 5).view(vocab, C)
    S = L - 1 + Pn
    payload = torch.zeros(B * S + 2, C, dtype=torch.bool)
    payload[: B * S] = True
    payload.view(-1)[: B * S * C].view(B, S, C)[:, img_col: img_col + Pn] = False
    out = Out(cuda, B * S, C, torch.bfloat16, sentinel=123.0, payload=payload)
    ok(lib, lib.vstar_op_llm_embed_text(None, dv(ids), L, img_col, Pn, dv(table), vocab, P(out.full), B, C))
    want = R.llm_embed_text(ids, img_col, Pn, table, out.before[: B * S].view(B, S, C))
    assert torch.equal(bits(out.get()), bits(want.view(-1, C)))


LAYOUT_SHAPES = [(5, 8), (5, 72), (5, 768), (577, 8), (577, 72), (577, 768)]


@pytest.mark.parametrize("rows,cols,b_rows", [(r, c, b) for r, c in LAYOUT_SHAPES + [(580, 72)] for b in (1, 5) if r % b == 0])
def test_add_bcast(lib, cuda, dv, rows, cols, b_rows):
    """EXACT: one rounding of an fp32 add."""
    a, b = mid_codes(rows * cols, 1).view(rows, cols), mid_codes(b_rows * cols, 2).view(b_rows, cols)
    out = Out(cuda, rows, cols, torch.bfloat16)
    ok(lib, lib.vstar_op_add_bcast(None, dv(a), dv(b), P(out.full), rows, cols, b_rows))
    assert torch.equal(bits(out.get()), bits(R.add_bcast(a, b)))


@pytest.mark.parametrize("rows_per,cols", LAYOUT_SHAPES)
@pytest.mark.parametrize("rep", [1, 3])
def test_add_bcast_repeat(lib, cuda, dv, rows_per, cols, rep):
    """EXACT; two source blocks, the last repeat of the second one not asked for when rep > 1."""
    n_out = 2 * rep - (1 if rep > 1 else 0)
    a, b = mid_codes(2 * rows_per * cols, 3).view(2 * rows_per, cols), mid_codes(cols, 4).view(1, cols)
    out = Out(cuda, n_out * rows_per, cols, torch.bfloat16)
    ok(lib, lib.vstar_op_add_bcast_repeat(None, dv(a), dv(b), P(out.full), n_out, rep, rows_per, cols))
    assert torch.equal(bits(out.get()), bits(R.add_bcast_repeat(a, b, n_out, rep, rows_per)))


@pytest.mark.parametrize("nrows,cols", LAYOUT_SHAPES)
def test_bcast_rows(lib, cuda, dv, nrows, cols):
    """EXACT with ld > cols and rep_stride > nrows: the columns past cols and the rows between the copies keep their sentinel."""
    nrep, ld, rep_stride = 3, cols + 8, nrows + 3
    src = bf_codes(nrows * ld, 6).view(nrows, ld)
    payload = torch.zeros(nrep * rep_stride + 2, ld, dtype=torch.bool)
    for r in range(nrep):
        payload[r * rep_stride: r * rep_stride + nrows, :cols] = True
    out = Out(cuda, nrep * rep_stride, ld, torch.bfloat16, sentinel=123.0, payload=payload)
    ok(lib, lib.vstar_op_bcast_rows(None, dv(src), P(out.full), nrep, rep_stride, nrows, cols, ld))
    assert torch.equal(bits(out.get()), bits(R.bcast_rows(src, out.before[: nrep * rep_stride], nrep, rep_stride, nrows, cols)))


@pytest.mark.parametrize("rows,cols", LAYOUT_SHAPES)
def test_owl_cls_mul(lib, cuda, dv, rows, cols):
    """EXACT: one rounding of an fp32 product; N - 1 = rows patch tokens per crop, 2 crops."""
    x = mid_codes(2 * (rows + 1) * cols, 7).view(2, rows + 1, cols)
    out = Out(cuda, 2 * rows, cols, torch.bfloat16)
    ok(lib, lib.vstar_op_owl_cls_mul(None, dv(x), P(out.full), 2, rows + 1, cols))
    assert torch.equal(bits(out.get()), bits(R.owl_cls_mul(x).view(-1, cols)))


@pytest.mark.parametrize("rows,cols", LAYOUT_SHAPES)
def test_gather_rows(lib, cuda, dv, rows, cols):
    """EXACT with reversed and repeated indices into a larger source."""
    x = bf_codes((rows + 3) * cols, 8).view(rows + 3, cols)
    idx = torch.arange(rows + 2, 2, -1, dtype=torch.int32)                   # reversed
    idx[1::3] = idx[0]                                                       # repeats
    idx[-1] = 0
    out = Out(cuda, rows, cols, torch.bfloat16)
    ok(lib, lib.vstar_op_gather_rows(None, dv(x), dv(idx), P(out.full), rows, cols))
    assert torch.equal(bits(out.get()), bits(R.gather_rows(x, idx)))


@pytest.mark.parametrize("cols", [1, 255, 257, 32003])
@pytest.mark.parametrize("out_stride", [1, 3])
def test_argmax_rows(lib, cuda, dv, cols, out_stride):
    """EXACT vs torch.argmax (first occurrence; NaN is the maximum).  The columns between cols and ld hold 1e9: a kernel that reads
    past the row finds them.  Rows: ties in neighbouring lanes / the next wave / the next 256-column stride, the maximum in the last
    column, all -inf, +inf among ties, all NaN, NaN twice next to +inf."""
    g = torch.Generator().manual_seed(cols)
    inf = float("inf")
    at = lambda *pos: sorted({min(max(p, 0), cols - 1) for p in pos})        # noqa: E731
    rows_spec = [
        (7.0, at(cols // 3, cols - 1)), (7.0, at(cols // 2, cols // 2 + 1, cols // 2 + 64)), (7.0, at(130, 130 + 256, 130 + 512)),
        (7.0, at(3, 256 + 3)), (7.0, at(cols - 1)), (None, "-inf"), (inf, at(cols // 2)), (None, "nan"), (NAN, at(cols // 2, cols - 1)),
    ]
    rows, ld = len(rows_spec), cols + 5
    x = torch.full((rows, ld), 1e9)
    x[:, :cols] = torch.rand(rows, cols, generator=g) * 2 - 1
    for r, (val, where) in enumerate(rows_spec):
        if where == "-inf":
            x[r, :cols] = -inf
        elif where == "nan":
            x[r, :cols] = NAN
        else:
            x[r, where] = val
    x[6, at(0, cols - 2)] = 7.0
    if cols > 1:
        x[8, 0] = inf                                                        # +inf BEFORE the first NaN: NaN still wins
    payload = torch.zeros(rows + 2, out_stride, dtype=torch.bool)
    payload[:rows, 0] = True
    out = Out(cuda, rows, 1, torch.int32, ld=out_stride, sentinel=-77, payload=payload)
    ok(lib, lib.vstar_op_argmax_rows(None, dv(x), rows, cols, ld, P(out.full), out_stride))
    got = out.get()[:, 0]
    assert ((got >= 0) & (got < cols)).all(), got.tolist()
    assert got.tolist() == R.argmax_rows(x[:, :cols]).tolist()


# ================================================================ norm.hip
NORM_SHAPES = [(5, 8), (7, 72), (6, 256), (5, 4096)]


def _norm_inputs(rows, cols, seed):
    """A source of rows + 4 rows — even ones 0.3 + 2 N(0, 1), odd ones 50 + N(0, 1) (mean >> std) — and a row index into it: a
    permutation with repeats, so that taking `row` for `row_index[row]` on either side shows."""
    g = torch.Generator().manual_seed(seed)
    n_src = rows + 4
    x = 0.3 + 2 * torch.randn(n_src, cols, generator=g)
    x[1::2] = 50 + torch.randn((n_src) // 2, cols, generator=g)
    idx = torch.randperm(n_src, generator=g)[:rows].to(torch.int32)
    idx[2] = idx[0]
    gam = (1 + 0.1 * torch.randn(cols, generator=g)).bfloat16()
    bet = (0.1 * torch.randn(cols, generator=g)).bfloat16()
    return x.bfloat16(), idx, gam, bet


@pytest.mark.parametrize("rows,cols", NORM_SHAPES)
@pytest.mark.parametrize("act,use_beta", [(0, True), (0, False), (1, True), (1, False)])
def test_layernorm_ex(lib, cuda, dv, rows, cols, act, use_beta):
    """STEP, atol 1e-2 (the LayerNorm gate of test_ops_gpu.py: |y| <= ~5 here, so one bf16 step of y is <= 2^-7 * 4 = 3e-2 relative
    part + the fp32 statistics' error on the mean >> std rows, which the absolute term covers).  act = 1: the reference rounds the
    affine result to bf16 before the exact-erf GELU."""
    x, idx, gam, bet = _norm_inputs(rows, cols, rows * 31 + cols + act)
    out = Out(cuda, rows, cols, torch.bfloat16)
    ok(lib, lib.vstar_op_layernorm_ex(None, dv(x), dv(gam), dv(bet) if use_beta else None, P(out.full), rows, cols,
                                      1e-6, dv(idx), act))
    ref = R.layernorm_ex(x, gam, bet if use_beta else None, 1e-6, idx, act)
    step_check("layernorm_ex", f"r{rows} c{cols} act{act} beta{int(use_beta)}", out.get(), ref, 1e-2, "1e-2")


@pytest.mark.parametrize("rows,cols", NORM_SHAPES)
def test_rmsnorm_ex(lib, cuda, dv, rows, cols):
    """STEP, atol 1e-2; rlp(x * rstd) before the weight multiply."""
    x, idx, gam, _ = _norm_inputs(rows, cols, rows * 17 + cols)
    out = Out(cuda, rows, cols, torch.bfloat16)
    ok(lib, lib.vstar_op_rmsnorm_ex(None, dv(x), dv(gam), P(out.full), rows, cols, 1e-6, dv(idx)))
    step_check("rmsnorm_ex", f"r{rows} c{cols}", out.get(), R.rmsnorm_ex(x, gam, 1e-6, idx), 1e-2, "1e-2")


def test_norm_ex_without_row_index_equals_the_plain_doors(lib, cuda, dv):
    x, _, gam, bet = _norm_inputs(7, 72, 99)
    xd, gd, bd = x[:7].contiguous().to(cuda), gam.to(cuda), bet.to(cuda)
    y = [torch.empty_like(xd) for _ in range(4)]
    ok(lib, lib.vstar_op_layernorm(None, P(xd), P(gd), P(bd), P(y[0]), 7, 72, 1e-5))
    ok(lib, lib.vstar_op_layernorm_ex(None, P(xd), P(gd), P(bd), P(y[1]), 7, 72, 1e-5, None, 0))
    ok(lib, lib.vstar_op_rmsnorm(None, P(xd), P(gd), P(y[2]), 7, 72, 1e-6))
    ok(lib, lib.vstar_op_rmsnorm_ex(None, P(xd), P(gd), P(y[3]), 7, 72, 1e-6, None))
    assert torch.equal(bits(y[0]), bits(y[1])) and torch.equal(bits(y[2]), bits(y[3]))


@pytest.mark.parametrize("rows,cols", [(5, 64), (6, 768), (5, 4096), (3, 8192)])
def test_ln_rstd(lib, cuda, dv, rows, cols):
    """vs fp64 1 / sqrt(var + eps).  Even rows are N(0, 1): rtol 1e-5.  Odd rows have |mean| / std = 30: the kernel forms
    var = E[x^2] - E[x]^2 in fp32, E[x^2] ~ mean^2 carries a relative error of up to sqrt(cols) * 2^-24 from its fp32 summation, i.e.
    (mean / std)^2 * sqrt(cols) * 2^-24 relative to var and half of that in rstd; the bound below allows twice that
    ((mean / std)^2 * 2^-23 * sqrt(cols)), computed from the inputs.  The partials form gets sums built on the host in torch's
    summation order (vstar_op_gemm_norm does not expose stats_sum, so the epilogue's own partials are not reachable from here):
    it is held to the same bounds rather than to bit-identity, and its NaN padding past 2 * cols / 64 must not be read.
    The two forms are also compared with EACH OTHER on the N(0, 1) rows.  They share the reduction across spans and the final
    formula and differ only in the order in which each span's 64 terms are added: whatever that order, a sum of 64 non-negative
    fp32 terms is within 63 * 2^-24 of the exact one, so the two sums of squares differ by at most 2 * 63 * 2^-24 relative, the
    shared butterfly (6 levels, at most 2 passes) on differently rounded inputs adds at most 2 * 8 * 2^-24, the mean^2 term is
    ~ 1 / cols of var and its difference negligible; rstd carries half the relative difference of var, and rsqrtf one fp32 ulp
    (2^-23) per side: rtol = 71 * 2^-24 + 2^-22 = 4.5e-6, tighter than what two results each within 1e-5 of fp64 would imply.
    With neither x nor partials the door returns an error without launching."""
    g = torch.Generator().manual_seed(cols)
    x = torch.randn(rows, cols, generator=g)
    x[1::2] += 30.0
    x = x.bfloat16()
    eps = 1e-5
    xd = x.double()
    ref = R.ln_rstd(x, eps)
    bound = torch.maximum(torch.tensor(1e-5, dtype=torch.float64),
                          (xd.mean(-1) / xd.std(-1, unbiased=False)) ** 2 * 2.0 ** -23 * math.sqrt(cols))
    ld = 2 * (cols // 64) + 3
    forms = {}
    for name, args in (("rows", (dv(x), None, 0)), ("partials", (None, dv(R.ln_partials(x, ld)), ld))):
        out = Out(cuda, rows, 1, torch.float32, pad_rows=3)
        ok(lib, lib.vstar_op_ln_rstd(None, args[0], args[1], args[2], rows, cols, eps, P(out.full)))
        got = out.get()[:, 0].double()
        rel = (got - ref).abs() / ref
        print(f"SMALLOP_ERR ln_rstd/{name} r{rows} c{cols}: rel N(0,1) rows {rel[0::2].max().item():.3e} [gate 1e-5]  "
              f"mean/std=30 rows {rel[1::2].max().item():.3e} [gate {bound[1::2].min().item():.3e} = (mean/std)^2 2^-23 sqrt(cols)]")
        assert (rel <= bound).all(), (rel / bound).max()
        forms[name] = got
    between = ((forms["rows"] - forms["partials"]).abs() / forms["partials"])[0::2].max().item()
    rtol = 71 * 2.0 ** -24 + 2.0 ** -22
    print(f"SMALLOP_ERR ln_rstd/rows-vs-partials r{rows} c{cols}: rel N(0,1) rows {between:.3e} [gate {rtol:.3e} = 71 2^-24 + 2^-22]")
    assert between <= rtol
    assert lib.vstar_op_ln_rstd(None, None, None, ld, rows, cols, eps, P(out.full)) != 0


@pytest.mark.parametrize("rows,K", [(5, 8), (300, 72)])
def test_scale_cols(lib, cuda, dv, rows, K):
    """EXACT, in place; the rows after `rows` are untouched."""
    W, w = mid_codes((rows + 2) * K, 11).view(rows + 2, K), mid_codes(K, 12)
    payload = torch.zeros(rows + 2, K, dtype=torch.bool)
    payload[:rows] = True
    out = Out(cuda, rows, K, torch.bfloat16, payload=payload)
    out.full.copy_(W)
    out.before = W.clone()
    ok(lib, lib.vstar_op_scale_cols(None, P(out.full), dv(w), rows, K))
    assert torch.equal(bits(out.get()), bits(R.scale_cols(W[:rows], w)))


@pytest.mark.parametrize("n", [1, 257])
def test_fill(lib, cuda, dv, n):
    out = Out(cuda, 1, n, torch.bfloat16, ld=n + 7, sentinel=123.0)
    ok(lib, lib.vstar_op_fill(None, P(out.full), n, 0.3))
    assert torch.equal(bits(out.get()[0]), bits(R.fill(n, 0.3)))


# ================================================================ heads.hip
@pytest.mark.parametrize("Q", [64, 72, 512])
@pytest.mark.parametrize("B,img_div", [(3, 1), (6, 3)])
def test_owl_class_logits(lib, cuda, dv, Q, B, img_div):
    """STEP with atol = 2^-7 * (elu(scale) + 1): |dot| <= 1 (normalised vectors) and |shift| <= 1 by construction, so dot + shift
    lies in [-2, 2] where one bf16 step is <= 2^-7; a flipped rounding of it (fp32 vs fp64 summation) moves the logit by that step
    times the multiplier.  15 / 30 rows -> 4 / 8 blocks of four, the last partly idle; the 4 columns after `scale` hold 1e9.
    That gate alone cannot see ONE missing rounding point (its effect is one flipped final rounding, the size of the gate), so
    the outputs are also counted against the ROUNDED reference bit for bit: a correct kernel differs from it only where the fp32
    order of a Q-term sum lands on the other side of a bf16 boundary — relative sum error <= Q 2^-24 against a half step of 2^-9,
    i.e. a flip chance <= 512 * 2^-15 = 1.6 % per rounding point and far less in the mean — so of the 15 / 30 outputs at most 2
    may differ, while a dropped or misplaced rounding double-rounds every output and changes about a quarter of them."""
    rows_per, ld, stride = 5, Q + 6, 11
    crops = B // img_div
    g = torch.Generator().manual_seed(Q + B)
    emb = torch.full((crops * rows_per + 1, ld), 1e9)
    emb[:, :Q] = torch.randn(crops * rows_per + 1, Q, generator=g)
    emb[:, Q] = torch.rand(crops * rows_per + 1, generator=g) * 2 - 1
    emb[:, Q + 1] = torch.randn(crops * rows_per + 1, generator=g) * 2
    emb[1, Q + 1], emb[3, Q + 1] = 1.5, -1.5                                 # both ELU branches for certain
    emb[2, :Q] = 0                                                           # an all-zero embedding row
    query = torch.randn(B, Q, generator=g).bfloat16()
    query[1] = 0                                                             # an all-zero query
    out = Out(cuda, B, rows_per, torch.float32, ld=stride, pad_rows=1)
    ok(lib, lib.vstar_op_owl_class_logits(None, dv(emb), ld, Q, dv(query), P(out.full), stride, B, rows_per, img_div))
    got = out.get()
    ref, mult = R.owl_class_logits(emb[:-1], Q, query, rows_per, img_div)
    assert torch.equal(got, got.bfloat16().float())                          # stored values are bf16-representable
    step_check("owl_class_logits", f"Q{Q} B{B} div{img_div}", got, ref, 2 ** -7 * mult, "2^-7 (elu(scale)+1)")
    differ = int((got.double() != R.rbf(ref)).sum())
    print(f"SMALLOP_ERR owl_class_logits/bits Q{Q} B{B} div{img_div}: {differ} of {got.numel()} outputs differ from the rounded reference [gate <= 2]")
    assert differ <= 2


@pytest.mark.parametrize("grid", [1, 5, 24])
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("img_div", [1, 2])
def test_owl_box_finish(lib, cuda, dv, grid, ld, img_div):
    """|err| <= 2^-8 (1 + |v| / 4), v the bf16 pre-sigmoid value: the output's own rounding is half a bf16 step of a value <= 1
    (2^-9), a flipped rounding of v (one step, <= 2^-7 |v|) moves the sigmoid by <= 2^-7 max(|v| sigmoid'(v)) = 2^-7 * 0.224 < 2^-9, and
    the fp32 logf / log1pf / expf errors are far below both; the |v| / 4 term is slack on top.  The last grid column (x = grid, coord = 1: the clip and the
    log1p(-1 + 1e-4) branch) and the last grid row are asserted separately.  Outputs lie in (0, 1]: with raw <= 6 on top of the
    coord = 1 bias of 9.21 the sigmoid exceeds 1 - 2^-9 and ROUNDS to 1.0 in bf16, in the reference as in the kernel."""
    B, n = 2, grid * grid
    crops = B // img_div
    g = torch.Generator().manual_seed(grid * 10 + ld)
    raw = torch.full((crops * n + 1, ld), 1e9)
    raw[:, :4] = 12 * torch.rand(crops * n + 1, 4, generator=g) - 6
    stride = n * 4 + 3
    out = Out(cuda, B, n * 4, torch.float32, ld=stride, pad_rows=1)
    ok(lib, lib.vstar_op_owl_box_finish(None, dv(raw), ld, P(out.full), stride, B, grid, img_div))
    got = out.get().view(B, n, 4)
    ref, v = R.owl_box_finish(raw[:-1], grid, B, img_div)
    assert torch.equal(got, got.bfloat16().float())
    assert ((got > 0) & (got <= 1)).all()
    assert ((got < 1) | (ref >= 1 - 2.0 ** -8)).all()                        # exactly 1.0 only within one bf16 step of it
    err, lim = (got.double() - ref).abs(), 2.0 ** -8 * (1 + v.abs() / 4)
    print(f"SMALLOP_ERR owl_box_finish g{grid} ld{ld} div{img_div}: abs {err.max().item():.3e} worst err/gate {(err / lim).max().item():.3f} "
          f"[gate 2^-8 (1 + |v|/4)]")
    assert (err <= lim).all()
    edge_bias = math.log(1.0001) - math.log1p(-1 + 1e-4)                     # 9.2104...
    p = torch.arange(n)
    for c, sel in ((0, p % grid == grid - 1), (1, p // grid == grid - 1)):
        crop = torch.arange(B) // img_div
        r = raw[:-1].view(crops, n, ld)[crop][:, sel, c]
        want = torch.sigmoid(R.rbf(R.rbf(r) + edge_bias))
        assert ((got[:, sel, c].double() - want).abs() <= 2.0 ** -8 * (1 + R.rbf(R.rbf(r) + edge_bias).abs() / 4)).all()
        assert (got[:, sel, c] > 0.9).all()                                  # v >= 9.21 - 6: a wrong branch (bias -> -inf / NaN) cannot pass


@pytest.mark.parametrize("B,h,w,C", [(1, 1, 1, 8), (2, 3, 5, 8), (1, 6, 6, 32)])
def test_upsample2x_im2col3x3(lib, cuda, dv, B, h, w, C):
    """EXACT.  Inputs are distinct values +-m 2^e (m in [128, 256), e in [-7, -2]): every blend with the weights 1, 3, 9 sixteenths
    is exact in fp32, so the only rounding is the final one to bf16 — checked here on the CPU first: torch's fp32 interpolate and
    the fp64 reference agree bit for bit on these inputs.  Zero padding of all nine taps at the four borders and corners shows
    because no input is zero."""
    g = torch.Generator().manual_seed(h * 7 + w)
    m = torch.arange(128, 256, dtype=torch.float64)
    pool = torch.cat([s * m * 2.0 ** e for s in (1, -1) for e in range(-7, -1)])
    src = pool[torch.randperm(len(pool), generator=g)[: B * h * w * C]].float().bfloat16().view(B, h, w, C)
    assert len(torch.unique(bits(src))) == src.numel()
    torch_up = F.interpolate(src.permute(0, 3, 1, 2).float(), scale_factor=2, mode="bilinear").bfloat16().permute(0, 2, 3, 1)
    assert torch.equal(bits(R.upsample2x(src)), bits(torch_up))
    rows = B * 4 * h * w
    out = Out(cuda, rows, 9 * C, torch.bfloat16)
    ok(lib, lib.vstar_op_upsample2x_im2col3x3(None, dv(src), P(out.full), B, h, w, C))
    assert torch.equal(bits(out.get()), bits(R.upsample2x_im2col3x3(src)))


def test_hyper_mask(lib, cuda, dv):
    """STEP with atol = 2^-8 * sum_c |h_c| |u_c| per element: the fp32 accumulation differs from fp64 by far less (32 terms), but a
    sum that cancels can land on the other side of a bf16 rounding boundary of a value as large as the sum of magnitudes."""
    B, npix, C, stride = 2, 37, 32, 50
    g = torch.Generator().manual_seed(12)
    hyper, up = torch.randn(B, C, generator=g).bfloat16(), torch.randn(B, npix, C, generator=g).bfloat16()
    out = Out(cuda, B, npix, torch.float32, ld=stride, pad_rows=1)
    ok(lib, lib.vstar_op_hyper_mask(None, dv(hyper), dv(up), P(out.full), stride, B, npix, C))
    got = out.get()
    ref, mag = R.hyper_mask(hyper, up)
    assert torch.equal(got, got.bfloat16().float())
    step_check("hyper_mask", f"B{B} npix{npix} C{C}", got, ref, 2.0 ** -8 * mag, "2^-8 sum|h||u|")
    assert lib.vstar_op_hyper_mask(None, dv(hyper), dv(up), P(out.full), stride, B, npix, 16) != 0


# ================================================================ quant.hip
def _quant_rows(rows, cols, ldx, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ldx), 1.0e4)                                       # the columns past `cols` would change every row's absmax
    x[:, :cols] = 2 * torch.randn(rows, cols, generator=g)
    x[0, :cols] = 0                                                          # all-zero row
    x[1, cols // 2] = 3.0e4                                                  # one huge outlier: the rest underflows towards zero
    x[2, :cols] = -0.75                                                      # a constant row
    return x.bfloat16()


@pytest.mark.parametrize("rows,cols", [(5, 8), (6, 72), (4, 2056)])
def test_quantize_rows_fp8(lib, cuda, dv, rows, cols):
    """scale EXACT vs fp32 absmax / 448 (1.0 for the zero row), bytes EXACT vs (x.float() * (1 / scale)).to(float8_e4m3fn);
    ldx > cols, ldq > cols, padding bytes untouched.  2056 columns: the second pass of the 2048-column stride, 8 columns long."""
    ldx, ldq = cols + 8, cols + 16
    x = _quant_rows(rows, cols, ldx, cols)
    q = Out(cuda, rows, cols, torch.uint8, ld=ldq, pad_rows=1, sentinel=0xAB)
    sc = Out(cuda, rows, 1, torch.float32)
    ok(lib, lib.vstar_op_quantize_rows_fp8(None, dv(x), ldx, P(q.full), ldq, P(sc.full), rows, cols))
    want_q, want_s = R.quantize_rows_fp8(x[:, :cols])
    assert want_s[0] == 1.0
    assert torch.equal(bits(sc.get()[:, 0]), bits(want_s))
    got_q = q.get()
    assert torch.equal(got_q, want_q), f"{(got_q != want_q).sum().item()} of {want_q.numel()} bytes differ"


@pytest.mark.parametrize("cols", [8, 72, 4096])
def test_rmsnorm_quant_fp8(lib, cuda, dv, cols):
    """The kernel's contract: the bytes and scales of vstar_op_quantize_rows_fp8 applied to vstar_op_rmsnorm's output on the same
    input — EXACT; and EXACT vs the CPU quantiser reference applied to that same 16-bit row.  The norm itself is gated against
    the CPU reference in test_rmsnorm_ex; end to end the dequantised row is within the norm's STEP gate plus half an e4m3 step
    (2^-4 relative for normals, scale * 2^-10 for subnormals) of the fp64 RMSNorm."""
    rows, eps = 5, 1e-6
    g = torch.Generator().manual_seed(cols)
    x = (0.3 + 2 * torch.randn(rows, cols, generator=g)).bfloat16()
    x[3] = 0                                                                 # a zero row: rstd = 1e3, output zero, scale 1
    gam = (1 + 0.1 * torch.randn(cols, generator=g)).bfloat16()
    xd, gd = x.to(cuda), gam.to(cuda)
    q = Out(cuda, rows, cols, torch.uint8, pad_rows=1, sentinel=0xAB)
    sc = Out(cuda, rows, 1, torch.float32)
    ok(lib, lib.vstar_op_rmsnorm_quant_fp8(None, P(xd), P(gd), P(q.full), P(sc.full), rows, cols, eps))
    y = torch.empty_like(xd)
    ok(lib, lib.vstar_op_rmsnorm(None, P(xd), P(gd), P(y), rows, cols, eps))
    q2 = torch.empty(rows, cols, dtype=torch.uint8, device=cuda)
    s2 = torch.empty(rows, dtype=torch.float32, device=cuda)
    ok(lib, lib.vstar_op_quantize_rows_fp8(None, P(y), cols, P(q2), cols, P(s2), rows, cols))
    got_q, got_s = q.get(), sc.get()[:, 0]
    assert torch.equal(got_q, q2.cpu()) and torch.equal(bits(got_s), bits(s2.cpu()))
    want_q, want_s = R.quantize_rows_fp8(y.cpu())
    assert torch.equal(got_q, want_q) and torch.equal(bits(got_s), bits(want_s))
    assert got_s[3] == 1.0 and (got_q[3] == 0).all()
    ref = R.rmsnorm_ex(x, gam, eps)
    deq = R.fp8_decode(got_q).double() * got_s.double()[:, None]
    lim = ref.abs() * (2 ** -7 + 2 ** -4) + 1e-2 + got_s.double()[:, None] * 2 ** -10
    assert ((deq - ref).abs() <= lim).all()


def test_rmsnorm_quant_fp8_refuses_rows_it_cannot_hold(lib, cuda, dv):
    x = torch.zeros(5, 4104, dtype=torch.bfloat16, device=cuda)
    q = torch.zeros(5, 4104, dtype=torch.uint8, device=cuda)
    s = torch.zeros(5, dtype=torch.float32, device=cuda)
    assert lib.vstar_op_rmsnorm_quant_fp8(None, P(x), P(x[0]), P(q), P(s), 5, 4104, 1e-6) != 0


# ================================================================ attention.hip: the SAM-head kernels
@pytest.mark.parametrize("B,Nq,Nk,H,D,kind", [
    (2, 7, 6, 8, 16, "plain"), (1, 5, 8, 2, 32, "plain"),                     # one thread per query, up to its 8-key boundary
    (1, 5, 9, 2, 32, "plain"),                                               # first size of the wave kernel
    (1, 3, 63, 2, 16, "plain"), (1, 3, 64, 2, 16, "plain"), (1, 3, 65, 2, 16, "plain"),
    (1, 5, 2304, 8, 16, "plain"), (1, 2, 2560, 2, 32, "plain"),              # 2560: every lane's 40 key slots in use
    (1, 3, 65, 2, 16, "spike"), (2, 7, 6, 8, 16, "spike"), (1, 3, 65, 2, 16, "low"),
])
def test_small_attention(lib, cuda, dv, B, Nq, Nk, H, D, kind):
    """STEP with atol = 2^-8 * max|V|: the probabilities are bf16 (sum ~ 1), so one flipped probability rounding or the __expf /
    fp32 summation error moves the output by at most a bf16 half step of a weight <= 1 times max|V|.  q and k are multiples of 1/8
    in [-2, 2]: every q.k is exact in fp32 AND fp64, so the bf16 scores of kernel and reference are the same numbers and the gate
    does not have to absorb a flipped score (one bf16 step of a score of 10 would be 6 % of a probability).  spike: q.k = 40 on
    the last key; low: every score ~ -300 (the running maximum must be subtracted)."""
    C = H * D
    g = torch.Generator().manual_seed(Nk * 3 + D)
    grid = lambda *s: (torch.randint(-16, 17, s, generator=g).float() / 8).bfloat16()     # noqa: E731
    q, k = grid(B, Nq, C), grid(B, Nk, C)
    v = torch.randn(B, Nk, C, generator=g).bfloat16()
    if kind == "spike":
        q[:], k[:, -1] = 1.25, 40.0 / (1.25 * D)
    elif kind == "low":
        q[:] = 10.0
        k = (-1200.0 / (10.0 * D) + torch.randint(-1, 2, (B, Nk, C), generator=g).float() / 8).bfloat16()
    out = Out(cuda, B * Nq, C, torch.bfloat16)
    ok(lib, lib.vstar_op_small_attention(None, dv(q), dv(k), dv(v), P(out.full), B, Nq, Nk, H, D))
    ref = R.small_attention(q, k, v, H).view(-1, C)
    step_check("small_attention", f"B{B} Nq{Nq} Nk{Nk} H{H} D{D} {kind}", out.get(), ref, 2.0 ** -8 * float(v.float().abs().max()),
               "2^-8 max|V|")


def test_small_attention_refuses_shapes_outside_its_domain(lib, cuda, dv):
    z = torch.zeros(2561 * 48, dtype=torch.bfloat16, device=cuda)
    assert lib.vstar_op_small_attention(None, P(z), P(z), P(z), P(z), 1, 1, 2561, 2, 16) != 0       # 41 keys per lane
    assert lib.vstar_op_small_attention(None, P(z), P(z), P(z), P(z), 1, 1, 9, 2, 24) != 0          # D = 24
