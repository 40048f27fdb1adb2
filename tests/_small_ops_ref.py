"""Plain CPU references of the small HIP kernels (heads.hip, elementwise.hip, norm.hip, quant.hip, the SAM-head attention).

One function per kernel, written from the kernel's stated contract (kernels.hpp, include/vstar_hip.h) and the HF / torch
definition it replaces — not from the kernel's loops.  Arithmetic is float64 unless the contract is "fp32 like torch" (single
adds / multiplies, the fp8 row scale), where float32 is what makes the result bit-defined.  The documented storage-type rounding
points are applied through `rbf` (float -> bfloat16 -> float64).  References of kernels gated by a tolerance return the value
BEFORE the final store rounding; the bit-exact ones return the stored dtype.

tests/test_small_ops_ref.py pins each of these to an independent torch formulation; tests/test_small_ops_gpu.py holds the
kernels to them on the MI355X.
"""
import math

import torch

FP8_MAX = 448.0


def rbf(t):
    """Round through bf16 storage (nearest even, via float32 like every producer on the path); float64 out."""
    return t.float().bfloat16().double()


# ---------------------------------------------------------------- layout kernels (bit-exact)
def im2col_patch(pix, ps, kpad):
    """pix [B, 3, I, I] -> [B * G * G, kpad]: row = (b, py, px), column k = c * ps * ps + ky * ps + kx, zero padded."""
    B, _, I, _ = pix.shape
    G = I // ps
    a = pix.reshape(B, 3, G, ps, G, ps).permute(0, 2, 4, 1, 3, 5).reshape(B * G * G, 3 * ps * ps)
    out = torch.zeros(B * G * G, kpad, dtype=pix.dtype)
    out[:, : 3 * ps * ps] = a
    return out


def vit_assemble_tokens(patch, cls, pos):
    """cat([class_embedding, patch_embeds], 1) + position_embedding: patch [B, P, C], cls [C], pos [P + 1, C] -> [B, P + 1, C]."""
    B = patch.shape[0]
    seq = torch.cat([cls.view(1, 1, -1).expand(B, 1, -1), patch], 1)
    return (seq.float() + pos.float()[None]).bfloat16()


def llm_embed_text(ids, img_col, P, table, x):
    """The text rows of the spliced sequence: ids [B, L] with the image placeholder at column img_col, x [B, L - 1 + P, C] (a copy
    is returned; the P image rows keep what x held).  Ids are clamped to [0, vocab)."""
    B, L = ids.shape
    out = x.clone()
    keep = [c for c in range(L) if c != img_col]
    text = table[ids[:, keep].clamp(0, table.shape[0] - 1).long()]          # [B, L - 1, C]
    out[:, :img_col] = text[:, :img_col]
    out[:, img_col + P:] = text[:, img_col:]
    return out


def add_bcast(a, b):
    """out[r] = a[r] + b[r % b_rows]."""
    idx = torch.arange(a.shape[0]) % b.shape[0]
    return (a.float() + b.float()[idx]).bfloat16()


def add_bcast_repeat(a, b, n_out, rep, rows_per):
    """Every block of rows_per rows of `a` repeated rep times, + b[0]: out [n_out * rows_per, cols]."""
    blocks = a.view(-1, rows_per, a.shape[-1]).repeat_interleave(rep, 0)[:n_out]
    return (blocks.float() + b.float().reshape(-1, a.shape[-1])[0].view(1, 1, -1)).bfloat16().reshape(n_out * rows_per, -1)


def bcast_rows(src, dst, nrep, rep_stride, nrows, cols):
    """dst viewed as rows of ld elements: rows r * rep_stride + i (i < nrows) receive columns [0, cols) of src row i."""
    out = dst.clone()
    for r in range(nrep):
        out[r * rep_stride: r * rep_stride + nrows, :cols] = src[:nrows, :cols]
    return out


def owl_cls_mul(x):
    """image_embeds[:, 1:, :] * image_embeds[:, :1, :]."""
    return (x[:, 1:].float() * x[:, :1].float()).bfloat16()


def gather_rows(x, idx):
    return x[idx.long()]


def argmax_rows(x):
    """First column of the maximum per row; NaN ranks above every number (torch.argmax)."""
    return torch.argmax(x, dim=-1).to(torch.int32)


def scale_cols(W, w):
    return (W.float() * w.float()[None]).bfloat16()


def fill(n, value):
    return torch.full((n,), value, dtype=torch.float32).bfloat16()


# ---------------------------------------------------------------- norms
def rf16(t):
    """Round through fp16 storage (nearest even, ONE rounding from float64: numpy's conversion); float64 out."""
    return torch.from_numpy(t.double().numpy().astype("float16")).double()


def layernorm_ex(x, gamma, beta, eps, row_index=None, act=0, rnd=rbf):
    """nn.LayerNorm over the last dim of x[row_index] (biased variance); act 1: exact-erf GELU of the bf16-rounded affine result
    (LayerNorm2d + GELU of the mask head).  float64, before the store rounding.  rnd: the storage type's rounding (rbf: the bf16
    build, rf16: the fp16 build of the same kernel)."""
    xs = x.double() if row_index is None else x.double()[row_index.long()]
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    y = (xs - mean) / torch.sqrt(var + eps) * gamma.double()
    if beta is not None:
        y = y + beta.double()
    if act == 1:
        t = rnd(y)
        y = 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
    return y


def rmsnorm_ex(x, gamma, eps, row_index=None, rnd=rbf):
    """LlamaRMSNorm: weight * (x * rsqrt(mean(x^2) + eps)).to(bf16).  float64, before the store rounding.  rnd as in layernorm_ex."""
    xs = x.double() if row_index is None else x.double()[row_index.long()]
    return gamma.double() * rnd(xs / torch.sqrt((xs ** 2).mean(-1, keepdim=True) + eps))


def ln_rstd(x, eps):
    xs = x.double()
    return 1.0 / torch.sqrt(xs.var(-1, unbiased=False) + eps)


def ln_partials(x, ld):
    """What a GEMM epilogue leaves for ln_rstd_partials: per row the sums of squares of the 64-column spans, then their sums; fp32."""
    rows, cols = x.shape
    n = cols // 64
    spans = x.float().view(rows, n, 64)
    out = torch.full((rows, ld), float("nan"), dtype=torch.float32)
    out[:, :n] = (spans * spans).sum(-1)
    out[:, n: 2 * n] = spans.sum(-1)
    return out


# ---------------------------------------------------------------- fp8 rows
def quantize_rows_fp8(x):
    """Per-row symmetric OCP e4m3: scale = absmax / 448 in fp32 (1 for an all-zero row), bytes = e4m3(x * (1 / scale)) with the
    product in fp32 — the model test_gemm_w8a8_fp8 uses.  Returns (bytes uint8 [rows, cols], scale fp32 [rows])."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    scale = torch.where(amax > 0, amax / torch.tensor(FP8_MAX, dtype=torch.float32), torch.ones_like(amax))
    inv = 1.0 / scale
    q = (xf * inv[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def fp8_decode(q):
    return q.view(torch.float8_e4m3fn).float()


def fp8_step(v):
    """Spacing of e4m3 at |v| (3 mantissa bits, smallest normal 2^-6, subnormal spacing 2^-9)."""
    e = torch.floor(torch.log2(v.double().abs().clamp_min(2.0 ** -6)))
    return 2.0 ** (e - 3)


def rmsnorm_bf16(x, gamma, eps):
    """The 16-bit row LlamaRMSNorm stores (fp32 statistics like torch)."""
    xf = x.float()
    y = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).bfloat16().float()
    return (gamma.float() * y).bfloat16()


def rmsnorm_quant_fp8(x, gamma, eps):
    return quantize_rows_fp8(rmsnorm_bf16(x, gamma, eps))


# ---------------------------------------------------------------- OWL-ViT heads
def owl_class_logits(emb, Q, query, rows_per_crop, img_div=1):
    """HF OwlViTClassPredictionHead with one query per record, in the bf16 model's arithmetic: every tensor op rounds its result
    to bf16 (norm, + 1e-6, divide, the dot product, + shift, elu, + 1, the product).  emb [crops * rows_per_crop, >= Q + 2] fp32 =
    dense0 | shift | scale; query [B, Q]; record b reads crop b // img_div.  Returns (logits [B, rows_per_crop] float64 BEFORE the
    final rounding, multiplier elu(scale) + 1 [B, rows_per_crop])."""
    B = query.shape[0]
    crop = torch.arange(B) // img_div
    e_all = emb.view(-1, rows_per_crop, emb.shape[-1])[crop]                 # [B, rows, ld]
    e = rbf(e_all[..., :Q])
    q = query.double()[:, None, :]
    en = rbf(rbf(e.pow(2).sum(-1, keepdim=True).sqrt()) + 1e-6)
    qn = rbf(rbf(q.pow(2).sum(-1, keepdim=True).sqrt()) + 1e-6)
    dot = rbf((rbf(e / en) * rbf(q / qn)).sum(-1))
    shift = rbf(e_all[..., Q])
    sc = rbf(e_all[..., Q + 1])
    elu = torch.where(sc > 0, sc, torch.expm1(sc))
    mult = rbf(rbf(elu) + 1.0)
    return rbf(dot + shift) * mult, mult


def box_bias(grid):
    """HF OwlViTForObjectDetection.compute_box_bias, [grid * grid, 4] float64."""
    ar = torch.arange(1, grid + 1, dtype=torch.float64)
    yy, xx = torch.meshgrid(ar, ar, indexing="ij")
    coords = (torch.stack([xx, yy], -1) / grid).reshape(-1, 2).clamp(0.0, 1.0)
    coord_bias = torch.log(coords + 1e-4) - torch.log1p(-coords + 1e-4)
    size = torch.full_like(coord_bias, 1.0 / grid)
    size_bias = torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)
    return torch.cat([coord_bias, size_bias], -1)


def owl_box_finish(raw, grid, B, img_div=1):
    """sigmoid(box_head(x).to(bf16) + box_bias) of record b on crop b // img_div: raw [crops * grid^2, >= 4] fp32.  Returns
    (boxes [B, grid^2, 4] float64 before the output rounding, the bf16 pre-sigmoid value v)."""
    crop = torch.arange(B) // img_div
    r = raw.view(-1, grid * grid, raw.shape[-1])[crop][..., :4]
    v = rbf(rbf(r) + box_bias(grid)[None])
    return torch.sigmoid(v), v


# ---------------------------------------------------------------- mask head
def _up2x_axis(x, dim):
    """Bilinear x2 along `dim`, align_corners=False: out[2i] = x[i-1]/4 + 3 x[i]/4, out[2i+1] = 3 x[i]/4 + x[i+1]/4, edges clamped."""
    n = x.shape[dim]
    i = torch.arange(n)
    prev, nxt = x.index_select(dim, (i - 1).clamp_min(0)), x.index_select(dim, (i + 1).clamp_max(n - 1))
    even, odd = 0.25 * prev + 0.75 * x, 0.75 * x + 0.25 * nxt
    shape = list(x.shape)
    shape[dim] = 2 * n
    return torch.stack([even, odd], dim + 1).reshape(shape)


def upsample2x(src):
    """src [B, h, w, C] -> bf16 [B, 2h, 2w, C]: F.interpolate(x.float(), scale_factor=2, mode="bilinear").to(bf16)."""
    return _up2x_axis(_up2x_axis(src.double(), 1), 2).float().bfloat16()


def upsample2x_im2col3x3(src):
    """... followed by the im2col of a 3x3 / pad 1 convolution: [B * 2h * 2w, 9 C], k = (ky * 3 + kx) * C + c."""
    up = upsample2x(src)
    B, H2, W2, C = up.shape
    pad = torch.zeros(B, H2 + 2, W2 + 2, C, dtype=up.dtype)
    pad[:, 1:-1, 1:-1] = up
    taps = [pad[:, ky: ky + H2, kx: kx + W2] for ky in range(3) for kx in range(3)]
    return torch.stack(taps, 3).reshape(B * H2 * W2, 9 * C)


def hyper_mask(hyper, up):
    """hyper [B, C], up [B, npix, C] -> (masks [B, npix] float64 before the bf16 rounding, sum_c |h| |u| for the gate)."""
    h, u = hyper.double()[:, None, :], up.double()
    return (h * u).sum(-1), (h.abs() * u.abs()).sum(-1)


# ---------------------------------------------------------------- SAM-head attention
def small_attention(q, k, v, H):
    """q [B, Nq, H * D], k / v [B, Nk, H * D] -> [B, Nq, H * D] float64 before the store rounding.  The bf16 model's rounding
    points: q k^T is a bf16 matmul, the division by sqrt(D) a bf16 op (fp32 multiply by 1 / sqrt(D)), softmax returns bf16."""
    B, Nq, C = q.shape
    D = C // H
    split = lambda t: t.double().view(B, -1, H, D).transpose(1, 2)            # noqa: E731  [B, H, N, D]
    qh, kh, vh = split(q), split(k), split(v)
    s = rbf(qh @ kh.transpose(-1, -2))
    s = (s.float() * (1.0 / torch.tensor(float(D), dtype=torch.float32).sqrt())).bfloat16().double()
    p = rbf(torch.softmax(s, -1))
    return (p @ vh).transpose(1, 2).reshape(B, Nq, C)
