"""tests/_small_ops_ref.py against independent torch formulations, so that a wrong reference cannot bless a wrong kernel.
Runs without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _small_ops_ref as R


def _randbf(g, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=g)).bfloat16()


@pytest.mark.parametrize("B,h,w,C", [(1, 1, 1, 8), (2, 3, 5, 8), (1, 6, 6, 32)])
def test_upsample2x_im2col3x3_is_interpolate_then_unfold(B, h, w, C):
    g = torch.Generator().manual_seed(h * 10 + w)
    src = _randbf(g, B, h, w, C)                                             # channels-last
    up = F.interpolate(src.permute(0, 3, 1, 2).float(), scale_factor=2, mode="bilinear").bfloat16()     # [B, C, 2h, 2w]
    cols = F.unfold(up.float(), 3, padding=1)                                # [B, C * 9, L], channel-major: c * 9 + ky * 3 + kx
    want = cols.view(B, C, 9, 4 * h * w).permute(0, 3, 2, 1).reshape(B * 4 * h * w, 9 * C).bfloat16()
    got = R.upsample2x_im2col3x3(src)
    # random bf16 inputs: the fp64 blend rounds once, torch's fp32 blend twice — one bf16 step at most, and only rarely
    diff = (got.float() - want.float()).abs()
    assert (diff <= want.float().abs() * 2 ** -7).all()
    assert (diff != 0).float().mean() < 1e-2
    assert torch.equal(got == 0, want == 0)                                  # the zero padding sits at the same taps


def test_upsample2x_is_bit_exact_on_exactly_representable_inputs():
    # multiples of 1/8 below 32: every blend (weights 1, 3, 9 sixteenths) is exact in fp32 and fp64, so the ONLY rounding is the
    # final one to bf16 and torch's fp32 interpolate must agree bit for bit
    g = torch.Generator().manual_seed(3)
    src = (torch.randint(-255, 256, (2, 3, 5, 8), generator=g).float() / 8).bfloat16()
    up = F.interpolate(src.permute(0, 3, 1, 2).float(), scale_factor=2, mode="bilinear").bfloat16().permute(0, 2, 3, 1)
    assert torch.equal(R.upsample2x(src).view(torch.int16), up.contiguous().view(torch.int16))


@pytest.mark.parametrize("B,I,ps,kpad", [(2, 28, 14, 640), (1, 32, 16, 768), (3, 28, 14, 588)])
def test_im2col_patch_is_unfold(B, I, ps, kpad):
    g = torch.Generator().manual_seed(I)
    pix = _randbf(g, B, 3, I, I)
    want = F.unfold(pix.float(), ps, stride=ps).transpose(1, 2).reshape(-1, 3 * ps * ps).bfloat16()
    got = R.im2col_patch(pix, ps, kpad)
    assert torch.equal(got[:, : 3 * ps * ps], want)
    assert (got[:, 3 * ps * ps:] == 0).all()
    # ... and a conv through it equals Conv2d(kernel = stride = ps)
    w = torch.randn(5, 3, ps, ps, generator=g)
    conv = F.conv2d(pix.float(), w, stride=ps).flatten(2).transpose(1, 2).reshape(-1, 5)
    assert torch.allclose(got[:, : 3 * ps * ps].float() @ w.view(5, -1).T, conv, atol=1e-3)


@pytest.mark.parametrize("act,use_beta", [(0, True), (1, True), (1, False)])
def test_layernorm_ex_is_layer_norm_then_gelu(act, use_beta):
    g = torch.Generator().manual_seed(act)
    x = _randbf(g, 9, 72) + 50
    gam, bet = _randbf(g, 72), (_randbf(g, 72) if use_beta else None)
    idx = torch.tensor([8, 0, 0, 3, 7], dtype=torch.int32)
    want = F.layer_norm(x.double()[idx.long()], (72,), gam.double(), None if bet is None else bet.double(), 1e-6)
    if act:
        want = F.gelu(want.float().bfloat16().double())
    got = R.layernorm_ex(x, gam, bet, 1e-6, idx, act)
    assert torch.allclose(got, want, rtol=1e-9, atol=1e-9)


def test_rmsnorm_ex_is_llama_rmsnorm():
    g = torch.Generator().manual_seed(1)
    x, gam = _randbf(g, 7, 72, scale=3.0), _randbf(g, 72)
    idx = torch.tensor([6, 6, 1], dtype=torch.int32)
    xs = x.double()[idx.long()]
    want = gam.double() * (xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + 1e-6)).float().bfloat16().double()
    assert torch.allclose(R.rmsnorm_ex(x, gam, 1e-6, idx), want, rtol=1e-12, atol=0)
    # the fp32 form rounds to the same stored row except where the fp32 statistics flip a rounding
    stored = R.rmsnorm_bf16(x[idx.long()], gam, 1e-6).double()
    assert ((stored - want).abs() <= want.abs() * 2 ** -7).all()


def test_ln_rstd_and_partials():
    g = torch.Generator().manual_seed(2)
    x = _randbf(g, 5, 256) + 3
    xd = x.double()
    want = F.layer_norm(xd, (256,), eps=1e-5)[:, 0] / (xd[:, 0] - xd.mean(-1))          # LayerNorm's own 1 / sqrt(var + eps)
    assert torch.allclose(R.ln_rstd(x, 1e-5), want, rtol=1e-9, atol=0)
    part = R.ln_partials(x, 11)
    assert torch.isnan(part[:, 8:]).all()
    assert torch.allclose(part[:, :4].sum(-1).double(), x.double().pow(2).sum(-1), rtol=1e-6)
    assert torch.allclose(part[:, 4:8].sum(-1).double(), x.double().sum(-1), rtol=1e-6)


@pytest.mark.parametrize("B,Nq,Nk,H,D", [(2, 7, 6, 8, 16), (1, 5, 9, 2, 32), (1, 3, 65, 2, 16)])
def test_small_attention_is_sdpa_within_bf16_noise(B, Nq, Nk, H, D):
    g = torch.Generator().manual_seed(Nk)
    q, k, v = _randbf(g, B, Nq, H * D), _randbf(g, B, Nk, H * D), _randbf(g, B, Nk, H * D)
    sp = lambda t: t.double().view(B, -1, H, D).transpose(1, 2)              # noqa: E731
    want = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(B, Nq, H * D)
    got = R.small_attention(q, k, v, H)
    smax = float((sp(q) @ sp(k).transpose(-1, -2)).abs().max()) / math.sqrt(D)
    # two half-step roundings of every score (2^-9 relative each) move a probability by <= 2 * 2^-8 * smax relative (numerator and
    # normaliser); its own rounding adds 2^-9
    bound = (2 * 2 ** -8 * smax + 2 ** -9) * float(v.float().abs().max())
    assert float((got - want).abs().max()) <= bound
    assert float((got - want).abs().max()) > 0                               # the rounding points are really there


def test_box_bias_is_hf_compute_box_bias():
    import numpy as np
    for n in (1, 5, 24):
        # transformers OwlViTForObjectDetection.normalize_grid_corner_coordinates + compute_box_bias, restated literally
        box_coordinates = np.stack(np.meshgrid(np.arange(1, n + 1), np.arange(1, n + 1)), axis=-1).astype(np.float32)
        box_coordinates /= np.array([n, n], np.float32)
        box_coordinates = box_coordinates.reshape(n * n, 2)
        box_coordinates = torch.from_numpy(box_coordinates)
        box_coordinates = torch.clip(box_coordinates, 0.0, 1.0)
        box_coord_bias = torch.log(box_coordinates + 1e-4) - torch.log1p(-box_coordinates + 1e-4)
        box_size = torch.full_like(box_coord_bias, 1.0 / n)
        box_size_bias = torch.log(box_size + 1e-4) - torch.log1p(-box_size + 1e-4)
        want = torch.cat([box_coord_bias, box_size_bias], dim=-1)
        got = R.box_bias(n)
        assert got.shape == (n * n, 4)
        assert torch.allclose(got.float(), want, rtol=2e-5, atol=2e-5)       # HF evaluates it in fp32
        assert got[n - 1, 0] == got[-1, 1] == math.log(1.0001) - math.log1p(-1 + 1e-4)      # the coord = 1 edge


def test_owl_box_finish_shapes_and_sigmoid():
    g = torch.Generator().manual_seed(4)
    raw = 6 * (2 * torch.rand(25, 8, generator=g) - 1)
    box, v = R.owl_box_finish(raw, 5, 2, img_div=2)
    assert box.shape == (2, 25, 4) and torch.equal(box[0], box[1])
    want = torch.sigmoid((raw[:, :4].bfloat16().double() + R.box_bias(5)).float().bfloat16().double())
    assert torch.equal(box[0], want)


def test_owl_class_logits_is_the_hf_head_in_bf16():
    # the HF module's forward on bf16 tensors, op by op (every torch op on bf16 rounds its result to bf16)
    g = torch.Generator().manual_seed(6)
    Q, rows = 64, 5
    emb = torch.randn(2 * rows, Q + 6, generator=g)
    emb[:, Q] = torch.rand(2 * rows, generator=g) * 2 - 1
    emb[:, Q + 1] = torch.randn(2 * rows, generator=g) * 2
    query = _randbf(g, 6, Q)
    got, mult = R.owl_class_logits(emb, Q, query, rows, img_div=3)
    e = emb[:, :Q].bfloat16().view(2, rows, Q).repeat_interleave(3, 0)
    e = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
    qn = query / (torch.linalg.norm(query, dim=-1, keepdim=True) + 1e-6)
    logits = torch.einsum("bpd,bd->bp", e, qn)
    shift = emb[:, Q].bfloat16().view(2, rows).repeat_interleave(3, 0)
    scale = F.elu(emb[:, Q + 1].bfloat16().view(2, rows).repeat_interleave(3, 0)) + 1
    want = (logits + shift) * scale
    assert torch.equal(mult.float().bfloat16(), scale)
    # torch's bf16 norm / einsum accumulate in fp32 in their own order: one flipped bf16 rounding of the normalised dot product
    err = (got.float().bfloat16().float() - want.float()).abs()
    assert (err <= 2 ** -7 * want.float().abs() + 2 ** -7 * scale.float()).all()
    assert (err == 0).float().mean() > 0.5


def test_quantize_rows_fp8_round_trip_properties():
    g = torch.Generator().manual_seed(8)
    x = _randbf(g, 7, 72, scale=2.0)
    x[2] = 0
    x[3, 5] = 3.0e4                                                          # one huge outlier
    x[4] = -0.75                                                             # a constant row
    q, scale = R.quantize_rows_fp8(x)
    assert q.dtype == torch.uint8 and scale.dtype == torch.float32
    dec = R.fp8_decode(q).double()
    assert torch.isfinite(dec).all()
    p = x.double() / scale.double()[:, None]
    assert ((dec - p).abs() * scale.double()[:, None] <= scale.double()[:, None] * R.fp8_step(p) / 2 * (1 + 1e-6)).all()
    amax = x.float().abs().amax(-1)
    for r in range(7):
        if amax[r] == 0:
            continue
        at = x[r].float().abs() == amax[r]
        assert (dec[r][at].abs() == 448).all()
        assert torch.equal(torch.sign(dec[r][at]), torch.sign(x[r][at].double()))
    assert scale[2] == 1.0 and (q[2] == 0).all()
    assert (dec[4] == -448).all() and scale[4] == torch.tensor(0.75) / 448


def test_layout_references_against_loops():
    g = torch.Generator().manual_seed(9)
    # vit_assemble_tokens
    patch, cls, pos = _randbf(g, 3, 4, 8), _randbf(g, 8), _randbf(g, 5, 8)
    tok = R.vit_assemble_tokens(patch, cls, pos)
    for b in range(3):
        assert torch.equal(tok[b, 0], (cls.float() + pos[0].float()).bfloat16())
        for p in range(4):
            assert torch.equal(tok[b, 1 + p], (patch[b, p].float() + pos[1 + p].float()).bfloat16())
    # llm_embed_text (prepare_inputs_labels_for_multimodal: the placeholder column is replaced by P image rows)
    table = _randbf(g, 50, 8)
    for img_col in (0, 3, 8):
        ids = torch.randint(0, 50, (2, 9), generator=g, dtype=torch.int32)
        ids[:, img_col] = -200
        ids[0, (img_col + 2) % 9], ids[1, (img_col + 4) % 9] = -7, 50
        x0 = torch.full((2, 12, 8), 123.0).bfloat16()
        out = R.llm_embed_text(ids, img_col, 4, table, x0)
        for b in range(2):
            seq = [table[min(max(int(i), 0), 49)] for i in ids[b, :img_col]] + [x0[b, 0]] * 4 + \
                  [table[min(max(int(i), 0), 49)] for i in ids[b, img_col + 1:]]
            assert torch.equal(out[b], torch.stack(seq))
    # add_bcast / add_bcast_repeat / bcast_rows / owl_cls_mul / gather_rows
    a, b5 = _randbf(g, 10, 8), _randbf(g, 5, 8)
    out = R.add_bcast(a, b5)
    assert all(torch.equal(out[r], (a[r].float() + b5[r % 5].float()).bfloat16()) for r in range(10))
    out = R.add_bcast_repeat(a, b5, 5, 3, 5)                                 # 2 blocks of 5 rows, 5 of the 6 repeats
    assert all(torch.equal(out[n * 5 + p], (a[(n // 3) * 5 + p].float() + b5[0].float()).bfloat16()) for n in range(5) for p in range(5))
    dst = torch.full((9, 16), 123.0).bfloat16()
    src = _randbf(g, 2, 16)
    out = R.bcast_rows(src, dst, 2, 4, 2, 8)
    for r in range(9):
        for c in range(16):
            want = src[r % 4, c] if (r < 8 and r % 4 < 2 and c < 8) else dst[r, c]
            assert out[r, c] == want
    x = _randbf(g, 2, 4, 8)
    out = R.owl_cls_mul(x)
    assert all(torch.equal(out[b, p], (x[b, 1 + p].float() * x[b, 0].float()).bfloat16()) for b in range(2) for p in range(3))
    idx = torch.tensor([3, 3, 0, 2, 1, 0], dtype=torch.int32)
    assert all(torch.equal(R.gather_rows(a, idx)[r], a[int(idx[r])]) for r in range(6))


def test_argmax_reference_rule():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, 5.0, 5.0, 2.0], [-inf, -inf, -inf, -inf], [0.0, nan, 9.0, nan], [nan, nan, nan, nan], [1.0, inf, inf, 3.0]])
    assert R.argmax_rows(x).tolist() == [1, 0, 1, 0, 1]
