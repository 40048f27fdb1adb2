"""Fake-quant restatement of the ViT towers under VSMConfig.vit_w8a8: oracle/vsm_oracle.py::vit_tower with the four block
linears of every encoder block on per-token / per-output-channel e4m3 operands — the scheme of vstar_amd/csrc/engine_base.hpp::
run_tower_w8.  The reference has no fp8 path; this file is the parity target of tests/test_vit8_engine_gpu.py.

Per block, in the storage type dt of the state dict (bf16 in the tests; `.to(dt)` marks the engine's 16-bit rounding points):
  1. h8, sa = quant_rows(dt(LayerNorm1(x)))
  2. qkv   = dt((h8 . W8_qkv^T) * sa[m] * sw[n] + b)              W8 / sw = quant_rows over the rows of the UNFOLDED weight
  3. att   = attention(qkv), then quant_rows(att)
  4. x     = dt(dt(acc * sa * sw + b) + x)                          out_proj
  5. quant_rows(dt(LayerNorm2(x))); m = quick_gelu(dt(acc * sa * sw + b)) in dt arithmetic (the bf16 kernels' rounding points)
  6. quant_rows(m); x = dt(dt(acc * sa * sw + b) + x)               fc2
The bias is added in fp32 BEFORE the rounding (oracle.linear_w8a8 has no bias and rounds the product).  quant=False switches every
quantisation off and takes the oracle's own F.linear: the function then IS vit_tower, which tests/test_vit8_oracle.py checks."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle.vsm_oracle import _ln, fp8_fake_quant, quick_gelu


def lin8(sd, keys, x: torch.Tensor, quant: bool = True) -> torch.Tensor:
    """Linear over the concatenated rows of sd[k + '.weight'] (k in keys) with bias; quant: both operands fake-quantised per row."""
    if not quant:      # (one F.linear per key, as vit_tower calls them)
        return torch.cat([F.linear(x, sd[k + ".weight"], sd[k + ".bias"]) for k in keys], dim=-1)
    w = torch.cat([sd[k + ".weight"] for k in keys], dim=0)
    b = torch.cat([sd[k + ".bias"] for k in keys], dim=0)
    xq, sx = fp8_fake_quant(x)
    wq, sw = fp8_fake_quant(w)
    return ((xq @ wq.T) * sx * sw.transpose(-1, -2) + b.float()).to(x.dtype)


def vit_tower8(sd, prefix: str, preln: str, pix: torch.Tensor, heads: int, n_blocks: int, quant: bool = True) -> torch.Tensor:
    """Hidden state after `n_blocks` encoder blocks, [B, 1 + P, C]; patch embedding and pre-LayerNorm stay as in vit_tower."""
    w = sd[prefix + "embeddings.patch_embedding.weight"]
    ps = w.shape[-1]
    x = F.conv2d(pix.to(w.dtype), w, None, stride=ps).flatten(2).transpose(1, 2)
    cls = sd[prefix + "embeddings.class_embedding"].expand(x.shape[0], 1, -1)
    x = torch.cat([cls, x], dim=1) + sd[prefix + "embeddings.position_embedding.weight"].unsqueeze(0)
    x = _ln(sd, prefix + preln, x)
    B, N, C = x.shape
    hd = C // heads
    for i in range(n_blocks):
        lp = f"{prefix}encoder.layers.{i}."
        h = _ln(sd, lp + "layer_norm1", x)
        qkv = lin8(sd, [lp + "self_attn.q_proj", lp + "self_attn.k_proj", lp + "self_attn.v_proj"], h, quant)
        q, k, v = qkv.split(C, dim=-1)
        q = q * (hd ** -0.5)
        q, k, v = (t.view(B, N, heads, hd).transpose(1, 2) for t in (q, k, v))
        att = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v
        att = att.transpose(1, 2).reshape(B, N, C)
        x = x + lin8(sd, [lp + "self_attn.out_proj"], att, quant)
        h = _ln(sd, lp + "layer_norm2", x)
        x = x + lin8(sd, [lp + "mlp.fc2"], quick_gelu(lin8(sd, [lp + "mlp.fc1"], h, quant)), quant)
    return x


def clip_features8(sd, cfg, pix: torch.Tensor, quant: bool = True) -> torch.Tensor:
    """oracle.clip_features under vit_w8a8: [B, P, C]."""
    n_blocks = cfg.clip_layers + 1 + cfg.clip_select_layer
    return vit_tower8(sd, "clip.vision_model.", "pre_layrnorm", pix, cfg.clip_heads, n_blocks, quant)[:, 1:]


def owl_feats8(sd, cfg, pix: torch.Tensor, quant: bool = True) -> torch.Tensor:
    """oracle.owl_visual_embs under vit_w8a8 (post-LayerNorm, class-token product and layer_norm stay bf16): [B, g, g, C]."""
    pre = "model.owlvit.vision_model."
    x = vit_tower8(sd, pre, "pre_layernorm", pix, cfg.owl_heads, cfg.owl_layers, quant)
    x = _ln(sd, pre + "post_layernorm", x)
    x = x[:, 1:, :] * x[:, :1, :]
    x = _ln(sd, "model.owlvit.layer_norm", x)
    g = int(math.isqrt(x.shape[1]))
    return x.reshape(x.shape[0], g, g, x.shape[-1])
