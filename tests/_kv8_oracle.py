"""Oracle of the block-scaled fp8 KV cache: the row round trip is oracle.vsm_oracle.mx_fake_quant on rows of 128
(4 blocks of 32 head-dim elements, one E8M0 byte each, OCP e4m3 codes), and the chain oracle is oracle.vqa_oracle.llama_forward with
K (after RoPE) and V round-tripped through fp16 before they are used or cached — the row's own key and value included."""
import math
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle.vqa_oracle import Past, rms_norm, rope_tables, rotate_half
from oracle.vsm_oracle import mx_fake_quant

LIMIT = 63488.0      # from here up the top grid point decodes to 65536 (+inf in fp16): outside the bit-for-bit claims


def kv8_round_trip(x: torch.Tensor) -> torch.Tensor:
    """Rows [..., 128] of any float dtype -> the values the cache holds for them: decode(quantise(fp16(x))), as fp32."""
    assert x.shape[-1] == 128
    return mx_fake_quant(x.to(torch.float16))[0]


def kv8_quantize(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """fp16 rows [rows, 128] -> (e4m3 code bytes uint8 [rows, 128], E8M0 bytes uint8 [rows, 4], xhat fp16 [rows, 128])."""
    t = torch.from_numpy(np.ascontiguousarray(x)).view(torch.float16)
    dec, e = mx_fake_quant(t)
    scale = torch.ldexp(torch.ones(e.shape), e.to(torch.int32) - 127).repeat_interleave(32, dim=-1)
    safe = torch.where(scale > 0, scale, torch.ones_like(scale))            # all-zero block: e = 0, codes 0
    codes = (dec / safe).to(torch.float8_e4m3fn).view(torch.uint8)          # exact: dec = code x scale
    return codes.numpy(), e.numpy(), dec.to(torch.float16).numpy()


def llama_forward_kv8(sd, cfg, x: torch.Tensor, past: Optional[Past] = None):
    """oracle.vqa_oracle.llama_forward, K (after RoPE) and V of the new rows round-tripped through the fp8 row format before they
    are used or cached.  x: inputs_embeds [T, H] (one sequence).  Returns (logits [T, vocab], new past)."""
    T, H = x.shape
    heads, hd = cfg.llm_heads, H // cfg.llm_heads
    P0 = 0 if past is None else past[0][0].shape[1]
    cos, sin = rope_tables(P0 + T, hd, cfg.llm_rope_theta, x.dtype)
    cos, sin = cos[P0:], sin[P0:]
    mask = torch.full((T, P0 + T), float("-inf")).triu(P0 + 1)
    new_past: Past = []
    for i in range(cfg.llm_layers):
        lp = f"model.layers.{i}."
        h = rms_norm(x, sd[lp + "input_layernorm.weight"], cfg.llm_rms_eps)
        q = F.linear(h, sd[lp + "self_attn.q_proj.weight"]).view(T, heads, hd).transpose(0, 1)
        k = F.linear(h, sd[lp + "self_attn.k_proj.weight"]).view(T, heads, hd).transpose(0, 1)
        v = F.linear(h, sd[lp + "self_attn.v_proj.weight"]).view(T, heads, hd).transpose(0, 1)
        q = q * cos + rotate_half(q) * sin
        k = k * cos + rotate_half(k) * sin
        k = kv8_round_trip(k).to(x.dtype)
        v = kv8_round_trip(v).to(x.dtype)
        if past is not None:
            k = torch.cat([past[i][0], k], dim=1)
            v = torch.cat([past[i][1], v], dim=1)
        new_past.append((k, v))
        w = (q @ k.transpose(-1, -2)) / math.sqrt(hd) + mask.to(q.dtype)
        w = torch.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
        att = (w @ v).transpose(0, 1).reshape(T, H)
        x = x + F.linear(att, sd[lp + "self_attn.o_proj.weight"])
        h = rms_norm(x, sd[lp + "post_attention_layernorm.weight"], cfg.llm_rms_eps)
        x = x + F.linear(F.silu(F.linear(h, sd[lp + "mlp.gate_proj.weight"])) * F.linear(h, sd[lp + "mlp.up_proj.weight"]),
                         sd[lp + "mlp.down_proj.weight"])
    x = rms_norm(x, sd["model.norm.weight"], cfg.llm_rms_eps)
    return F.linear(x, sd["lm_head.weight"]), new_past


def rel_l2(got, ref) -> float:
    g = np.asarray(got, np.float64).ravel()
    r = np.asarray(ref, np.float64).ravel()
    return float(np.linalg.norm(g - r) / max(np.linalg.norm(r), 1e-30))
