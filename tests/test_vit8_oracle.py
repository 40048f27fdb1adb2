"""CPU checks of the vit_w8a8 parity target (tests/_vit8_oracle.py) and of the config field's place in the ABI.

The fake-quant towers must (a) BE oracle.vit_tower when the quantisation is switched off — the restatement adds nothing else — and
(b) sit a quantisation's distance from the plain towers: more than 1e-4 (the quantisation does something) and less than 0.15 (it costs
a few percent; measured 4.1e-2 - 4.2e-2 at two blocks for both towers, with the bf16 towers 5e-3 from the fp32 ones)."""
import ctypes

import numpy as np
import pytest
import torch

from _vit8_oracle import vit_tower8
from oracle import vsm_oracle
from vstar_amd.config import CVstarConfig, VSMConfig
from vstar_amd.weights import random_state_dict

NARROW = dict(clip_hidden=256, clip_heads=4, clip_mlp=1024, owl_hidden=256, owl_heads=4, owl_mlp=512)
REAL = dict(clip_hidden=1024, clip_heads=16, clip_mlp=4096, owl_hidden=768, owl_heads=12, owl_mlp=3072)
TOWERS = {"clip": ("clip.vision_model.", "pre_layrnorm", 224), "owl": ("model.owlvit.vision_model.", "pre_layernorm", 768)}


def rel_l2(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / ref.norm())


def _tower_args(cfg, which):
    prefix, preln, px = TOWERS[which]
    heads = cfg.clip_heads if which == "clip" else cfg.owl_heads
    blocks = cfg.clip_blocks if which == "clip" else cfg.owl_layers
    pix = torch.randn(1, 3, px, px, generator=torch.Generator().manual_seed(5)).bfloat16()
    return prefix, preln, pix, heads, blocks


@pytest.fixture(scope="module", params=["narrow", "real"])
def model(request):
    cfg = VSMConfig.tiny(**(NARROW if request.param == "narrow" else REAL))
    return cfg, random_state_dict(cfg, seed=0, dtype=torch.bfloat16)


@pytest.mark.parametrize("which", ["clip", "owl"])
def test_vit8_oracle_is_vit_tower_without_quantisation(model, which):
    cfg, sd = model
    args = _tower_args(cfg, which)
    assert torch.equal(vit_tower8(sd, *args, quant=False), vsm_oracle.vit_tower(sd, *args))


@pytest.mark.parametrize("which", ["clip", "owl"])
def test_vit8_oracle_sits_a_quantisation_away_from_the_plain_tower(model, which):
    cfg, sd = model
    args = _tower_args(cfg, which)
    d = rel_l2(vit_tower8(sd, *args), vsm_oracle.vit_tower(sd, *args))
    print(f"{which}: fake-quant tower vs bf16 tower rel-L2 {d:.3e}")
    assert 1e-4 < d < 0.15, d


def test_lin8_adds_the_bias_in_fp32_before_the_rounding():
    """bf16(acc * sa * sw + b), not bf16(bf16(acc * sa * sw) + b).  One-element rows quantise exactly (code 448 on both sides), so the
    product is 3 * 87 = 261: a tie between the bf16 neighbours 260 and 262 that rounds to 260 on its own, after which + 0.25 is lost;
    added in fp32 first, 261.25 rounds to 262."""
    from _vit8_oracle import lin8
    sd = {"l.weight": torch.tensor([[87.0] + [0.0] * 7]).bfloat16(), "l.bias": torch.tensor([0.25]).bfloat16()}
    x = torch.tensor([[3.0] + [0.0] * 7]).bfloat16()
    assert float(lin8(sd, ["l"], x)) == 262.0
    assert float((torch.tensor(261.0).bfloat16() + torch.tensor(0.25).bfloat16())) == 260.0      # what the other order would give


def test_vit_w8a8_takes_reserved_0_and_the_struct_keeps_its_size():
    assert CVstarConfig.vit_w8a8.offset == 100
    assert CVstarConfig.llm_w8a8.offset == 96
    assert ctypes.sizeof(CVstarConfig) == 4 * 32
    c = VSMConfig.tiny(vit_w8a8=1).to_c()
    assert c.vit_w8a8 == 1 and c.llm_w8a8 == 0 and list(c.reserved) == [0] * 6
    assert VSMConfig().vit_w8a8 == 0 and np.all(np.frombuffer(bytes(VSMConfig.tiny().to_c()), np.int32)[25:] == 0)
