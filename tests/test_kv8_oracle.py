"""Block-scaled fp8 KV cache without a GPU: the row round trip's representability in fp16, idempotence and the
documented boundary; the chain oracle's noise floor and the size of the quantisation effect (printed: DESIGN.md quotes them); the
configuration plumbing."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import vqa_oracle as O
from tests._kv8_oracle import LIMIT, kv8_quantize, kv8_round_trip, llama_forward_kv8, rel_l2
from vstar_amd import config as C
from vstar_amd.config import CVqaConfig, VQAConfig
from vstar_amd.weights import random_state_dict

U = 2.0 ** -24


def _rows_of_all_patterns():
    """Every finite fp16 bit pattern with |x| < 63488 at least once, in random company (blocks mix magnitudes), plus rows of
    subnormal-only blocks and rows whose blocks hold one pattern each."""
    bits = np.arange(0x10000, dtype=np.uint16)
    vals = bits.view(np.float16)
    ok = np.isfinite(vals) & (np.abs(vals.astype(np.float32)) < LIMIT)
    pool = bits[ok]
    g = np.random.default_rng(0)
    mixed = g.choice(pool, size=(3000, 128))                                   # all magnitudes in one block
    by_mag = pool[np.abs(pool.view(np.float16).astype(np.float32)).argsort(kind="stable")]
    near = np.resize(by_mag, ((len(by_mag) + 127) // 128, 128))                # neighbours in magnitude share a block
    sub = (g.integers(-1023, 1024, (64, 128))).astype(np.float32) * U          # subnormal-only blocks
    return np.concatenate([mixed.view(np.float16), near.view(np.float16), sub.astype(np.float16)], axis=0)


def test_round_trip_is_representable_in_fp16_idempotent_and_bounded():
    x = torch.from_numpy(_rows_of_all_patterns())
    assert float(x.float().abs().max()) < LIMIT and len(np.unique(x.numpy().view(np.uint16))) > 63000
    dec = kv8_round_trip(x)
    assert torch.equal(dec.half().float(), dec)                                # exactly representable: formats 1 and 2 hold the same numbers
    assert torch.equal(kv8_round_trip(dec.half()), dec)                        # a round trip of a round trip changes nothing
    # the error of a value is at most half a grid step of its block: 2^-4 of the block's power-of-two bound (e4m3: 3 mantissa bits)
    amax = x.float().reshape(-1, 4, 32).abs().amax(-1, keepdim=True)
    err = (dec - x.float()).reshape(-1, 4, 32).abs()
    assert bool((err <= amax / 8 + 1e-30).all())
    # the documented boundary: 63488 is the first fp16 whose block decodes to 65536 (not an fp16 number); 63456 (the fp16 below) does not
    row = torch.zeros(1, 128, dtype=torch.float16)
    row[0, 5] = 63488.0
    assert float(kv8_round_trip(row)[0, 5]) == 65536.0
    row[0, 5] = 63456.0
    assert float(kv8_round_trip(row)[0, 5]) == 61440.0


def test_numpy_face_of_the_oracle():
    g = np.random.default_rng(1)
    x = (g.standard_normal((9, 128)) * 3).astype(np.float16)
    x[1] = 0
    x[2, :32] = 0
    codes, e, xhat = kv8_quantize(x)
    assert codes.shape == (9, 128) and e.shape == (9, 4) and codes.dtype == np.uint8 and e.dtype == np.uint8
    assert (e[1] == 0).all() and (codes[1] == 0).all() and e[2, 0] == 0
    dec = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy() * np.repeat(np.ldexp(1.0, e.astype(np.int32) - 127), 32, axis=1)
    assert np.array_equal(dec.astype(np.float32), xhat.astype(np.float32))
    # the smallest power of two that brings the block maximum to <= 448
    amax = np.abs(x.astype(np.float32)).reshape(9, 4, 32).max(-1)
    nz = amax > 0
    s = np.ldexp(1.0, e.astype(np.int32) - 127)
    assert (amax[nz] / s[nz] <= 448).all() and (amax[nz] / s[nz] > 224).all()


def test_chain_oracle_noise_and_quantisation_effect():
    """The fp16 chain against the fp32 chain of the QUANTISED oracle (its noise floor: the gate of the GPU test is 3 x this), against
    the same figure of the plain oracle, and the effect of the quantisation itself; a continuation with `past` agrees with the
    one-shot prefill of the fp32 chain."""
    cfg = VQAConfig.tiny(llm_hidden=512, llm_heads=4, llm_mlp=1024)
    sd = random_state_dict(cfg, seed=3)
    sd16 = {k: v.half() for k, v in sd.items()}
    sd32 = {k: v.float() for k, v in sd16.items()}
    g = torch.Generator().manual_seed(7)
    ids = [1] + torch.randint(3, 300, (95,), generator=g).tolist()
    emb32 = sd32["model.embed_tokens.weight"][torch.tensor(ids)]
    emb16 = sd16["model.embed_tokens.weight"][torch.tensor(ids)]
    q32, _ = llama_forward_kv8(sd32, cfg, emb32)
    q16, _ = llama_forward_kv8(sd16, cfg, emb16)
    p32, _ = O.llama_forward(sd32, cfg, emb32)
    p16, _ = O.llama_forward(sd16, cfg, emb16)
    noise_q, noise_p, effect = rel_l2(q16.float(), q32), rel_l2(p16.float(), p32), rel_l2(q32, p32)
    same = float((q32.argmax(-1) == p32.argmax(-1)).float().mean())
    print(f"kv8 chain oracle: fp16-vs-fp32 noise {noise_q:.2e} (plain oracle {noise_p:.2e}), quantisation effect {effect:.2e}, "
          f"row arg-maxes unchanged {same:.3f}")
    assert 0 < noise_p < noise_q < 0.1 and noise_q < effect < 0.2 and same > 0.8
    # with `past`: 64 rows, then 32 more — in the fp32 chain the split changes summation shapes only
    a, past = llama_forward_kv8(sd32, cfg, emb32[:64])
    b, past2 = llama_forward_kv8(sd32, cfg, emb32[64:], past)
    assert past2[0][0].shape[1] == 96 and rel_l2(torch.cat([a, b]), q32) < 1e-4
    # the cache holds round-tripped rows: quantising them again changes nothing
    k0 = past2[0][0]
    assert torch.equal(kv8_round_trip(k0), k0)


def test_config_plumbing():
    assert ctypes.sizeof(CVqaConfig) == 4 * (25 + 8)
    assert CVqaConfig.kv_cache_format.offset == 4 * 27 and CVqaConfig.reserved.offset == 4 * 28      # the former reserved[0]
    assert CVqaConfig.decode_weight_format.offset == 4 * 26
    c = VQAConfig.tiny()
    assert c.kv_cache_format == 0 and c.to_c().kv_cache_format == 0 and c.kv_bits() == 0
    c8 = c.with_kv_bits(8)
    assert c8.kv_cache_format == C.KVFMT_MXFP8 == 1 and c8.to_c().kv_cache_format == 1 and c8.kv_bits() == 8
    assert c8.with_kv_bits(0) == c and C.KVFMT_MXFP8_EMULATED == 2
    # independent of the weight modes
    both = c.with_decode_bits(4).with_kv_bits(8)
    assert both.decode_bits() == 4 and both.kv_bits() == 8 and both.with_decode_bits(8).kv_bits() == 8
    with pytest.raises(ValueError):
        c.with_kv_bits(4)
    # the header declares the field and the constants
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vstar_vqa.h")).read()
    assert "int32_t kv_cache_format;" in hdr and "int32_t reserved[5];" in hdr
    assert "#define VSTAR_VQA_KVFMT_MXFP8 1" in hdr and "#define VSTAR_VQA_KVFMT_MXFP8_EMULATED 2" in hdr


def test_cli_flags():
    from types import SimpleNamespace

    import vstar_bench_eval
    from vstar_amd.vqa import VQA_LLM
    assert vstar_bench_eval.parse_args([]).vqa_kv_bits == 0
    a = vstar_bench_eval.parse_args(["--vqa-kv-bits", "8", "--vqa-decode-bits", "4"])
    assert a.vqa_kv_bits == 8 and a.vqa_decode_bits == 4
    with pytest.raises(SystemExit):
        vstar_bench_eval.parse_args(["--vqa-kv-bits", "4"])
    # the user-level spelling: an engine built in the mode is accepted, a mismatch is refused
    c8 = VQAConfig.tiny().with_kv_bits(8)
    assert VQA_LLM(engine=SimpleNamespace(cfg=c8), kv_cache_bits=8).cfg == c8
    with pytest.raises(ValueError, match="kv_cache_bits"):
        VQA_LLM(engine=SimpleNamespace(cfg=VQAConfig.tiny()), kv_cache_bits=8)
