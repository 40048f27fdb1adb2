"""Which block linears stream a tile-major image is decided in one place for all decode weight formats (LlmCached::build_quantised
and the fp16 tile block of LlmCached::init).  Whatever that decision is, an image holds the same weights as
the row-major arrays in another order, so an engine built with VSTAR_DECODE_TILED=0 (no image anywhere) and one built without it
must produce the same bits: tokens and logits, at batch 1 (the LDS-ring kernel where the format has one) and at batch 3."""
import functools

import numpy as np
import pytest
import torch

from vstar_amd.config import VQAConfig
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

STEPS = 8


def _cfg(hidden, bits):
    # hidden 512 (4 heads of 128): the smallest width at which the fp16 and int8 images are built at all and the ring kernel runs
    # (K >= 512); mlp 1024: whole 32-row gate|up tiles and K % 128 == 0 for down.  hidden 256: int8 builds no image, int4 builds them.
    return VQAConfig.tiny(llm_hidden=hidden, llm_heads=hidden // 128, llm_mlp=2 * hidden, llm_layers=2, llm_vocab=320, max_slots=4,
                          max_ctx=128).with_decode_bits(bits)


@functools.lru_cache(maxsize=None)
def _weights(hidden):
    return random_state_dict(_cfg(hidden, 0), seed=17, dtype=torch.float16)


def _prompts(n):
    g = torch.Generator().manual_seed(40 + n)
    return [[1] + torch.randint(3, 300, (11 + 3 * i,), generator=g).tolist() for i in range(n)]


def _greedy(eng, prompts):
    """Prefill, then STEPS greedy steps of all sequences: per forward call the wanted rows' logits and their arg-max."""
    n = len(prompts)
    want = [(i, -1) for i in range(n)]
    logits, tok = eng.forward([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], want)
    out = [(logits, tok.copy())]
    for t in range(STEPS):
        step = [Seq([int(tok[i])], kv_slot=i, past_len=len(prompts[i]) + t) for i in range(n)]
        logits, tok = eng.forward(step, want)
        out.append((logits, tok.copy()))
    return out


@pytest.mark.parametrize("hidden,bits", [(512, 0), (512, 8), (512, 4), (256, 8), (256, 4)])
def test_tile_major_images_do_not_change_a_bit(cuda, monkeypatch, hidden, bits):
    runs = []
    for flag in ("0", None):
        if flag is None:
            monkeypatch.delenv("VSTAR_DECODE_TILED", raising=False)
        else:
            monkeypatch.setenv("VSTAR_DECODE_TILED", flag)          # read when the decode runner is built
        eng = VqaEngine(_cfg(hidden, bits), 0)
        eng.load_state_dict(_weights(hidden))
        assert eng.decode_weight_bits() == bits
        runs.append([_greedy(eng, _prompts(n)) for n in (1, 3)])
        del eng
    for row_major, tiled in zip(*runs):
        assert len(row_major) == len(tiled) == STEPS + 1
        for (la, ta), (lb, tb) in zip(row_major, tiled):
            assert np.isfinite(la.astype(np.float32)).all()
            assert ta.tolist() == tb.tolist()
            assert np.array_equal(la.view(np.int16), lb.view(np.int16))
