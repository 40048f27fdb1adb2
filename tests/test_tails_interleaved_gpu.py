"""The five tails of `LlmCached::forward` (arg-max, sampling, beam select, scoring, verify) leave no state behind for each other:
two engines with the same weights run the same six calls on the same rows, one in the reverse order of the other, and every
output is bit-equal.  Each call is made in both regimes: on the prompts (prefill: more than 64 fresh rows, and the re-prefill that
gives the next call an identical KV state) and on a decode step behind them (cached)."""
import numpy as np
import pytest
import torch

from vstar_amd.config import IMAGE_TOKEN_INDEX, VQAConfig
from vstar_amd.vqa import sampling_params
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

CALLS = ("forward", "sample", "beam", "score", "verify", "verify_sampled")


def _engine(cfg, pixels):
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
    eng.encode_images(pixels, 0)
    return eng


def _call(eng, name, seqs, wanted, groups, draft, targets):
    """One tail on the wanted rows -> its outputs as a list of arrays."""
    n = len(wanted)
    prm = [sampling_params(0.8, 50, 0.9, seed=11 + j, step=j) for j in range(n)]
    if name == "forward":
        return list(eng.forward(seqs, wanted))
    if name == "sample":
        return [eng.forward_sample(seqs, wanted, prm)]
    if name == "beam":                                   # one group per wanted row
        return list(eng.forward_beam(seqs, wanted, np.zeros(n, np.float32), np.arange(n + 1), 2, logits=True))
    if name == "score":
        return list(eng.forward_score(seqs, wanted, targets, rank=True))
    return list(eng.forward_verify(seqs, wanted, groups, draft, prm if name == "verify_sampled" else None))


def _run(eng, order, prompts, cur, nxt):
    """Every call of `order` on the prompts (prefill regime), then on the decode step behind them (cached regime): one row [cur]
    per sequence, for the verify tail the rows [cur, draft] with the draft `nxt` a prior greedy step gave."""
    nseq = len(prompts)
    pre = [Seq(p, kv_slot=i) for i, p in enumerate(prompts)]
    last = [(i, -1) for i in range(nseq)]
    out = {}
    for name in order:
        verify = name.startswith("verify")
        out[name, "prefill"] = _call(eng, name, pre, last, np.arange(nseq + 1), [-1] * nseq, cur)
        rows = [[int(cur[i]), int(nxt[i])] if verify else [int(cur[i])] for i in range(nseq)]
        step = [Seq(rows[i], kv_slot=i, past_len=len(prompts[i])) for i in range(nseq)]
        wanted = [(i, r) for i in range(nseq) for r in range(len(rows[i]))]
        groups = np.arange(0, 2 * nseq + 1, 2)
        draft = sum([[int(nxt[i]), -1] for i in range(nseq)], [])
        out[name, "cached"] = _call(eng, name, step, wanted, groups, draft, nxt)
    return out


def test_tails_in_either_order_give_the_same_bits(cuda):
    cfg = VQAConfig.tiny()
    assert cfg.max_slots >= 4
    pixels = torch.randn(1, 3, cfg.clip_image_size, cfg.clip_image_size, generator=torch.Generator().manual_seed(3))
    a, b = _engine(cfg, pixels), _engine(cfg, pixels)
    prompts = [a.expand_ids([1, IMAGE_TOKEN_INDEX] + text, [0], [], None, None) for text in ([5, 6, 7], [9, 10, 11, 12, 13])]
    assert sum(len(p) for p in prompts) > 64             # the prefill regime
    # the greedy tokens both orders refer to: the prompts' arg-max, and the arg-max of the one-row decode step behind them
    _, cur = a.forward([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [(i, -1) for i in range(2)], logits=False)
    _, nxt = a.forward([Seq([int(cur[i])], kv_slot=i, past_len=len(prompts[i])) for i in range(2)], [(0, 0), (1, 0)], logits=False)
    cur, nxt = cur.copy(), nxt.copy()
    out_a = _run(a, CALLS, prompts, cur, nxt)
    out_b = _run(b, CALLS[::-1], prompts, cur, nxt)
    assert set(out_a) == set(out_b) and len(out_a) == 2 * len(CALLS)
    for key, arrays in out_a.items():
        assert len(arrays) == len(out_b[key])
        for i, (x, y) in enumerate(zip(arrays, out_b[key])):
            assert x.dtype == y.dtype and np.array_equal(x, y), (key, i)
    for regime, greedy in (("prefill", cur), ("cached", nxt)):
        assert np.array_equal(out_a["forward", regime][1], greedy)
        assert (out_a["score", regime][1] == 0).all()    # the target is the arg-max: rank 0
        assert np.isfinite(out_a["score", regime][0]).all()
    acc, tok = out_a["verify", "cached"]
    assert acc.tolist() == [1, 1]                        # the true draft is accepted,
    assert tok[0::2].tolist() == nxt.tolist() and (tok[1::2] >= 0).all()      # and one more token follows it
    acc, tok = out_a["verify", "prefill"]
    assert acc.tolist() == [0, 0] and tok.tolist() == cur.tolist()
