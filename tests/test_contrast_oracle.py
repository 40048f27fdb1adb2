"""Contrastive search without a GPU: the oracle of the step (tests/_contrast_oracle.py) on a table-driven toy
model, the ABI additions, and the Python argument checks that fire before the engine is touched.  Every test here needs a symbol
or keyword the feature adds."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _contrast_oracle as C
from vstar_amd import _lib


def table_model(hidden_of, logits_of):
    """model_fn of a toy model whose hidden row is a function of the token at that position and whose logits row is a function
    of the last token."""
    def fn(tokens):
        return np.stack([hidden_of[t] for t in tokens]), logits_of[tokens[-1]]
    return fn


def greedy(model_fn, prompt, max_new, eos=None):
    seq, out = list(prompt), []
    for _ in range(max_new):
        x = np.asarray(model_fn(seq)[1], np.float64)
        out.append(int(np.argmax(x)))                  # (the first maximum: the lowest index)
        seq.append(out[-1])
        if out[-1] == eos:
            break
    return out


def test_alpha_zero_is_greedy_for_every_k():
    g = np.random.default_rng(0)
    V, H = 12, 8
    fn = table_model(g.standard_normal((V, H)), g.standard_normal((V, V)) * 3)
    for prompt in ([1], [3, 7, 2]):
        ref = greedy(fn, prompt, 9)
        for k in (2, 5, 12):
            assert C.contrastive_search(fn, prompt, 0.0, k, 9) == ref, (prompt, k)
    assert C.contrastive_search(fn, [1], 0.0, 3, 9, eos=ref[2])[-1] == ref[2]          # it stops behind eos


def test_hand_computed_three_steps():
    # four tokens with hidden rows h0 .. h3 and transition probabilities P[last]; prompt [0], alpha = 0.5, k = 2
    hid = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [-1.0, 0.0]])
    P = np.array([[0.60, 0.30, 0.05, 0.05],           # candidates 0 (0.6), 1 (0.3)
                  [0.05, 0.50, 0.40, 0.05],           # candidates 1 (0.5), 2 (0.4)
                  [0.05, 0.05, 0.50, 0.40],           # candidates 2 (0.5), 3 (0.4)
                  [0.25, 0.25, 0.25, 0.25]])
    fn = table_model(hid, np.log(P))
    # step 1, history [h0]:          0: 0.5 * 0.6 - 0.5 * 1 = -0.2          1: 0.5 * 0.3 - 0.5 * 0 = 0.15               -> 1
    # step 2, history [h0, h1]:      1: 0.25 - 0.5 * 1 = -0.25              2: 0.2 - 0.5 / sqrt(2) = -0.1536            -> 2
    # step 3, history [h0, h1, h2]:  2: 0.25 - 0.5 * 1 = -0.25              3: 0.2 - 0.5 * max(-1, 0, -0.707) = 0.2     -> 3
    assert C.contrastive_search(fn, [0], 0.5, 2, 3) == [1, 2, 3]
    assert greedy(fn, [0], 3) == [0, 0, 0]
    tok, prob = C.topk_probs(np.log(P[1]), 2)
    assert tok.tolist() == [1, 2] and np.allclose(prob, [0.5, 0.4], rtol=1e-6) and prob.dtype == np.float32
    pen = C.penalty(hid[[1, 2]], hid[:2])
    assert np.allclose(pen, [1.0, np.sqrt(0.5)], rtol=1e-15)
    s, score = C.score_select(prob, pen, 0.5)
    assert s == 1 and np.allclose(score, [-0.25, 0.2 - 0.5 * np.sqrt(0.5)], atol=1e-7)
    assert C.penalty(hid[[3]], hid[:3])[0] == 0.0                                   # the max of (-1, 0, -0.707)


def test_ties_zero_norm_and_order_rules():
    assert C.score_select([0.5, 0.5, 0.5], [0.2, 0.2, 0.2], 0.6)[0] == 0            # the lowest index on a tie
    assert C.score_select([0.1, 0.5, 0.5], [0.2, 0.2, 0.2], 0.6)[0] == 1
    assert C.score_select([0.3, 0.2], [0.9, 0.1], 0.0)[0] == 0 and C.score_select([0.3, 0.2], [0.9, 0.1], 1.0)[0] == 1
    z = np.zeros((1, 8))
    h = np.ones((3, 8))
    assert C.penalty(z, h)[0] == 0.0                                               # a zero candidate
    assert C.penalty(h[:1], np.concatenate([z, z]))[0] == 0.0                       # an all-zero history
    assert C.penalty(-h[:1], np.concatenate([z, h[:1]]))[0] == 0.0                  # max(0, -1)
    inf, nan = float("inf"), float("nan")
    assert C.topk_probs([1.0, 2.0, 2.0, 3.0], 3)[0].tolist() == [3, 1, 2]           # ties: the lower index first
    assert C.topk_probs([0.0, -0.0, 0.0, -0.0], 4)[0].tolist() == [0, 1, 2, 3]      # -0 == +0
    assert C.topk_probs([1.0, nan, -inf, 0.5], 4)[0].tolist() == [0, 3, 1, 2]       # a NaN sorts as -inf
    assert C.topk_probs([-inf, 0.0, -inf, -inf], 2)[1].tolist() == [1.0, 0.0]


def test_fixed_order_sums():
    g = np.random.default_rng(1)
    for H in (8, 256, 520, 4096):
        h = g.standard_normal(H).astype(np.float16)
        sq = C.row_sum32(h.astype(np.float32) ** 2)
        exact = float((h.astype(np.float64) ** 2).sum())
        assert sq.dtype == np.float32 and abs(float(sq) - exact) <= (H + 16) * 2.0 ** -24 * exact
        assert C.rnorm32(h) == np.float32(1.0) / np.sqrt(sq)
    assert C.rnorm32(np.zeros(16, np.float16)) == 0.0
    # the order is the stated one: lane l adds pieces l, l + 64, ... one element at a time, then the butterfly
    t = g.standard_normal(8 * 130).astype(np.float32)
    lanes = np.zeros(64, np.float32)
    for p in range(130):
        for e in range(8):
            lanes[p % 64] = lanes[p % 64] + t[8 * p + e]
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ o]
    assert C.row_sum32(t) == lanes[0] and (lanes == lanes[0]).all()


def test_abi_additions():
    lib = _lib.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "vstar_vqa.h").read_text()
    for name in ("vstar_vqa_forward_contrast_begin", "vstar_vqa_forward_contrast_step", "vstar_vqa_op_contrast"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTS_VQA and hasattr(lib, name), name
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes, name
    assert "#define VSTAR_VQA_ABI_VERSION 1" in header and "int32_t reserved[5];" in header
    assert len(lib.vstar_vqa_forward_contrast_begin.argtypes) == 12 and len(lib.vstar_vqa_forward_contrast_step.argtypes) == 18
    assert len(lib.vstar_vqa_op_contrast.argtypes) == 20
    # the op entry refuses bad arguments before any device work (no GPU needed to get there); the message names the field
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    buf = np.zeros(64, np.float32)
    sel, tok = np.zeros(4, np.int32), np.zeros(64, np.int32)

    def call(logits=buf, cand=buf, hist=buf, hidden=8, hist_len=(3,), goff=(0, 2), prob=(0.5, 0.25), alpha=0.5, rows=2):
        hl, go, pr = np.asarray(hist_len, np.int32), np.asarray(goff, np.int32), np.asarray(prob, np.float32)
        rc = lib.vstar_vqa_op_contrast(p(logits) if logits is not None else None, _lib.F16, rows, 8, 8, p(cand) if cand is not None else None,
                                       hidden, p(hist) if hist is not None else None, p(buf), len(go) - 1, 4, p(hl), p(go), p(pr), alpha, 2,
                                       p(sel), p(tok), p(buf), None)
        return rc, lib.vstar_vqa_last_error(None)

    for kw, word in ((dict(logits=None), b"dev_logits"), (dict(cand=None), b"dev_cand_hidden"), (dict(hist=None), b"dev_hist"),
                     (dict(hidden=12), b"hidden"), (dict(hist_len=(0,)), b"hist_len"), (dict(hist_len=(4,)), b"hist_len"),
                     (dict(alpha=1.5), b"alpha"), (dict(prob=(0.5, 1.5)), b"cand_prob"), (dict(prob=(0.5, float("nan"))), b"cand_prob"),
                     (dict(rows=33, goff=(0, 33), prob=[0.1] * 33), b"group_off"), (dict(goff=(0, 1)), b"group_off")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_python_argument_checks_fire_before_the_engine():
    from vstar_amd.api import LlavaSearchModel
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa import VQA_LLM, check_contrast
    cfg = VQAConfig.tiny()
    llm = VQA_LLM(cfg=cfg, engine=SimpleNamespace(cfg=cfg))             # the checks below fire before the engine is touched
    one = [dict(image=None, question="q")]
    for a in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="penalty_alpha"):
            llm.free_form_batch(one, 4, penalty_alpha=a, top_k=4)
    for k in (50, 1, 0, 33, None, 2.5):                                 # 50: the sampling default has to be overridden
        with pytest.raises(ValueError, match="top_k"):
            llm.free_form_batch(one, 4, penalty_alpha=0.6, top_k=k)
    with pytest.raises(ValueError, match="top_k"):
        llm.free_form_inference(None, "q", penalty_alpha=0.6)
    with pytest.raises(ValueError, match="speculative"):
        llm.free_form_batch(one, 4, penalty_alpha=0.6, top_k=4, speculative=3)
    with pytest.raises(NotImplementedError, match="temperature"):
        llm.free_form_batch(one, 4, penalty_alpha=0.6, top_k=4, temperature=0.7)
    with pytest.raises(NotImplementedError, match="num_beams"):
        llm.free_form_batch(one, 4, penalty_alpha=0.6, top_k=4, num_beams=2)
    with pytest.raises(NotImplementedError, match="logits rules"):
        llm.free_form_batch(one, 4, penalty_alpha=0.6, top_k=4, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="logprobs"):
        llm.free_form_batch(one, 4, penalty_alpha=0.6, top_k=4, logprobs=2)
    with pytest.raises(ValueError, match="KV slots"):
        llm.free_form_batch(one * 3, 4, penalty_alpha=0.6, top_k=4)      # 3 x 4 > max_slots = 8, the beam path's message style
    # the existing cases keep their precedence and messages
    with pytest.raises(NotImplementedError, match="log-softmax"):
        llm.free_form_batch(one, 4, num_beams=2, repetition_penalty=1.2, penalty_alpha=0.6, top_k=4)
    with pytest.raises(NotImplementedError, match="beam sampling"):
        llm.free_form_batch(one, 4, num_beams=2, temperature=0.5, penalty_alpha=0.6, top_k=4)
    with pytest.raises(ValueError, match="logprobs"):
        llm.free_form_batch(one, 4, logprobs=33, penalty_alpha=0.6, top_k=4)
    model = LlavaSearchModel(llm)
    ids = torch.tensor([[1, 5, 6]])
    with pytest.raises(ValueError, match="penalty_alpha"):
        model.generate(ids, penalty_alpha=2.0, top_k=4)
    with pytest.raises(ValueError, match="top_k"):
        model.generate(ids, penalty_alpha=0.6)
    with pytest.raises(ValueError, match="contrastive"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, prompt_lookup_num_tokens=3)
    with pytest.raises(NotImplementedError, match="do_sample"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, do_sample=True, temperature=0.7)
    with pytest.raises(NotImplementedError, match="num_beams"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, num_beams=2)
    with pytest.raises(NotImplementedError, match="logits rules"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, no_repeat_ngram_size=2)
    with pytest.raises(NotImplementedError, match="logprobs"):
        model.generate(ids, penalty_alpha=0.6, top_k=4, return_dict_in_generate=True, output_scores=True)
    with pytest.raises(ValueError, match="KV slots"):
        model.generate(ids, penalty_alpha=0.6, top_k=9)
    with pytest.raises(ValueError, match="alpha"):
        llm.contrastive_decode([], [], 4, 1.5, 4)
    with pytest.raises(ValueError, match="k must"):
        llm.contrastive_decode([], [], 4, 0.5, 33)
    kw = dict(sampled=False, num_beams=1, speculative=0, rules=None, logprobs=None)
    assert check_contrast(None, 50, **kw) is None and check_contrast(0, 50, **kw) is None and check_contrast(0.6, 4, **kw) == 0.6
    assert check_contrast(1, 32, **kw) == 1.0 and check_contrast(0.25, 2, **kw) == 0.25
