"""Per-token log-probabilities on the MI355X (csrc/logprob.hip): the op against the CPU oracle
(tests/_logprob_oracle.py) and, bit for bit, against the scoring kernel; the engine's stage against the op applied to the logits of
the same call; the decode drivers against host loops; and the calls that do not ask, which must not move.  Every test here needs a
symbol or keyword the feature adds."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _logprob_oracle as L
from tests import _score_oracle as S
from tests.test_logit_rules_gpu import _image, _plans_for, _prepare
from tests.test_score_gpu import _prompts, make_row, op_score
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.logits import LogitRules
from vstar_amd.spec import ReplayDrafter
from vstar_amd.vqa import VQA_LLM, sampling_params
from vstar_amd.vqa_engine import Seq, TokenLogprobs, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu


def op_logprobs(lib, x_dev, tokens, n_top, vocab=None, want_rank=True):
    """vstar_vqa_op_logprobs on device rows x_dev [rows, ld], the first `vocab` (default ld) of each -> TokenLogprobs."""
    rows, ld = x_dev.shape
    vocab = ld if vocab is None else vocab
    tk = np.ascontiguousarray(tokens, np.int32)
    lp = np.empty(rows, np.float32)
    rank = np.empty(rows, np.int32) if want_rank else None
    tt, tl = np.empty((rows, n_top), np.int32), np.empty((rows, n_top), np.float32)
    dt = _lib.F16 if x_dev.dtype == torch.float16 else _lib.BF16
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None       # noqa: E731
    _lib.check_vqa(lib.vstar_vqa_op_logprobs(ctypes.c_void_p(x_dev.data_ptr()), dt, rows, vocab, ld, p(tk), n_top, p(lp), p(rank),
                                             p(tl), p(tt)))
    return TokenLogprobs(lp, rank, tt, tl)


def same_bits(a: TokenLogprobs, b: TokenLogprobs):
    return all(x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def check_against_oracle(got: TokenLogprobs, logits, tokens, n_top, what):
    """The project's <= 1-ulp rule (tests/test_score_gpu.check_rows): the float outputs equal the oracle's fp32 value or its fp32
    neighbour, the integer outputs are equal exactly.  Returns how many floats needed the neighbour."""
    lp, rank, tt, tl = L.logprobs(logits, tokens, n_top)
    assert np.array_equal(got.top_token, tt), what
    if got.rank is not None:
        assert np.array_equal(got.rank, rank), what
    d1, d2 = S.ulp_distance(got.token_logprob, lp), S.ulp_distance(got.top_logprob, tl)
    assert d1.max() <= 1 and (d2.size == 0 or d2.max() <= 1), (what, int(d1.max()), int(d2.max(initial=0)))
    return int((d1 == 1).sum() + (d2 == 1).sum())


KINDS = ("random", "peaked", "flat", "masked")


def op_case(dtype, V, cuda):
    g = torch.Generator().manual_seed(V)
    x = torch.stack([make_row(KINDS[r % 4], V, g) for r in range(12)]).to(dtype)
    tk = torch.randint(0, V, (12,), generator=g)
    tk[0] = int(x[0].float().argmax())                                 # the arg-max: rank 0
    if V > 4:
        tk[3] = int(torch.isinf(x[3].float()).nonzero()[0])            # a -inf token: -inf
    xd = torch.zeros(12, V + 5, dtype=dtype)
    xd[:, :V] = x
    return x, tk, xd.to(cuda)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [1, 2, 33, 320, 32001, 32768, 32769, 40003])
def test_op_against_oracle(cuda, lib, dtype, V):
    x, tk, xd = op_case(dtype, V, cuda)
    n_nb = 0
    xf = x.float()
    am = op_logprobs(lib, xd, xf.argmax(-1).numpy(), 0, vocab=V)         # the arg-max's own log-probability
    for n_top in (0, 1, 5, 32):
        got = op_logprobs(lib, xd, tk.numpy(), n_top, vocab=V)
        n_nb += check_against_oracle(got, x, tk, n_top, (dtype, V, n_top))
        assert got.rank[0] == 0
        if V > 4:
            assert got.token_logprob[3] == -np.inf
        if n_top:
            free = (xf == xf.max(-1, keepdim=True).values).sum(-1).numpy() == 1       # a tie-free maximum: entry 0 is the arg-max
            assert free.any() and np.array_equal(got.top_token[free, 0], xf.argmax(-1).numpy()[free])
            assert np.array_equal(got.top_logprob[free, 0].view(np.int32), am.token_logprob[free].view(np.int32))
            assert (got.top_token[:, min(n_top, V):] == -1).all() and np.isnan(got.top_logprob[:, min(n_top, V):]).all()
        no_rank = op_logprobs(lib, xd, tk.numpy(), n_top, vocab=V, want_rank=False)          # the rank is optional
        assert no_rank.rank is None and same_bits(no_rank._replace(rank=got.rank), got)
    print(f"logprob op vs oracle {dtype} V={V}: {n_nb} floats needed the fp32 neighbour")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [320, 32001, 40003])
def test_op_equals_the_scoring_kernel_bit_for_bit(cuda, lib, dtype, V):
    x, tk, xd = op_case(dtype, V, cuda)
    got = op_logprobs(lib, xd, tk.numpy(), 5, vocab=V)
    nll, rank, _ = op_score(lib, xd, tk.numpy(), vocab=V)
    assert np.array_equal(got.token_logprob.view(np.int32), (-nll).view(np.int32)) and np.array_equal(got.rank, rank)
    for j in range(5):
        nll_j, _, _ = op_score(lib, xd, got.top_token[:, j], vocab=V)
        assert np.array_equal(got.top_logprob[:, j].view(np.int32), (-nll_j).view(np.int32)), j


def test_op_special_rows_and_errors(cuda, lib):
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[1.0, 2.0, 2.0, 3.0],          # ties: index order among equals
                      [1.5, 1.5, 1.5, 1.5],          # all flat
                      [-inf, 0.0, -inf, -inf],       # one-hot with -inf
                      [1.0, nan, 0.0, 0.5],          # a NaN element: last, every log-probability NaN
                      [0.0, -0.0, 0.0, -0.0],        # -0 == +0: index order
                      [-inf, 0.0, -inf, -inf],       # a -inf chosen token
                      [4.0, 3.0, 2.0, 1.0]])         # no token on this row
    tk = [1, 2, 1, 0, 3, 0, -1]
    for dtype in (torch.float16, torch.bfloat16):
        xd = x.to(dtype).to(cuda)
        for n_top in (3, 4, 6):
            got = op_logprobs(lib, xd, tk, n_top)
            check_against_oracle(got, x.to(dtype), tk, n_top, ("special", dtype, n_top))
        assert got.top_token.tolist() == [[3, 1, 2, 0, -1, -1], [0, 1, 2, 3, -1, -1], [1, 0, 2, 3, -1, -1], [0, 3, 2, 1, -1, -1],
                                          [0, 1, 2, 3, -1, -1], [1, 0, 2, 3, -1, -1], [-1] * 6]
        assert got.rank.tolist() == [1, 0, 0, 0, 0, 1, -1]
        lp, tl = got.token_logprob, got.top_logprob
        assert lp[1] == np.float32(-np.log(4.0)) and (tl[1, :4] == lp[1]).all() and lp[2] == 0.0 and tl[2, :4].tolist() == [0.0, -inf, -inf, -inf]
        assert np.isnan(lp[3]) and np.isnan(tl[3]).all() and lp[5] == -inf and np.isnan(lp[6]) and np.isnan(tl[6]).all()
    xd = torch.zeros(2, 8, dtype=torch.float16, device=cuda)
    with pytest.raises(_lib.VstarError, match="n_top"):
        op_logprobs(lib, xd, [0, 1], 33)
    with pytest.raises(_lib.VstarError, match="token"):
        op_logprobs(lib, xd, [0, 8], 2)
    ok = op_logprobs(lib, xd, [0, -5], 2)                              # the library stays usable
    assert ok.top_token.tolist() == [[0, 1], [-1, -1]] and S.ulp_distance(ok.token_logprob[:1], np.float32([-np.log(8.0)])).max() <= 1


# ------------------------------------------------ the engine ------------------------------------------------
_ENGINES = {}


def _engine(kind):
    """tiny: VQAConfig.tiny(); kv8: the same with kv_cache_format = 1; w4: with decode_weight_format = 1."""
    if kind not in _ENGINES:
        cfg = VQAConfig.tiny()
        cfg = cfg.with_kv_bits(8) if kind == "kv8" else cfg.with_decode_bits(4) if kind == "w4" else cfg
        assert (cfg.kv_cache_format, cfg.decode_weight_format) == {"tiny": (0, 0), "kv8": (1, 0), "w4": (0, 1)}[kind]
        eng = VqaEngine(cfg, 0)
        eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
        _ENGINES[kind] = (eng, cfg)
    return _ENGINES[kind]


@pytest.mark.parametrize("kind", ["tiny", "kv8", "w4"])
def test_engine_stage_equals_op_on_the_logits_of_the_same_call(cuda, lib, kind):
    eng, cfg = _engine(kind)
    g = torch.Generator().manual_seed(7)
    rows = _prompts(eng)

    def on_logits(lg, tokens, n=5):
        return op_logprobs(lib, torch.from_numpy(lg).to(cuda), tokens, n)

    def argmax_and_sample(seqs, want):
        lg0, am0 = eng.forward(seqs, want)
        lg1, am1, rec = eng.forward(seqs, want, logprobs=5)
        assert np.array_equal(lg1.view(np.int16), lg0.view(np.int16)) and np.array_equal(am1, am0)
        assert rec.top_token.shape == (len(want), 5) and rec.token_logprob.dtype == np.float32 and rec.rank.dtype == np.int32
        assert same_bits(rec, on_logits(lg0, am0)) and (rec.rank == 0).all() and np.array_equal(rec.top_token[:, 0], am0)
        none, am2, rec0 = eng.forward(seqs, want, logits=False, logprobs=0)
        assert none is None and np.array_equal(am2, am0) and same_bits(rec0, on_logits(lg0, am0, 0))
        prm = [sampling_params(0.8, 50, 0.9, seed=11 + j, step=j) for j in range(len(want))]
        tok0 = eng.forward_sample(seqs, want, prm)
        tok1, rec = eng.forward_sample(seqs, want, prm, logprobs=5)
        assert np.array_equal(tok1, tok0) and same_bits(rec, on_logits(lg0, tok0))       # of the un-warped row
        return lg0, am0, prm

    # a ragged prefill: the last row of every sequence (one of them three times), some inner rows
    seqs = [Seq(r, kv_slot=i) for i, r in enumerate(rows)]
    argmax_and_sample(seqs, [(0, -1), (1, -1), (1, -1), (1, -1), (2, -1), (0, 5), (2, 100), (1, 0)])
    # forked multi-row continuations, every row wanted: the verify call's shape
    conts = [torch.randint(3, 300, (n,), generator=g).tolist() for n in (7, 1, 12, 4)]
    fork = [Seq(c, kv_slot=4 + j, past_len=len(rows[j % 3]), prefix_slot=j % 3) for j, c in enumerate(conts)]
    want = [(j, t) for j, c in enumerate(conts) for t in range(len(c))]
    groups = np.concatenate([[0], np.cumsum([len(c) for c in conts])])
    lg0, am0, prm = argmax_and_sample(fork, want)
    # drafts: the arg-max on even rows (accepted by the greedy verify), a wrong token on the odd ones
    drafts = sum([[int(am0[groups[j] + r]) if r % 2 == 0 else (int(am0[groups[j] + r]) + 1) % cfg.llm_vocab for r in range(len(c) - 1)] + [-1]
                  for j, c in enumerate(conts)], [])
    for p in (None, prm):
        acc0, tok0 = eng.forward_verify(fork, want, groups, drafts, p)
        acc1, tok1, rec = eng.forward_verify(fork, want, groups, drafts, p, logprobs=5)
        assert np.array_equal(acc1, acc0) and np.array_equal(tok1, tok0) and same_bits(rec, on_logits(lg0, tok0))
        behind = tok0 < 0
        assert behind.any() and (~behind).sum() == int(acc0.sum()) + len(conts)
        assert np.isnan(rec.token_logprob[behind]).all() and (rec.rank[behind] == -1).all() and (rec.top_token[behind] == -1).all() \
            and np.isnan(rec.top_logprob[behind]).all() and not np.isnan(rec.token_logprob[~behind]).any()
    if kind == "tiny":      # with edits: the record is of the EDITED row
        edits = LogitRules.pack(_plans_for(len(want), cfg.llm_vocab, 3, am0))
        lgE, amE = eng.forward(fork, want, edits=edits)
        lgE1, amE1, rec = eng.forward(fork, want, edits=edits, logprobs=5)
        assert np.array_equal(lgE1.view(np.int16), lgE.view(np.int16)) and np.array_equal(amE1, amE) and amE.tolist() != am0.tolist()
        assert same_bits(rec, on_logits(lgE, amE)) and not same_bits(rec, on_logits(lg0, amE))
        # the tails without such an output refuse; bad arguments are refused before any device work; the engine stays usable
        import inspect
        assert "logprobs" not in inspect.signature(VqaEngine.forward_beam).parameters
        assert "logprobs" not in inspect.signature(VqaEngine.forward_score).parameters
        for n in (33, -1):
            with pytest.raises(ValueError, match="logprobs"):
                eng.forward(fork, want, logprobs=n)
        bad = _lib.VqaLogprobs(33, rec.token_logprob.ctypes.data, None, rec.top_logprob.ctypes.data, rec.top_token.ctypes.data)
        args, _keep = eng._rows_args(fork, want)
        with pytest.raises(_lib.VstarError, match="n_top"):
            _lib.check_vqa(eng.lib.vstar_vqa_forward_logprobs(eng.handle, *args, None, None, None, ctypes.byref(bad)), eng.handle)
        lg2, am2 = eng.forward(fork, want)
        assert np.array_equal(lg2.view(np.int16), lg0.view(np.int16)) and np.array_equal(am2, am0)


# ------------------------------------------------ the decode loops ------------------------------------------------
QUESTIONS = ("What is in the picture?", "Describe it.", "What colour is the bus?")


def _host_rows(llm, samples, ids):
    """The logits rows VQA_LLM._decode's engine calls pick from, by the same calls with logits=True: one prefill of every sample,
    then one call per position over the sequences that generate a token there (ids: what they generated)."""
    eng = llm.engine
    seqs, lens, _ = _prepare(llm, samples)
    n = len(seqs)
    lg, _ = eng.forward(seqs, [(i, -1) for i in range(n)])
    rows = [[lg[i]] for i in range(n)]
    pos, t = list(lens), 1
    live = [i for i in range(n) if len(ids[i]) > t]
    while live:
        lg, _ = eng.forward([Seq([ids[i][t - 1]], kv_slot=seqs[i].kv_slot, past_len=pos[i]) for i in live], [(j, 0) for j in range(len(live))])
        for j, i in enumerate(live):
            rows[i].append(lg[j])
            pos[i] += 1
        t += 1
        live = [i for i in live if len(ids[i]) > t]
    return [torch.from_numpy(np.stack(r)) for r in rows]


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_free_form_batch_logprobs_equal_host_loop(cuda, sampled):
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    samples = [dict(image=_image(i), question=q) for i, q in enumerate(QUESTIONS)]
    kw = dict(temperature=0.8, top_p=0.9, seed=11) if sampled else {}
    texts0 = llm.free_form_batch(samples, 8, **kw)
    ids0 = [list(o) for o in llm.generated_ids]
    assert llm.generated_logprobs is None
    texts = llm.free_form_batch(samples, 8, logprobs=3, **kw)
    ids = [list(o) for o in llm.generated_ids]
    assert texts == texts0 and ids == ids0 and len(llm.generated_logprobs) == 3
    n_nb = 0
    for i, (rec, x) in enumerate(zip(llm.generated_logprobs, _host_rows(llm, samples, ids))):
        assert len(rec.token_logprob) == len(ids[i]) == len(x) and rec.top_token.shape == (len(ids[i]), 3)
        n_nb += check_against_oracle(rec, x, ids[i], 3, ("free_form_batch", sampled, i))
        if not sampled:
            assert (rec.rank == 0).all() and rec.top_token[:, 0].tolist() == ids[i]
    if sampled:
        assert any((rec.rank > 0).any() for rec in llm.generated_logprobs)      # some draw is not the arg-max: its own log-probability
    llm.free_form_inference(samples[1]["image"], samples[1]["question"], max_new_tokens=8, logprobs=3, **({**kw, "seed": 12} if sampled else {}))
    assert list(llm.generated_ids[0]) == ids[1] and len(llm.generated_logprobs) == 1
    print(f"free_form_batch logprobs vs host loop ({'sampled' if sampled else 'greedy'}): {n_nb} floats needed the fp32 neighbour")


def test_speculative_decode_logprobs_equal_the_op_on_its_verify_rows(cuda, lib):
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    eos, V, max_new, n = llm.eos_token_id, cfg.llm_vocab, 12, 3
    g = torch.Generator().manual_seed(93)
    prompts = [[1] + torch.randint(3, 300, (8 + 2 * i,), generator=g).tolist() for i in range(n)]
    lens = [len(p) for p in prompts]
    seqs = [Seq(p, kv_slot=i) for i, p in enumerate(prompts)]
    plain = llm.greedy_decode(seqs, lens, max_new)
    replay = ReplayDrafter(prompts, plain, V, corrupt=0.35, seed=n)
    ids0 = llm.speculative_decode(seqs, lens, prompts, max_new, 3, None, replay)
    # spies: every call that asks is repeated with logits=True (the same rows again: the same K/V, the logits the call picked from)
    expect = [[] for _ in range(n)]
    real_forward, real_verify = eng.forward, eng.forward_verify

    def forward(step, want, logits=True, edits=None, logprobs=None):
        res = real_forward(step, want, logits=logits, edits=edits, logprobs=logprobs)
        if logprobs is not None:
            lg, am = real_forward(step, want)
            assert np.array_equal(am, res[1]) and same_bits(res[2], op_logprobs(lib, torch.from_numpy(lg).to(cuda), am, logprobs))
            for j, s in enumerate(step):
                expect[s.kv_slot].append(res[2].rows(slice(j, j + 1)))
        return res

    def forward_verify(step, wanted, groups, draft, params=None, edits=None, logprobs=None):
        res = real_verify(step, wanted, groups, draft, params, edits=edits, logprobs=logprobs)
        if logprobs is not None:
            lg, _ = real_forward(step, wanted)
            acc, tok, rec = res
            assert same_bits(rec, op_logprobs(lib, torch.from_numpy(lg).to(cuda), tok, logprobs))
            for j, s in enumerate(step):
                new = [int(t) for t in tok[groups[j]:groups[j] + int(acc[j]) + 1]]
                keep = new.index(eos) + 1 if eos in new else len(new)
                expect[s.kv_slot].append(rec.rows(slice(groups[j], groups[j] + keep)))
        return res
    eng.forward, eng.forward_verify = forward, forward_verify
    try:
        ids, recs = llm.speculative_decode(seqs, lens, prompts, max_new, 3, None, replay, logprobs=3)
    finally:
        del eng.forward, eng.forward_verify
    assert ids == ids0 and 0 < llm.spec_stats["accepted"] < llm.spec_stats["drafted"]
    for i in range(n):
        assert len(recs[i].token_logprob) == len(ids[i]) and recs[i].top_token.shape == (len(ids[i]), 3)
        assert same_bits(recs[i], TokenLogprobs.concat(expect[i], 3))
        assert (recs[i].rank == 0).all() and recs[i].top_token[:, 0].tolist() == ids[i] and not np.isnan(recs[i].token_logprob).any()


def test_generate_returns_transition_scores(cuda):
    from vstar_amd.api import LlavaSearchModel
    from vstar_amd import vqa
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    model = LlavaSearchModel(llm)
    image, q = _image(5), "What is in the picture?"
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), llm.tokenizer)).unsqueeze(0)
    pix = llm.image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0]
    kw = dict(images=pix.unsqueeze(0).half(), max_new_tokens=6)
    plain = model.generate(input_ids, **kw)
    out = model.generate(input_ids, return_dict_in_generate=True, output_scores=True, top_logprobs=2, **kw)
    assert torch.equal(out.sequences, plain) and out.scores is None
    llm.free_form_inference(image, q, max_new_tokens=6, logprobs=2)
    rec = llm.generated_logprobs[0]
    T = plain.shape[1] - input_ids.shape[1]
    assert out.transition_scores.shape == (1, T) and out.transition_scores.dtype == torch.float32
    assert out.top_tokens.shape == (1, T, 2) and out.top_logprobs.shape == (1, T, 2) and out.token_ranks.shape == (1, T)
    assert same_bits(TokenLogprobs(out.transition_scores[0].numpy(), out.token_ranks[0].numpy(), out.top_tokens[0].numpy(),
                                   out.top_logprobs[0].numpy()), rec)
    only = model.generate(input_ids, return_dict_in_generate=True, **kw)
    assert torch.equal(only.sequences, plain) and vars(only).keys() == {"sequences"}
    assert torch.equal(model.generate(input_ids, output_scores=True, **kw), plain)         # without the flag: the tensor, as in HF


# ------------------------------------------------ nothing else moved ------------------------------------------------
def test_nothing_else_moved(cuda):
    """An engine that never asks, recorded; after ONE call with logprobs the same calls give the same bytes."""
    cfg = VQAConfig.tiny()
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
    llm = VQA_LLM(cfg=cfg, engine=eng)
    s = dict(image=_image(2), question=QUESTIONS[0])

    def snapshot():
        out = []
        rows = _prompts(eng, (20, 33), seed=4)          # (encodes its images: the decodes below overwrite the feature slots)
        lg, am = eng.forward([Seq(r, kv_slot=i) for i, r in enumerate(rows)], [(0, -1), (1, -1)])
        out += [lg.tobytes(), am.tobytes()]
        pos, cur = [len(r) for r in rows], am
        for _ in range(3):
            lg, cur = eng.forward([Seq([int(cur[i])], kv_slot=i, past_len=pos[i]) for i in range(2)], [(0, 0), (1, 0)])
            out += [lg.tobytes(), cur.tobytes()]
            pos = [p + 1 for p in pos]
        for kw in (dict(), dict(temperature=0.8, top_p=0.9, seed=11), dict(num_beams=2), dict(speculative=3), dict(repetition_penalty=1.3)):
            llm.free_form_inference(s["image"], s["question"], max_new_tokens=6, **kw)
            out.append([list(x) for x in llm.generated_ids])
        return out
    before = snapshot()
    assert eng.forward([Seq([1, 5, 6, 7], kv_slot=0)], [(0, -1)], logits=False, logprobs=5)[2].top_token.shape == (1, 5)
    assert snapshot() == before


GRAPH_CHILD = """
import json, torch
from vstar_amd.config import VSMConfig
from vstar_amd.engine import VstarEngine
from vstar_amd.weights import random_state_dict
cfg = VSMConfig.tiny(max_text_len=128)
eng = VstarEngine(cfg, 0)
eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.bfloat16, share_layers=True))
clip = torch.randn(1, 3, cfg.clip_image_size, cfg.clip_image_size, generator=torch.Generator().manual_seed(3))
print("IDS " + json.dumps([int(t) for t in eng.generate(clip, [1, -200, 5, 6, 7, 8], 8, 2)]))
"""


def test_decode_graph_on_and_off_give_the_same_ids(cuda):
    """The captured greedy step shares the runner this feature extends: VSTAR_DECODE_GRAPH=1 and =0 decode the same ids.  The
    switch is read once per process, so each setting runs in a child."""
    ids = []
    for v in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", GRAPH_CHILD], cwd=str(Path(__file__).resolve().parents[1]),
                           env={**os.environ, "VSTAR_DECODE_GRAPH": v}, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        ids.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("IDS ")][-1][4:]))
    assert ids[0] == ids[1] and len(ids[0]) >= 1


def test_eval_loop_records_logprobs_only_when_asked(cuda, tmp_path):
    """eval_model on a two-question synthetic benchmark: --vqa-logprobs off writes today's records; on adds `freeform_logprobs`, the
    rest of every record unchanged, single and batched free-form passes alike."""
    from types import SimpleNamespace
    from PIL import Image
    from vstar_amd import bench_eval
    from vstar_amd.config import VSMConfig
    from vstar_amd.vsm import VSM
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    vsm = VSM(SimpleNamespace(version="synthetic", vision_tower="synthetic", conv_type="llava_v1", use_mm_start_end=True,
                              model_max_length=512), cfg=VSMConfig.tiny(max_text_len=128), synthetic_seed=0)
    rng = np.random.default_rng(9)
    for split in ("direct_attributes", "relative_position"):
        (tmp_path / split).mkdir()
        Image.fromarray(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)).save(tmp_path / split / "img0.jpg")
        json.dump({"question": "What is the colour of the mug?", "options": ["red", "blue"]}, open(tmp_path / split / "img0.json", "w"))
    real = llm.free_form_batch
    llm.free_form_batch = lambda samples, *a, **kw: real(samples, 5, **kw)          # short answers: five new tokens
    llm.free_form_inference = lambda image, question, **kw: llm.free_form_batch([dict(image=image, question=question)], **kw)[0]
    base = dict(benchmark_folder=str(tmp_path), minimum_size_scale=4.0, minimum_size=224, vsm_model_path="synthetic", max_found_objects=5)
    try:
        runs = {}
        for name, kw in (("off", {}), ("on", dict(vqa_logprobs=2)), ("on_batched", dict(vqa_logprobs=2, vqa_batch=2))):
            runs[name] = bench_eval.eval_model(SimpleNamespace(**base, **kw, output_path=str(tmp_path / f"{name}.json")), llm, vsm)
            assert json.load(open(tmp_path / f"{name}.json")) == runs[name]
    finally:
        del llm.free_form_batch, llm.free_form_inference
    for split, recs in runs["off"].items():
        for a, b, c in zip(recs, runs["on"][split], runs["on_batched"][split]):
            assert "freeform_logprobs" not in a and {k: v for k, v in b.items() if k != "freeform_logprobs"} == a
            lp = b["freeform_logprobs"]
            assert set(lp) == {"mean_token_logprob", "token_ids", "token_logprob", "token_rank", "top_tokens", "top_logprobs"}
            T = len(lp["token_ids"])
            assert 1 <= T <= 5 and len(lp["token_logprob"]) == T and np.shape(lp["top_tokens"]) == (T, 2)
            assert lp["mean_token_logprob"] == float(np.mean(lp["token_logprob"])) and lp["token_rank"] == [0] * T
            assert [row[0] for row in lp["top_tokens"]] == lp["token_ids"] and c["freeform_logprobs"]["token_ids"] == lp["token_ids"]
