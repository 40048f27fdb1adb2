"""Per-token log-probabilities without a GPU: the oracle of the stage (tests/_logprob_oracle.py) against
torch.log_softmax + torch.topk and against transformers' compute_transition_scores, the ABI additions, and the Python argument checks
that fire before the engine is touched.  Every test here needs a symbol or keyword the feature adds."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _logprob_oracle as L
from tests import _score_oracle as S
from vstar_amd import _lib


def tie_free_rows(rows, V, dtype, g):
    """Rows of V distinct values: for the 16-bit types a random choice among all bit patterns with 2^-6 <= |v| <= 20 (smaller
    magnitudes are distinct logits whose log-softmax values collapse in double: ties for the yardstick, not for the oracle)."""
    if dtype == torch.float32:
        x = torch.stack([(torch.randperm(V, generator=g).float() - V // 2) / 64 for _ in range(rows)])
    else:
        pool = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
        pool = pool[torch.isfinite(pool.float()) & (pool.float().abs() <= 20) & (pool.float().abs() >= 2.0 ** -6)]
        x = torch.stack([pool[torch.randperm(len(pool), generator=g)[:V]] for _ in range(rows)])
    assert all(len(set(r.tolist())) == V for r in x.float())
    return x


def test_oracle_equals_log_softmax_and_topk():
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        for V in (1, 2, 33, 320, 2049):
            g = torch.Generator().manual_seed(V)
            x = tie_free_rows(6, V, dtype, g)
            t = torch.randint(0, V, (6,), generator=g)
            n = 5
            lp, rank, tt, tl = L.logprobs(x, t, n)
            ref = torch.log_softmax(x.double(), -1)
            k = min(n, V)
            rv, ri = torch.topk(ref, k, dim=-1)
            assert np.array_equal(tt[:, :k], ri.numpy().astype(np.int32)) and (tt[:, k:] == -1).all() and np.isnan(tl[:, k:]).all()
            assert S.ulp_distance(tl[:, :k], rv.float().numpy()).max() <= 1
            assert S.ulp_distance(lp, ref.gather(-1, t[:, None])[:, 0].float().numpy()).max() <= 1
            assert np.array_equal(rank, (ref > ref.gather(-1, t[:, None])).sum(-1).numpy().astype(np.int32))
            nll = S.score(x, t)[0].numpy()
            assert np.array_equal(lp.view(np.int32), (-nll).view(np.int32))           # the sign-flipped nll, bit for bit


def test_oracle_order_rules_and_unread_rows():
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[1.0, 2.0, 2.0, 3.0],        # ties: the lower index first
                      [0.0, -0.0, 0.0, -0.0],      # -0 == +0: index order
                      [1.0, nan, -inf, 0.5],       # a NaN sorts as -inf: behind the numbers, index order against the -inf
                      [1.0, 2.0, 3.0, 4.0]])       # no token on this row
    lp, rank, tt, tl = L.logprobs(x, [1, 3, 0, -1], 6)
    assert tt.tolist() == [[3, 1, 2, 0, -1, -1], [0, 1, 2, 3, -1, -1], [0, 3, 1, 2, -1, -1], [-1] * 6]
    assert rank.tolist() == [1, 0, 0, -1]
    assert np.isnan(lp[2]) and np.isnan(lp[3]) and np.isnan(tl[3]).all() and np.isnan(tl[:, 4:]).all()
    assert lp[1] == np.float32(-np.log(4.0)) and tl[0, 0] == np.float32(3.0 - np.log(np.exp(1.0) + 2 * np.exp(2.0) + np.exp(3.0)))
    lp0, rank0, tt0, tl0 = L.logprobs(x, [1, 3, 0, -1], 0)
    assert tt0.shape == (4, 0) and tl0.shape == (4, 0) and np.array_equal(rank0, rank)


def test_oracle_equals_transformers_transition_scores():
    pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM
    EOS = 2
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=23, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=2, max_position_embeddings=128, bos_token_id=1, eos_token_id=EOS, pad_token_id=EOS)
    model = LlamaForCausalLM(cfg).eval()
    for seed in range(3):
        prompt = torch.randint(3, 23, (1, 5), generator=torch.Generator().manual_seed(seed))
        with torch.no_grad():
            out = model.generate(prompt, do_sample=False, max_new_tokens=8, output_scores=True, return_dict_in_generate=True,
                                 pad_token_id=EOS, eos_token_id=EOS)
        hf = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)[0]
        new = out.sequences[0, prompt.shape[1]:]
        rows = torch.stack([s[0] for s in out.scores]).float()
        lp, rank, tt, _ = L.logprobs(rows, new[:len(rows)], 1)
        # HF normalises in fp32 (log_softmax of the fp32 scores); the oracle in double, rounded once: a few fp32 ulps of the lse apart
        np.testing.assert_allclose(lp, hf[:len(rows)].numpy(), rtol=0, atol=8 * 2.0 ** -23 * max(1.0, float(rows.abs().max())))
        assert (rank == 0).all() and np.array_equal(tt[:, 0], new[:len(rows)].numpy().astype(np.int32))     # greedy: the arg-max


def test_abi_additions():
    lib = _lib.load()
    header = (Path(__file__).resolve().parents[1] / "include" / "vstar_vqa.h").read_text()
    names = ("vstar_vqa_forward_logprobs", "vstar_vqa_forward_sample_logprobs", "vstar_vqa_forward_verify_logprobs",
             "vstar_vqa_op_logprobs")
    for name in names:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTS_VQA and hasattr(lib, name), name
    assert "#define VSTAR_VQA_MAX_TOP_LOGPROBS 32" in header and _lib.MAX_TOP_LOGPROBS == 32
    assert "#define VSTAR_VQA_ABI_VERSION 1" in header
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(_lib.VqaLogprobs) == 5 * P                     # int32 n_top padded to pointer alignment, four pointers
    assert [(n, getattr(_lib.VqaLogprobs, n).offset) for n, _ in _lib.VqaLogprobs._fields_] == \
        [("n_top", 0), ("token_logprob", P), ("token_rank", 2 * P), ("top_logprob", 3 * P), ("top_token", 4 * P)]
    # the op entry refuses bad arguments before any device work (no GPU needed to get there)
    tok = np.zeros(2, np.int32)
    out = np.zeros(2, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    assert lib.vstar_vqa_op_logprobs(None, _lib.F16, 2, 8, 8, p(tok), 0, p(out), None, None, None) != 0
    assert lib.vstar_vqa_op_logprobs(p(out), _lib.F16, 2, 8, 8, p(tok), 33, p(out), None, None, None) != 0
    assert b"n_top" in lib.vstar_vqa_last_error(None)
    tok[1] = 8
    assert lib.vstar_vqa_op_logprobs(p(out), _lib.F16, 2, 8, 8, p(tok), 0, p(out), None, None, None) != 0
    assert b"token" in lib.vstar_vqa_last_error(None)


def test_python_argument_checks_fire_before_the_engine():
    from vstar_amd.api import LlavaSearchModel
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa import VQA_LLM
    from vstar_amd.vqa_engine import TokenLogprobs, check_logprobs
    cfg = VQAConfig.tiny()
    llm = VQA_LLM(cfg=cfg, engine=SimpleNamespace(cfg=cfg))             # the checks below fire before the engine is touched
    one = [dict(image=None, question="q")]
    with pytest.raises(ValueError, match="logprobs"):
        llm.free_form_batch(one, 4, logprobs=33)
    with pytest.raises(ValueError, match="logprobs"):
        llm.free_form_batch(one, 4, logprobs=-1)
    with pytest.raises(ValueError, match="logprobs"):
        llm.free_form_inference(None, "q", logprobs=-1)
    with pytest.raises(NotImplementedError, match="beam"):
        llm.free_form_batch(one, 4, num_beams=2, logprobs=1)
    # the existing cases keep their precedence and messages
    with pytest.raises(NotImplementedError, match="log-softmax"):
        llm.free_form_batch(one, 4, num_beams=2, repetition_penalty=1.2, logprobs=1)
    with pytest.raises(NotImplementedError, match="beam sampling"):
        llm.free_form_batch(one, 4, num_beams=2, temperature=0.5, logprobs=1)
    with pytest.raises(ValueError, match="speculative"):
        llm.free_form_batch(one, 4, num_beams=2, speculative=3, logprobs=1)
    model = LlavaSearchModel(llm)
    ids = torch.tensor([[1, 5, 6]])
    for n in (33, -1):
        with pytest.raises(ValueError, match="logprobs"):
            model.generate(ids, return_dict_in_generate=True, output_scores=True, top_logprobs=n)
    with pytest.raises(NotImplementedError, match="beam"):
        model.generate(ids, num_beams=2, return_dict_in_generate=True, output_scores=True)
    assert check_logprobs(None) is None and check_logprobs(0) == 0 and check_logprobs(32) == 32
    with pytest.raises(ValueError):
        check_logprobs(1.5)
    rec = TokenLogprobs.concat([], 3)
    assert rec.token_logprob.shape == (0,) and rec.top_token.shape == (0, 3) and rec.top_logprob.dtype == np.float32
