"""CPU checks of beam search: the oracle (tests/_beam_oracle.py) against installed transformers and against
hand-worked scripted cases, and the production host scorer (vstar_amd/beam.py) against the oracle."""
import math

import numpy as np
import pytest
import torch

from tests import _beam_oracle as O
from vstar_amd.beam import BeamSearch

EOS = 2


def drive(logits_fn, k, prompt_len, eos, max_new, length_penalty=1.0, early_stopping=False, num_return_sequences=1):
    """vstar_amd/beam.py fed like VQA_LLM.beam_decode feeds it, with the device select played by the oracle's candidates."""
    bs = BeamSearch(k, prompt_len, eos, prompt_len + max_new, length_penalty, early_stopping)
    while True:
        lp = O.log_probs(logits_fn([list(t) for t in bs.tokens]))
        s, t, r = O.candidates(lp, torch.from_numpy(bs.scores), 2 * k)
        bs.process(s.numpy(), t.numpy(), r.numpy())
        if bs.done or len(bs.tokens[0]) >= max_new:
            break
    return bs.finalize(num_return_sequences)


def random_fn(V, seed, eos_boost=0.0, dtype=torch.float16):
    """Deterministic logits of a history (a hash of it seeds the row)."""
    def fn(hist):
        rows = []
        for h in hist:
            g = torch.Generator().manual_seed(seed * 1000003 + hash(tuple(h)) % 1000003)
            x = torch.randn(V, generator=g) * 2
            x[EOS] += eos_boost
            rows.append(x)
        return torch.stack(rows).to(dtype)
    return fn


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("early_stopping", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [1.0, 0.0, 2.0, -0.5])
def test_scorer_equals_oracle(k, early_stopping, length_penalty):
    for seed in range(4):
        fn = random_fn(11, seed, eos_boost=1.5)
        kw = dict(length_penalty=length_penalty, early_stopping=early_stopping, num_return_sequences=min(k, 2))
        assert drive(fn, k, 7, EOS, 9, **kw) == O.beam_search(fn, k, 7, EOS, 9, **kw), (seed, kw)


def test_eos_below_rank_k_is_ignored():
    # k = 2, V = 4.  Step 1 from the start rows: row 0 = lp of [0, 1, 2, 3]; EOS (2) ranks 2nd (< k): a hypothesis.
    # Step 2: EOS ranks 3rd (>= k): skipped, the running beams take ranks 1, 2, 4.
    x1 = [[0.0, 1.0, 2.0, 3.0]] * 2
    x2 = [[5.0, 4.0, 0.0, 3.0], [0.0, 0.0, 4.5, 0.0]]
    fn = O.scripted([x1, x2])
    trace = []
    out = O.beam_search(fn, 2, 5, EOS, 2, trace=trace)
    _, _, (s, t, r) = trace[1]
    assert int(t[2]) == EOS                      # rank 2 EOS was not added: the two finished ones are rank-1 EOS and finalize's
    got = drive(O.scripted([x1, x2]), 2, 5, EOS, 2)
    assert got == out


def test_length_penalty_uses_unexpanded_length():
    # one step, k = 1: EOS at rank 0 -> a hypothesis of the prompt alone, score lp(EOS) / prompt_len ** lp
    x = [[0.0, 0.0, 3.0, 0.0]]
    bs = BeamSearch(1, 17, EOS, 17 + 4, length_penalty=1.0)
    lp = O.log_probs(torch.tensor(x))
    s, t, r = O.candidates(lp, torch.from_numpy(bs.scores), 2)
    bs.process(s.numpy(), t.numpy(), r.numpy())
    assert len(bs.hyps) == 1 and bs.hyps.beams[0][0] == pytest.approx(float(s[0]) / 17, rel=1e-12)
    assert bs.hyps.beams[0][1] == []


def test_is_done_three_modes():
    from vstar_amd.beam import BeamHypotheses
    # worst = -1.2 after two hypotheses; best -20 at cur_len 10: False mode -1.2 >= -2.0, never mode -1.2 >= -20 / 20 = -1.0
    for es, expect20, expect5 in ((True, True, True), (False, True, False), ("never", False, False)):
        h = BeamHypotheses(2, 1.0, es, max_length=20)
        h.add([5], 10, -10.0)
        assert not h.is_done(-1.0, 10)          # fewer than k hypotheses
        h.add([6], 10, -12.0)
        assert h.is_done(-20.0, 10) == expect20
        assert h.is_done(-5.0, 10) == expect5
    h = BeamHypotheses(1, 1.0, "never", max_length=100)
    h.add([1], 10, -10.0)                       # worst -1.0
    assert h.is_done(-50.0, 10) is False        # never: -50 / 100 = -0.5 > -1.0
    assert BeamHypotheses(1, 1.0, False, 100).is_done(-50.0, 10) is False


def test_finalize_unfinished_and_eos_append():
    # no EOS ever: finalize adds the running beams; the best gets EOS appended iff shorter than max_length
    fn = random_fn(6, 0, eos_boost=-50.0)
    for max_new in (1, 3):
        out = O.beam_search(fn, 2, 4, EOS, max_new)
        assert len(out[0]) == max_new and EOS not in out[0]              # length == max_length: no EOS appended
        assert drive(fn, 2, 4, EOS, max_new) == out
    # finished early (early_stopping=True): the best hypothesis is shorter than max_length and gets EOS appended
    fn = random_fn(6, 1, eos_boost=4.0)
    out = O.beam_search(fn, 2, 4, EOS, 10, early_stopping=True, num_return_sequences=2)
    assert all(o[-1] == EOS for o in out) and len(out[0]) == len(out[1])
    assert drive(fn, 2, 4, EOS, 10, early_stopping=True, num_return_sequences=2) == out


def test_tie_rule_smaller_flat_index():
    lp = torch.tensor([[-1.0, -2.0, -1.0], [-1.0, -1.0, -3.0]])
    s, t, r = O.candidates(lp, torch.zeros(2), 4)
    assert (r * 3 + t).tolist() == [0, 2, 3, 4]
    # the fp32 add collapses different lp onto one score: ties on s, not on lp
    lp = torch.tensor([[-1.0, -1.5, -2.0, -0.5]]).half()
    s, t, r = O.candidates(lp, torch.tensor([-1e9]), 2)
    assert t.tolist() == [0, 1] and s[0] == s[1]


def test_oracle_equals_transformers_generate():
    transformers = pytest.importorskip("transformers")
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=23, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                      num_key_value_heads=2, max_position_embeddings=128, bos_token_id=1, eos_token_id=EOS, pad_token_id=EOS)
    model = LlamaForCausalLM(cfg).eval()
    with torch.no_grad():
        model.lm_head.weight[EOS] *= 3.0
    mismatches = []
    for seed in range(6):
        g = torch.Generator().manual_seed(seed)
        prompt = torch.randint(3, 23, (1, 5), generator=g)
        for k in (2, 3):
            with torch.no_grad():
                hf = model.generate(prompt, num_beams=k, do_sample=False, max_new_tokens=8, length_penalty=0.0,
                                    early_stopping=False, num_return_sequences=1, pad_token_id=EOS, eos_token_id=EOS)

            def fn(hist):
                with torch.no_grad():
                    ids = torch.tensor([prompt[0].tolist() + h for h in hist])
                    return model(ids).logits[:, -1, :].float()
            ours = O.beam_search(fn, k, 5, EOS, 8, length_penalty=0.0, exact=False)
            if hf[0, 5:].tolist() != ours[0][:hf.shape[1] - 5]:
                mismatches.append((seed, k, hf[0, 5:].tolist(), ours[0]))
    assert not mismatches, f"installed transformers {transformers.__version__} differs: {mismatches}"


def test_scorer_rejects_bad_arguments():
    with pytest.raises(ValueError):
        BeamSearch(2, 5, EOS, 10, early_stopping="sometimes")
    bs = BeamSearch(2, 5, EOS, 10)
    with pytest.raises(ValueError):
        bs.process([0.0, -1.0, -2.0, -3.0], [EOS, EOS, EOS, 5], [0, 0, 0, 0])     # 4 candidates leave < 2 running beams
    with pytest.raises(ValueError):
        BeamSearch(2, 5, EOS, 10).finalize(3)
    assert math.isclose(float(BeamSearch(3, 1, EOS, 5).scores[1]), -1e9)
