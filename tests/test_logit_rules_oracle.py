"""Logits rules without a GPU: the oracle of the edit stage (tests/_logit_oracle.py) against transformers' own
logits processors, `LogitRules.plan` + the oracle edit against the chained HF classes, `LogitRules.pack` and the list check behind
vstar_vqa_op_edit on bad inputs, the ABI additions, and the failures that used to be silent.  Every test here needs a symbol or
keyword the feature adds."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _logit_oracle as O
from vstar_amd import _lib
from vstar_amd.logits import LogitRules

THETAS = (0.7, 1.05, 1.2, 1.3, 2.0, 1.0000001)
DTYPES = [torch.float16, torch.bfloat16]


def all_patterns(dtype):
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)       # wraps: every 16-bit pattern once


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_penalty_equals_transformers_on_every_bit_pattern(dtype):
    lp = pytest.importorskip("transformers").generation.logits_process
    x = all_patterns(dtype)
    ids = torch.arange(65536, dtype=torch.long)[None]
    for theta in THETAS:
        ref = lp.RepetitionPenaltyLogitsProcessor(penalty=theta)(ids, x[None].clone())[0]
        got = O.penalise(x, theta)
        assert ref.dtype == dtype and O.same_bits(got, ref), theta
        # apart from NaN payloads (same_bits) the bits themselves agree: count what the NaN rule excuses
        diff = int((got.view(torch.int16) != ref.view(torch.int16)).sum())
        assert diff <= int(torch.isnan(x).sum())
        # -0 takes the divide and stays -0; NaN stays NaN; the sign never flips
        neg0 = torch.tensor([-0.0], dtype=dtype)
        assert O.penalise(neg0, theta).view(torch.int16).item() == neg0.view(torch.int16).item()
        assert bool(torch.isnan(got[torch.isnan(x)]).all())


def _hf_chain(lp, case, dtype_scores, reverse=False):
    h, V = case["history"], case["V"]
    ids = torch.tensor([h], dtype=torch.long)
    procs = []
    if case["theta"] != 1.0:
        procs.append(lp.RepetitionPenaltyLogitsProcessor(penalty=case["theta"]))
    if case["ngram"]:
        procs.append(lp.NoRepeatNGramLogitsProcessor(case["ngram"]))
    if case["bad"]:
        procs.append(lp.NoBadWordsLogitsProcessor([list(w) for w in case["bad"]], eos_token_id=case["eos"]))
    if case["min_new"]:
        procs.append(lp.MinNewTokensLengthLogitsProcessor(len(h) - case["n_gen"], case["min_new"], case["eos"]))
    if case["allowed"] is not None:
        procs.append(lp.PrefixConstrainedLogitsProcessor(lambda b, sent: case["allowed"], 1))
    if case["suppress"]:
        procs.append(lp.SuppressTokensLogitsProcessor(case["suppress"]))
    s = dtype_scores[None].clone()
    for p in (reversed(procs) if reverse else procs):
        s = p(ids, s)
    return s[0]


def _random_case(rng):
    V = int(rng.integers(12, 51))
    L = int(rng.integers(0, 41))
    h = [int(t) for t in rng.integers(0, V, L)]
    n_gen = int(rng.integers(0, L + 1))
    eos = int(rng.integers(0, V))
    bad = []
    if rng.random() < 0.6:
        singles = [t for t in rng.integers(0, V, int(rng.integers(1, 4))).tolist() if t != eos] or [(eos + 1) % V]
        bad += [[int(t)] for t in singles]
        if rng.random() < 0.3:
            bad.append([eos])                                            # HF filters [eos] out of the bad words
        for _ in range(int(rng.integers(0, 4))):                         # multi-token words: half of them end where the history ends
            m = int(rng.integers(2, 4))
            if L >= m - 1 and rng.random() < 0.5:
                bad.append(h[L - (m - 1):] + [int(rng.integers(0, V))])
            else:
                bad.append([int(t) for t in rng.integers(0, V, m)])
    allowed = None
    if rng.random() < 0.4:
        allowed = sorted(set(int(t) for t in rng.integers(0, V, int(rng.integers(1, 8)))))
    return dict(V=V, history=h, n_gen=n_gen, eos=eos, theta=float(rng.choice(THETAS)) if rng.random() < 0.6 else 1.0,
                ngram=int(rng.integers(0, 4)), bad=bad, min_new=int(rng.integers(0, 6)) if rng.random() < 0.5 else 0,
                suppress=sorted(set(int(t) for t in rng.integers(0, V, int(rng.integers(0, 4))))) if rng.random() < 0.4 else [],
                allowed=allowed)


def test_plan_and_oracle_edit_equal_the_chained_hf_classes():
    lp = pytest.importorskip("transformers").generation.logits_process
    rng = np.random.default_rng(20240607)
    n_cases, counts = 240, dict(pen=0, ban=0, allow=0)
    for c in range(n_cases):
        case = _random_case(rng)
        rules = LogitRules(case["theta"], case["ngram"], case["bad"] or None, case["min_new"], case["suppress"] or None,
                           (lambda b, hist: case["allowed"]) if case["allowed"] is not None else None)
        got_plan = rules.plan(case["history"], case["n_gen"], case["eos"])
        ora_plan = O.plan(case["history"], case["n_gen"], case["eos"], repetition_penalty=case["theta"], no_repeat_ngram_size=case["ngram"],
                          bad_words_ids=case["bad"], min_new_tokens=case["min_new"], suppress_tokens=case["suppress"],
                          allowed_tokens_fn=(lambda b, hist: case["allowed"]) if case["allowed"] is not None else None)
        assert got_plan == ora_plan, case
        for key, lst in zip(("pen", "ban", "allow"), (got_plan[0], got_plan[2], got_plan[3])):
            counts[key] += bool(lst)
            assert lst == sorted(set(lst)) and all(0 <= t < case["V"] for t in lst)
        x32 = torch.from_numpy(rng.standard_normal(case["V"]).astype(np.float32) * 3)
        for dtype in DTYPES:
            x = x32.to(dtype)
            got = O.edit_row(x, *got_plan)
            ref = _hf_chain(lp, case, x)
            assert got.dtype == ref.dtype == dtype
            assert (got.view(torch.int16) == ref.view(torch.int16)).all(), (case, got_plan)
            if c % 4 == 0:                                               # the order of HF's list does not change the result
                assert (got.view(torch.int16) == _hf_chain(lp, case, x, reverse=True).view(torch.int16)).all(), case
        # pack -> the same lists back
        off, tok, pen = LogitRules.pack([got_plan, ([], 1.0, [], []), got_plan])
        assert off[0] == 0 and off[3] == off[6] and (np.diff(off) >= 0).all() and pen[0] == np.float32(case["theta"])
        assert [tok[off[i]:off[i + 1]].tolist() for i in range(3)] == [got_plan[0], got_plan[2], got_plan[3]]
        assert tok[off[6]:].tolist() == tok[:off[3]].tolist()
    assert all(v >= 0.2 * n_cases for v in counts.values()), counts


def test_history_leaves_placeholders_out_and_empty_allow_list_raises():
    r = LogitRules(repetition_penalty=1.3, no_repeat_ngram_size=2)
    # <image> (-200) between 7 and 9: no token, 7 and 9 are adjacent
    pen, theta, ban, allow = r.plan([5, 7, -200, 9, 4, 7], 0, 2)
    assert pen == [4, 5, 7, 9] and theta == 1.3 and ban == [9] and allow == []
    assert O.plan([5, 7, -200, 9, 4, 7], 0, 2, repetition_penalty=1.3, no_repeat_ngram_size=2) == (pen, theta, ban, allow)
    with pytest.raises(ValueError):
        LogitRules(allowed_tokens_fn=lambda b, h: []).plan([1, 2], 0, 2)
    assert not LogitRules().active and LogitRules(min_new_tokens=1).active
    for kw in (dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(min_new_tokens=-2), dict(bad_words_ids=[]),
               dict(bad_words_ids=[[]]), dict(bad_words_ids=[[3, -1]])):
        with pytest.raises(ValueError):
            LogitRules(**kw)


def _op_edit_rc(lib, rows, vocab, off, tok, pen):
    """vstar_vqa_op_edit on a pointer that is never dereferenced: the lists are checked before any device work."""
    off, tok = np.ascontiguousarray(off, np.int32), np.ascontiguousarray(tok, np.int32)
    pen = np.ascontiguousarray(pen, np.float32)
    fake = np.zeros(16, np.uint16)
    rc = lib.vstar_vqa_op_edit(ctypes.c_void_p(fake.ctypes.data), _lib.F16, rows, vocab, vocab, ctypes.c_void_p(off.ctypes.data),
                               ctypes.c_void_p(tok.ctypes.data) if tok.size else None, ctypes.c_void_p(pen.ctypes.data))
    return rc, (lib.vstar_vqa_last_error(None) or b"").decode()


def test_pack_and_edit_check_on_bad_inputs(lib):
    # pack sorts and de-duplicates hand-made plans
    off, tok, pen = LogitRules.pack([([5, 3, 5], 1.2, [9, 0], []), ([], 1.0, [], [7, 7, 1])])
    assert off.tolist() == [0, 2, 4, 4, 4, 4, 6] and tok.tolist() == [3, 5, 0, 9, 1, 7] and pen.tolist() == [np.float32(1.2), 1.0]
    assert off.dtype == tok.dtype == np.int32 and pen.dtype == np.float32
    V = 10
    bad = {
        "a decreasing offset": ([0, 2, 1, 1], [3, 5], [1.2], "must not decrease"),
        "a repeated id": ([0, 2, 2, 2], [3, 3], [1.2], "strictly increasing"),
        "a decreasing id": ([0, 0, 2, 2], [5, 3], [1.2], "strictly increasing"),
        "an id equal to vocab": ([0, 0, 0, 1], [V], [1.2], "outside [0, vocab)"),
        "a negative id": ([0, 0, 1, 1], [-1], [1.2], "outside [0, vocab)"),
        "theta = 0": ([0, 1, 1, 1], [3], [0.0], "finite and > 0"),
        "theta = NaN": ([0, 1, 1, 1], [3], [float("nan")], "finite and > 0"),
        "theta = inf": ([0, 1, 1, 1], [3], [float("inf")], "finite and > 0"),
        "off[0] != 0": ([1, 2, 2, 2], [3, 5], [1.2], "off[0] must be 0"),
    }
    for name, (off, tok, pen, msg) in bad.items():
        rc, err = _op_edit_rc(lib, 1, V, off, tok, pen)
        assert rc == -1 and msg in err, (name, rc, err)
    # theta is not read where nothing is penalised: a bad theta on a ban-only row passes the check (and then needs a device)
    if not torch.cuda.is_available():
        rc, err = _op_edit_rc(lib, 1, V, [0, 0, 1, 1], [3], [0.0])
        assert rc != 0 and "vstar_vqa_op_edit" in err and "finite" not in err


def test_abi_struct_and_exports(lib):
    assert ctypes.sizeof(_lib.VqaLogitEdits) == 3 * ctypes.sizeof(ctypes.c_void_p)
    assert [(_n, getattr(_lib.VqaLogitEdits, _n).offset) for _n, _ in _lib.VqaLogitEdits._fields_] == \
        [("off", 0), ("tok", ctypes.sizeof(ctypes.c_void_p)), ("penalty", 2 * ctypes.sizeof(ctypes.c_void_p))]
    for name in ("vstar_vqa_forward_edits", "vstar_vqa_forward_sample_edits", "vstar_vqa_forward_verify_edits", "vstar_vqa_op_edit",
                 "vstar_vqa_logit_edit_capacity"):
        assert name in _lib.EXPORTS_VQA and hasattr(lib, name), name
    assert lib.vstar_vqa_logit_edit_capacity(None) == 0


def test_rules_fail_loudly_where_they_used_to_vanish():
    from vstar_amd.api import LlavaSearchModel
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa import VQA_LLM
    cfg = VQAConfig.tiny()
    llm = VQA_LLM(cfg=cfg, engine=SimpleNamespace(cfg=cfg))             # the checks below fire before the engine is touched
    with pytest.raises(NotImplementedError, match="log-softmax"):
        llm.free_form_batch([dict(image=None, question="q")], 4, num_beams=2, repetition_penalty=1.2)
    with pytest.raises(NotImplementedError, match="log-softmax"):
        llm.free_form_inference(None, "q", num_beams=3, no_repeat_ngram_size=2)
    model = LlavaSearchModel(llm)
    ids = torch.tensor([[1, 5, 6]])
    with pytest.raises(ValueError, match="repetition_penalty"):
        model.generate(ids, repetition_penalty=0)
    with pytest.raises(NotImplementedError, match="log-softmax"):
        model.generate(ids, num_beams=2, suppress_tokens=[4])
    with pytest.raises(ValueError):
        llm.free_form_batch([dict(image=None, question="q")], 4, min_new_tokens=-1)
