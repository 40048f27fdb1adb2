"""Contrastive search on the MI355X (csrc/contrast.hip): the op against the CPU oracle (tests/_contrast_oracle.py)
with derived tolerances; the engine's begin call against the reference algorithm's final-norm hidden states; every decode step against
the checks derived from what it read; alpha = 0 against the greedy decode; the adopted K/V rows against a yardstick slot, bit for bit;
a ragged batch against solo runs; and the calls that do not ask, which must not move.  Every test here needs a symbol the feature adds.

THE PENALTY BOUND.  For 16-bit rows a, b of H elements every product a_i b_i is exact in fp32, so the fp32 dot product d~ of the
kernel differs from the exact d by at most (first order) H u sum |a_i b_i| <= H u |a| |b| with u = 2^-24, whatever the (fixed)
summation order: H u in units of the cosine.  Each squared norm has relative error <= H u, its square root H u / 2, the two norms
together H u.  The roundings of the two square roots, the two divisions and the two multiplies add <= 6 u, and |cos| <= 1 + O(u).  So
|pen - oracle| <= (2 H + 16) 2^-24, the 16 leaving room for the second-order terms; the max over positions does not widen it."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import vqa_oracle as O
from tests import _contrast_oracle as C
from tests import _score_oracle as S
from tests.test_logprob_gpu import op_logprobs
from tests.test_vqa_gpu import rel_l2
from tests.test_vqa_oracle import load_case
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.vqa import VQA_LLM
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu


def pen_bound(hidden):
    return (2 * hidden + 16) * 2.0 ** -24


# ------------------------------------------------ the op ------------------------------------------------
def op_case(dtype, hidden, hist_lens, group_rows, vocab, seed, planted=False):
    """Host tensors of one op call: n groups with hist_lens[g] history rows and group_rows[g] candidates.  The history buffer is
    [n, cap, hidden] with cap = max(hist_lens) + 3, sentinel rows behind every group's history; logits [rows, vocab + 5] with NaN in
    the padding columns.  planted (groups of >= 5 rows, hist_len >= 2): candidate 0 duplicates a history row (cosine 1), 1 is the
    negation of another (its -1 never is the max), 2 is a zero row (cosine 0), 3 and 4 are equal rows with equal probabilities (a
    tie: the lower index), and the probabilities are spread so that every group's pick has a wide margin."""
    g = torch.Generator().manual_seed(seed)
    n, rows, cap = len(hist_lens), sum(group_rows), max(hist_lens) + 3
    hist = torch.randn(n, cap, hidden, generator=g).to(dtype)
    hist[0, 0] *= 37.0                                               # rows of very different norms
    cand = torch.randn(rows, hidden, generator=g).to(dtype)
    goff = np.concatenate([[0], np.cumsum(group_rows)]).astype(np.int32)
    prob = torch.rand(rows, generator=g).float().numpy()
    if planted:
        spreads = ([0.30, 0.45, 0.60, 0.95, 0.95], [0.95, 0.30, 0.15, 0.45, 0.45], [0.10, 0.35, 0.95, 0.55, 0.55])
        for gi in range(n):
            r0, L = int(goff[gi]), hist_lens[gi]
            cand[r0] = hist[gi, L // 2]
            cand[r0 + 1] = -hist[gi, L - 1]
            cand[r0 + 2] = 0
            cand[r0 + 4] = cand[r0 + 3]
            prob[r0:r0 + 5] = spreads[gi % 3]
            prob[r0 + 5:r0 + group_rows[gi]] *= 0.05                  # the rest of a larger group stays out of the contest
    x = torch.full((rows, vocab + 5), float("nan"))
    x[:, :vocab] = torch.randn(rows, vocab, generator=g) * 3
    return dict(dtype=dtype, hidden=hidden, hist_lens=list(hist_lens), goff=goff, cand=cand, hist=hist, prob=prob.astype(np.float32),
                logits=x.to(dtype), vocab=vocab, cap=cap)


def case_rnorm(case):
    """The reciprocal norms the kernels keep for the case's history rows (the oracle's bit-exact restatement); sentinel 7 behind."""
    rn = np.full(case["hist"].shape[:2], 7.0, np.float32)
    for gi, L in enumerate(case["hist_lens"]):
        if L > 0:                                                      # (the refused cases pass a hist_len of 0)
            rn[gi, :L] = C.rnorm32(case["hist"][gi, :L].float().numpy())
    return rn


def op_contrast(lib, case, alpha, k, cuda):
    """vstar_vqa_op_contrast on a copy of the case -> dict(sel, tok, prob, pen, hist, rn): the outputs and the history afterwards."""
    dt = _lib.F16 if case["dtype"] == torch.float16 else _lib.BF16
    xd, cd, hd = case["logits"].to(cuda), case["cand"].to(cuda), case["hist"].to(cuda)
    rn0 = case_rnorm(case)
    rd = torch.from_numpy(rn0).to(cuda)
    rows, n = len(case["prob"]), len(case["hist_lens"])
    hl = np.asarray(case["hist_lens"], np.int32)
    sel, tok, pb, pen = np.empty(n, np.int32), np.empty((n, k), np.int32), np.empty((n, k), np.float32), np.empty(rows, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)      # noqa: E731
    d = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    _lib.check_vqa(lib.vstar_vqa_op_contrast(d(xd), dt, rows, case["vocab"], xd.shape[1], d(cd), case["hidden"], d(hd), d(rd), n, case["cap"],
                                             p(hl), p(case["goff"]), p(case["prob"]), alpha, k, p(sel), p(tok), p(pb), p(pen)))
    return dict(sel=sel, tok=tok, prob=pb, pen=pen, hist=hd.cpu(), rn=rd.cpu().numpy(), rn0=rn0)


def oracle_step(case):
    """The float64 penalties of every candidate row of the case."""
    pen = np.empty(len(case["prob"]), np.float64)
    for gi, L in enumerate(case["hist_lens"]):
        r0, r1 = case["goff"][gi], case["goff"][gi + 1]
        pen[r0:r1] = C.penalty(case["cand"][r0:r1].double().numpy(), case["hist"][gi, :L].double().numpy())
    return pen


def planted_gap(case, pen64, alpha):
    """Per group: (the oracle's pick, its score margin over the best candidate that is not an exact duplicate of it)."""
    out = []
    for gi in range(len(case["hist_lens"])):
        r0, r1 = case["goff"][gi], case["goff"][gi + 1]
        s, score = C.score_select(case["prob"][r0:r1], pen64[r0:r1], alpha)
        cb = case["cand"][r0:r1].view(torch.int16)
        others = [c for c in range(r1 - r0) if not (torch.equal(cb[c], cb[s]) and case["prob"][r0 + c] == case["prob"][r0 + s])]
        out.append((s, float(score[s] - max(score[c] for c in others)) if others else np.inf))
    return out


def check_op(case, got, alpha, k, pen64, what):
    """The derived checks of one op call against the oracle."""
    H = case["hidden"]
    bits = lambda t: t.view(torch.int16)              # noqa: E731
    err = np.abs(got["pen"].astype(np.float64) - pen64).max()
    print(f"contrast op {what}: max |pen - oracle| = {err:.3e} (bound {pen_bound(H):.3e})")
    assert err <= pen_bound(H), (what, err)
    for gi, L in enumerate(case["hist_lens"]):
        r0, r1 = case["goff"][gi], case["goff"][gi + 1]
        s = int(got["sel"][gi])
        assert s == C.score_select(case["prob"][r0:r1], got["pen"][r0:r1], alpha)[0], (what, gi)       # the exact double recomputation
        tok, pb = C.topk_probs(case["logits"][r0 + s, :case["vocab"]].double().numpy(), k)
        assert np.array_equal(got["tok"][gi], tok), (what, gi)
        assert S.ulp_distance(got["prob"][gi], pb).max() <= 1, (what, gi)
        # the appended row and reciprocal norm are exact, nothing else of the history is written
        assert torch.equal(bits(got["hist"][gi, L]), bits(case["cand"][r0 + s])), (what, gi)
        assert got["rn"][gi, L].view(np.int32) == np.asarray(C.rnorm32(case["cand"][r0 + s].float().numpy())).view(np.int32), (what, gi)
        keep = torch.ones(case["cap"], dtype=torch.bool)
        keep[L] = False
        assert torch.equal(bits(got["hist"][gi][keep]), bits(case["hist"][gi][keep])), (what, gi)
        assert np.array_equal(got["rn"][gi][keep.numpy()].view(np.int32), got["rn0"][gi][keep.numpy()].view(np.int32)), (what, gi)


OP_CASES = [   # (hidden, hist_lens, group_rows, vocab): every hidden, hist_len, group size, group count and vocab of the contract
    (8, (1,), (1,), 32),
    (8, (65, 1, 257), (2, 5, 32), 320),
    (256, (63,), (2,), 320),
    (256, (64, 65, 1025), (32, 1, 5), 32),
    (4096, (257,), (5,), 32003),
    (4096, (1, 63, 64), (1, 32, 2), 320),
    (5120, (1025,), (32,), 32),
    (5120, (65, 257, 63), (5, 2, 1), 32003),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hidden,hist_lens,group_rows,vocab", OP_CASES, ids=[f"H{c[0]}-L{'_'.join(map(str, c[1]))}-m{'_'.join(map(str, c[2]))}-V{c[3]}" for c in OP_CASES])
def test_op_against_oracle(cuda, lib, dtype, hidden, hist_lens, group_rows, vocab):
    case = op_case(dtype, hidden, hist_lens, group_rows, vocab, seed=hidden + vocab)
    pen64 = oracle_step(case)
    for alpha, k in ((0.6, 4), (0.0, 2), (1.0, min(32, vocab))):
        got = op_contrast(lib, case, alpha, k, cuda)
        check_op(case, got, alpha, k, pen64, (str(dtype), hidden, hist_lens, alpha, k))
    again = op_contrast(lib, case, alpha, k, cuda)                   # two runs: identical bits
    for key in ("sel", "tok", "prob", "pen", "rn"):
        assert np.array_equal(got[key].view(np.int32), again[key].view(np.int32)), key
    assert torch.equal(got["hist"].view(torch.int16), again["hist"].view(torch.int16))


PLANTED = [(8, (2, 65, 1025), (5, 5, 7)), (256, (257, 64, 2), (5, 32, 5)), (4096, (63, 1025, 65), (6, 5, 5)), (5120, (257,), (5,))]


def planted_case(dtype, hidden, hist_lens, group_rows):
    return op_case(dtype, hidden, hist_lens, group_rows, 320, seed=3 * hidden + 1, planted=True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hidden,hist_lens,group_rows", PLANTED, ids=[f"H{c[0]}" for c in PLANTED])
def test_op_planted_margins(cuda, lib, dtype, hidden, hist_lens, group_rows):
    case = planted_case(dtype, hidden, hist_lens, group_rows)
    pen64 = oracle_step(case)
    alpha, k = 0.5, 4
    gaps = planted_gap(case, pen64, alpha)
    # the oracle alone first: the planted penalties are what they were planted as, and every pick has >= 10 x the bound of margin
    for gi in range(len(hist_lens)):
        r0 = case["goff"][gi]
        assert abs(pen64[r0] - 1.0) < 1e-12 and pen64[r0 + 2] == 0.0 and pen64[r0 + 3] == pen64[r0 + 4], gi
        assert gaps[gi][1] >= 10 * pen_bound(hidden), (gi, gaps[gi])
    assert len({s for s, _ in gaps}) > 1 or len(hist_lens) == 1       # the groups do not all pick the same candidate
    got = op_contrast(lib, case, alpha, k, cuda)
    check_op(case, got, alpha, k, pen64, ("planted", str(dtype), hidden))
    assert got["sel"].tolist() == [s for s, _ in gaps]
    for gi in range(len(hist_lens)):
        r0 = case["goff"][gi]
        assert got["pen"][r0 + 2] == 0.0                              # a zero-norm row: cosine 0, not NaN
        assert got["pen"][r0 + 3].view(np.int32) == got["pen"][r0 + 4].view(np.int32)      # equal rows: equal bits


def test_op_refuses_bad_arguments_and_stays_usable(cuda, lib):
    case = op_case(torch.float16, 256, (65,), (5,), 320, seed=5)
    ok = op_contrast(lib, case, 0.5, 4, cuda)
    for change, word in ((dict(hist_lens=[0]), "hist_len"), (dict(hist_lens=[case["cap"]]), "hist_len"), (dict(hidden=252), "hidden"),
                         (dict(prob=np.full(5, 2.0, np.float32)), "cand_prob"), (dict(goff=np.asarray([0, 4], np.int32)), "group_off")):
        with pytest.raises(_lib.VstarError, match=word):
            op_contrast(lib, dict(case, **change), 0.5, 4, cuda)
    for alpha, k, word in ((1.5, 4, "alpha"), (0.5, 1, "k_next"), (0.5, 33, "k_next")):
        with pytest.raises(_lib.VstarError, match=word):
            op_contrast(lib, case, alpha, k, cuda)
    again = op_contrast(lib, case, 0.5, 4, cuda)
    assert all(np.array_equal(ok[key].view(np.int32), again[key].view(np.int32)) for key in ("sel", "tok", "prob", "pen"))


# ------------------------------------------------ the engine ------------------------------------------------
_ENGINES = {}
GOLDEN_PLAIN = os.path.join(os.path.dirname(__file__), "golden", "vqa_tiny_plain.npz")


def _engine(kind="tiny"):
    """tiny: VQAConfig.tiny(max_slots=16); kv8: the same with kv_cache_format = 1; weights of seed 0."""
    if kind not in _ENGINES:
        cfg = VQAConfig.tiny(max_slots=16)
        cfg = cfg.with_kv_bits(8) if kind == "kv8" else cfg
        assert cfg.kv_cache_format == (1 if kind == "kv8" else 0)
        eng = VqaEngine(cfg, 0)
        eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
        _ENGINES[kind] = (eng, cfg)
    return _ENGINES[kind]


def _text_prompt(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [1] + torch.randint(3, 300, (n - 1,), generator=g).tolist()


def test_begin_fills_the_history_and_returns_the_top_k(cuda, lib):
    z, cfg0, pix, ids, opts, n_obj, il, ol = load_case(GOLDEN_PLAIN)
    eng, cfg = _engine()
    assert dataclasses.replace(cfg0, max_slots=16) == cfg         # (the golden file's prompt; the weights are this engine's, seed 0)
    H = cfg.llm_hidden

    def ref_hidden(dtype):          # oracle/vqa_oracle.py's final-norm hidden states: its forward with an identity lm_head
        sd = random_state_dict(cfg, 0, dtype)
        lo, sh = O.encode_images(sd, cfg, pix.to(dtype))
        emb = O.splice(sd, ids, lo[:1], sh[:1], lo[1:], sh[1:], il, ol)
        return O.llama_forward(dict(sd, **{"lm_head.weight": torch.eye(H, dtype=dtype)}), cfg, emb)[0].float().numpy()

    gold, h16 = ref_hidden(torch.float32), ref_hidden(torch.float16)
    eng.encode_images(pix, 0)
    rows = eng.expand_ids(ids, [0], list(range(1, 1 + n_obj)), il, ol)
    k = 8
    tok, prob = eng.forward_contrast_begin([Seq(rows, kv_slot=3)], [(0, -1)], k)
    hist = eng.contrast_hist(3)
    assert hist.shape == gold.shape == (len(rows), H)
    per_row = [(rel_l2(hist[j], gold[j]), rel_l2(h16[j], gold[j])) for j in range(len(rows))]
    print("contrast begin: history rel_l2 %.2e (noise %.2e); worst position %.2e (its noise %.2e)" %
          ((rel_l2(hist, gold), rel_l2(h16, gold)) + max(per_row)))
    assert rel_l2(hist, gold) <= max(5e-3, 3 * rel_l2(h16, gold))
    for j, (err, noise) in enumerate(per_row):
        assert err <= max(5e-3, 3 * noise), (j, err, noise)
    # the next candidates are the top-n of the logprob op on the logits row of the same rows
    lg, am = eng.forward([Seq(rows, kv_slot=4)], [(0, -1)])
    rec = op_logprobs(lib, torch.from_numpy(lg).to(cuda), am, k)
    assert np.array_equal(tok, rec.top_token) and tok[0, 0] == am[0]
    # p = float32(exp(x - lse)) against top_logprob = float32(x - lse): the rounding of the latter is <= 2^-24 |lp| in the exponent
    lp = rec.top_logprob.astype(np.float64)
    assert (np.abs(prob.astype(np.float64) - np.exp(lp)) <= 2.0 ** -23 * (1.0 + np.abs(lp)) * np.exp(lp)).all()
    tk, pk = C.topk_probs(lg[0].astype(np.float64), k)
    assert np.array_equal(tok[0], tk) and S.ulp_distance(prob[0], pk).max() <= 1
    # a chunked prefill continues the history; any other past_len is refused
    half = len(rows) // 2
    eng.forward_contrast_begin([Seq(rows[:half], kv_slot=5)], [(0, -1)], k)
    with pytest.raises(_lib.VstarError, match="past_len"):
        eng.forward_contrast_begin([Seq(rows[half:], kv_slot=5, past_len=half - 1)], [(0, -1)], k)
    tok2, prob2 = eng.forward_contrast_begin([Seq(rows[half:], kv_slot=5, past_len=half)], [(0, -1)], k)
    h5 = eng.contrast_hist(5)
    assert h5.shape == hist.shape and rel_l2(h5, gold) <= max(5e-3, 3 * rel_l2(h16, gold))


def _step_seqs(cand_tok, owner, k, pos):
    return [Seq([int(cand_tok[c])], kv_slot=owner + c, past_len=pos, prefix_slot=owner) for c in range(k)]


@pytest.mark.parametrize("kind", ["tiny", "kv8"])
def test_decode_is_self_consistent_at_every_step(cuda, lib, kind):
    eng, cfg = _engine(kind)
    H, k, alpha, owner = cfg.llm_hidden, 5, 0.6, 4
    rows = _text_prompt(23, 41)
    tok, prob = eng.forward_contrast_begin([Seq(rows, kv_slot=owner)], [(0, -1)], k)
    ct, cp, pos, sels = tok[0].copy(), prob[0].copy(), len(rows), []
    for step in range(6):
        before = eng.contrast_hist(owner)
        assert before.shape == (pos, H)
        seqs = _step_seqs(ct, owner, k, pos)
        lg, _ = eng.forward(seqs, [(c, 0) for c in range(k)])        # the identical k rows by the plain path: the step's logits
        sel, ntok, nprob, pen = eng.forward_contrast_step(seqs, [0, k], cp, alpha, k, penalties=True)
        cand, after = eng.contrast_cand(), eng.contrast_hist(owner)
        assert cand.shape == (k, H) and after.shape == (pos + 1, H)
        err = np.abs(pen.astype(np.float64) - C.penalty(cand, before)).max()
        assert err <= pen_bound(H), (step, err)
        s = int(sel[0])
        assert s == C.score_select(cp, pen, alpha)[0], step
        tk, pk = C.topk_probs(lg[s].astype(np.float64), k)
        assert np.array_equal(ntok[0], tk) and S.ulp_distance(nprob[0], pk).max() <= 1, step
        assert np.array_equal(after[:pos], before) and np.array_equal(after[pos], cand[s]), step
        sels.append(s)
        ct, cp, pos = ntok[0].copy(), nprob[0].copy(), pos + 1
    print(f"contrast decode ({kind}): picks {sels}")


@pytest.mark.parametrize("k", [2, 8])
def test_alpha_zero_is_the_greedy_decode(cuda, k):
    eng, cfg = _engine()
    llm = VQA_LLM(cfg=cfg, engine=eng)
    rows = _text_prompt(31, 43)
    ref = llm.greedy_decode([Seq(rows, kv_slot=0)], [len(rows)], 24)
    got = llm.contrastive_decode([Seq(rows, kv_slot=8)], [len(rows)], 24, 0.0, k)
    assert got == ref and len(ref[0]) == 24


@pytest.mark.parametrize("kind", ["tiny", "kv8"])
def test_adopted_rows_equal_a_yardstick_slot_bit_for_bit(cuda, kind):
    eng, cfg = _engine(kind)
    k, alpha, owner, yard, T = 4, 0.9, 4, 12, 10
    rows = _text_prompt(19, 47)
    tok, prob = eng.forward_contrast_begin([Seq(rows, kv_slot=owner)], [(0, -1)], k)
    ct, cp, pos, out, sels = tok[0].copy(), prob[0].copy(), len(rows), [], []
    for _ in range(T):
        sel, ntok, nprob = eng.forward_contrast_step(_step_seqs(ct, owner, k, pos), [0, k], cp, alpha, k)
        out.append(int(ct[int(sel[0])]))
        sels.append(int(sel[0]))
        ct, cp, pos = ntok[0].copy(), nprob[0].copy(), pos + 1
    assert any(s != 0 for s in sels), sels                            # a winner outside the owner slot: its K/V row was copied
    eng.forward([Seq(rows, kv_slot=yard)], [])
    for t, x in enumerate(out):
        eng.forward([Seq([x], kv_slot=yard, past_len=len(rows) + t)], [])
    probe = 7
    a, _ = eng.forward([Seq([probe], kv_slot=owner, past_len=pos)], [(0, 0)])
    b, _ = eng.forward([Seq([probe], kv_slot=yard, past_len=pos)], [(0, 0)])
    assert np.array_equal(a.view(np.int16), b.view(np.int16))
    for layer in range(cfg.llm_layers):
        assert np.array_equal(eng.kv_rows(layer, owner)[:, :, :pos], eng.kv_rows(layer, yard)[:, :, :pos]), layer


def test_batch_equals_solo_runs(cuda):
    eng, cfg = _engine()
    llm = VQA_LLM(cfg=cfg, engine=eng)
    k, alpha, T = 4, 0.6, 12
    prompts = [_text_prompt(n, 50 + n) for n in (9, 27, 16)]
    free = [llm.contrastive_decode([Seq(p, kv_slot=0)], [len(p)], T, alpha, k)[0] for p in prompts]
    llm.eos_token_id = free[1][3]                                     # sample 1 now ends early, on its fourth token at the latest
    solo = [llm.contrastive_decode([Seq(p, kv_slot=0)], [len(p)], T, alpha, k)[0] for p in prompts]
    assert len(solo[1]) <= 4 and solo[1][-1] == llm.eos_token_id and max(len(s) for s in solo) == T
    both = llm.contrastive_decode([Seq(p, kv_slot=i * k) for i, p in enumerate(prompts)], [len(p) for p in prompts], T, alpha, k)
    assert both == solo
    with pytest.raises(ValueError, match="KV slots"):
        llm.contrastive_decode([Seq(p, kv_slot=i * k) for i, p in enumerate(prompts * 2)], [len(p) for p in prompts * 2], T, alpha, k)


def test_stale_history_and_broken_rules_are_refused(cuda):
    eng, cfg = _engine()
    k, owner = 4, 4
    rows = _text_prompt(15, 61)
    P = len(rows)
    tok, prob = eng.forward_contrast_begin([Seq(rows, kv_slot=owner)], [(0, -1)], k)
    seqs = _step_seqs(tok[0], owner, k, P)
    eng.forward([Seq([5], kv_slot=owner, past_len=P - 2)], [])        # a plain forward that rewinds the owner
    with pytest.raises(_lib.VstarError, match="history"):
        eng.forward_contrast_step(seqs, [0, k], prob[0], 0.5, k)
    assert eng.contrast_hist(owner).shape[0] == P - 2
    tok, prob = eng.forward_contrast_begin([Seq(rows, kv_slot=owner)], [(0, -1)], k)
    for bad, kw, word in (([Seq(s.rows, s.kv_slot, P - 1, owner) for s in seqs], {}, "past_len"),
                          ([Seq(s.rows, owner + 1, P, owner) for s in seqs], {}, "kv_slot"),
                          ([Seq(s.rows, s.kv_slot, P, owner if i else owner + 1) for i, s in enumerate(seqs)], {}, "prefix_slot"),
                          (seqs, dict(alpha=-0.5), "alpha"), (seqs, dict(prob=[0.5, 0.5, 0.5, float("inf")]), "cand_prob"),
                          (seqs, dict(goff=[0, 2]), "group_off"), (seqs, dict(k=1), "k_next")):
        with pytest.raises(_lib.VstarError, match=word):
            eng.forward_contrast_step(bad, kw.get("goff", [0, k]), kw.get("prob", prob[0]), kw.get("alpha", 0.5), kw.get("k", k))
    sel, ntok, nprob = eng.forward_contrast_step(seqs, [0, k], prob[0], 0.5, k)      # the engine stays usable
    assert 0 <= sel[0] < k and eng.contrast_hist(owner).shape[0] == P + 1


def test_an_engine_that_never_asks_is_untouched(cuda):
    cfg = VQAConfig.tiny()
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
    rows = _text_prompt(12, 71)
    lg, am = eng.forward([Seq(rows, kv_slot=0)], [(0, -1)])
    assert np.isfinite(lg.astype(np.float32)).all() and am[0] == int(lg[0].astype(np.float32).argmax())
    with pytest.raises(_lib.VstarError, match="no contrast call"):
        eng.debug_read("contrast_hist:0", 16)
    other, cfg16 = _engine()
    ref, _ = other.forward([Seq(rows, kv_slot=9)], [(0, -1)])         # an engine that ran contrast calls gives the same plain logits
    assert np.array_equal(lg.view(np.int16), ref.view(np.int16))
