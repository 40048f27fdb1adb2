"""Speculative decoding on the MI355X (csrc/spec.hip): the verify op against the CPU oracle
(tests/_spec_oracle.py), the engine tail against the op, `VQA_LLM.speculative_decode` against a host loop over the same engine
calls, and the public keywords.  Every test here needs symbols or keywords this feature adds."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sampling_oracle as S
from tests import _spec_oracle as O
from tests.test_sampling_gpu import KINDS, U_EPS, make_row, op_sample
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.spec import ReplayDrafter, no_draft
from vstar_amd.vqa import VQA_LLM, sampling_params
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu


def op_verify(lib, x_dev, groups, draft, params=None, vocab=None):
    rows, ld = x_dev.shape
    go, dr = np.ascontiguousarray(groups, np.int32), np.ascontiguousarray(draft, np.int32)
    acc, tok = np.empty(len(go) - 1, np.int32), np.empty(rows, np.int32)
    prm = (_lib.VqaSampling * rows)(*params) if params is not None else None
    dt = _lib.F16 if x_dev.dtype == torch.float16 else _lib.BF16
    _lib.check_vqa(lib.vstar_vqa_op_verify(ctypes.c_void_p(x_dev.data_ptr()), dt, rows, ld if vocab is None else vocab, ld,
                                           ctypes.c_void_p(go.ctypes.data), len(go) - 1, ctypes.c_void_p(dr.ctypes.data),
                                           ctypes.cast(prm, ctypes.c_void_p) if prm is not None else None,
                                           ctypes.c_void_p(acc.ctypes.data), ctypes.c_void_p(tok.ctypes.data)))
    return acc, tok


SIZES = (1, 2, 7, 16, 16, 7, 2, 1, 7)           # rows of the groups of one call (several groups, 59 rows)
PATTERNS = ("right", "wrong0", "wrong_mid", "wrong_last")


def _rows_for(V, g, dtype, n):
    rows = []
    for r in range(n):
        kind = KINDS[r % 4]
        x = make_row(kind, V, g, dtype)
        if r % 11 == 5 and V > 2:               # tied maxima
            x[[1, V // 2, V - 1]] = x.float().max().to(dtype) if torch.isfinite(x.float().max()) else x[0]
        if r % 13 == 7 and V > 2:               # NaNs in the row
            x[::3] = float("nan")
        rows.append(x)
    return rows


def _drafts(right, sizes, V):
    """right[r]: the token that would be accepted on row r.  Per group one of the four patterns."""
    draft, r0 = [], 0
    for gi, m in enumerate(sizes):
        pat = PATTERNS[gi % 4]
        bad = {"right": -1, "wrong0": 0, "wrong_mid": (m - 1) // 2, "wrong_last": m - 2}[pat]
        for j in range(m - 1):
            t = int(right[r0 + j])
            draft.append((t + 1 + gi % max(V - 1, 1)) % V if j == bad else t)     # (V = 1: there is no wrong token)
        draft.append(-1)
        r0 += m
    return draft


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [1, 2, 320, 32001, 32769, 131075])
def test_op_against_oracle(cuda, lib, dtype, V):
    g = torch.Generator().manual_seed(V)
    n = sum(SIZES)
    rows = _rows_for(V, g, dtype, n)
    rows.append(torch.full((V,), float("nan"), dtype=dtype))            # an all-NaN row in a group of its own (greedy: token 0)
    sizes = SIZES + (1,)
    groups = np.concatenate([[0], np.cumsum(sizes)])
    ld = V + 13
    x = torch.zeros(len(rows), ld, dtype=dtype)
    x[:, :V] = torch.stack(rows)
    xd = x.to(cuda)
    # ---- greedy ----
    am = [O.greedy_choice(r.float().numpy()) for r in rows]
    draft = _drafts(am, sizes, V)
    acc, tok = op_verify(lib, xd, groups, draft, None, vocab=V)
    for gi in range(len(sizes)):
        r0, r1 = groups[gi], groups[gi + 1]
        a, toks = O.verify_greedy([r.float().numpy() for r in rows[r0:r1]], draft[r0:r1])
        assert acc[gi] == a and tok[r0:r1].tolist() == toks, (gi, int(acc[gi]), a, tok[r0:r1].tolist(), toks)
        assert tok[r0:r0 + a + 1].tolist() == am[r0:r0 + a + 1]
    if V > 1:
        assert len(set(acc.tolist())) > 2                                # full, partial and zero acceptance all occur
    # ---- sampled: the all-NaN row is an all -inf row (a uniform draw) ----
    combos = [(0.7, 50, 0.9), (1.0, 0, 1.0), (5.0, V + 7, 0.5), (0.01, 1, 1.0), (0.7, 0, 0.0)]
    prm, seeds = [], []
    likely = []
    for r, row in enumerate(rows):
        t, k, p = combos[r % len(combos)]
        s = S.scaled_scores(row, float(np.float32(t)))
        likely.append(int(np.argmax(s)))
    draft = _drafts(likely, sizes, V)
    excused = 0
    for gi in range(len(sizes)):
        r0, r1 = int(groups[gi]), int(groups[gi + 1])
        for seed in range(1000 * gi, 1000 * gi + 8):                     # a seed for which the oracle's decisions are clear of a boundary
            pr = [(float(np.float32(combos[r % len(combos)][0])), combos[r % len(combos)][1], combos[r % len(combos)][2], seed, 3 + r, seed * 3)
                  for r in range(r0, r1)]
            ref = O.verify_sampled(rows[r0:r1], draft[r0:r1], pr)
            if ref[2] > 10 * U_EPS:
                break
        seeds.append((seed, ref))
        prm += [sampling_params(combos[r % len(combos)][0], combos[r % len(combos)][1], combos[r % len(combos)][2], seed=seed, step=3 + r,
                                stream=seed * 3) for r in range(r0, r1)]
    acc, tok = op_verify(lib, xd, groups, draft, prm, vocab=V)
    for gi, (seed, (a, toks, dist)) in enumerate(seeds):
        r0, r1 = int(groups[gi]), int(groups[gi + 1])
        if (int(acc[gi]), tok[r0:r1].tolist()) != (a, toks):
            assert dist < U_EPS, (gi, seed, int(acc[gi]), a, tok[r0:r1].tolist(), toks, dist)
            excused += r1 - r0
    print(f"sampled verify vs oracle, V = {V}: {len(rows)} rows, {excused} rows in groups excused at a boundary")
    assert excused <= 0.02 * len(rows)
    # ---- groups without a draft are vstar_vqa_op_sample, bit for bit ----
    acc1, tok1 = op_verify(lib, xd, np.arange(len(rows) + 1), [-1] * len(rows), prm, vocab=V)
    ref_tok, _, _ = op_sample(lib, xd, prm, vocab=V)
    assert (acc1 == 0).all() and tok1.tolist() == ref_tok.tolist()


def test_op_distribution_chi_square(cuda, lib):
    scipy_stats = pytest.importorskip("scipy.stats")
    g = torch.Generator().manual_seed(21)
    V = 1000
    x = (torch.randn(V, generator=g) * 2).half()
    xd = x[None].expand(256, V).contiguous().to(cuda)
    ref = S.sample_row(x, 0.8, 50, 0.9, 0.5)
    q = ref["q"]
    order = np.argsort(-q)
    for name, xdraft in (("likely", int(order[0])), ("unlikely", int(order[ref["n_kept"] - 1])), ("unkept", int(order[-1]))):
        counts, n = np.zeros(V, np.int64), 0
        groups = np.arange(0, 257, 2)                                    # 128 groups of [row with the draft, last row]
        draft = [xdraft, -1] * 128
        for launch in range(158):                                        # 20224 first tokens
            prm = [sampling_params(0.8, 50, 0.9, seed=4321, step=launch * 256 + r) for r in range(256)]
            acc, tok = op_verify(lib, xd, groups, draft, prm)
            first = tok[0::2]
            assert ((first == xdraft) == (acc == 1)).all()
            np.add.at(counts, first, 1)
            n += 128
        assert counts[q == 0].sum() == 0
        exp = q * n
        big = exp >= 5
        obs, ex = np.append(counts[big], counts[~big].sum()), np.append(exp[big], exp[~big].sum())
        if ex[-1] == 0:
            obs, ex = obs[:-1], ex[:-1]
        stat, pval = scipy_stats.chisquare(obs, ex)
        print(f"chi-square, {name} draft (q = {q[xdraft]:.4f}): {len(obs)} bins, {n} draws, stat {stat:.1f}, p {pval:.4f}")
        assert pval > 1e-4


def test_op_rejects_bad_arguments(cuda, lib):
    xd = torch.zeros(20, 8, dtype=torch.float16, device=cuda)
    ok = ([0, 3], [1, 2, -1])
    op_verify(lib, xd[:3], *ok)
    for groups, draft in (([0, 3], [1, 8, -1]), ([0, 3], [1, -2, -1]), ([0, 3], [1, 2, 3]), ([0, 17], [0] * 16 + [-1]),
                          ([0, 2], [1, -1, -1]), ([0, 2, 2, 3], [1, -1, -1]), ([1, 3], [1, 2, -1])):
        with pytest.raises(_lib.VstarError):
            op_verify(lib, xd[:len(draft)], groups, draft)
    p = sampling_params(1.0, 50, None)
    p.temperature = 0.0
    with pytest.raises(_lib.VstarError):
        op_verify(lib, xd[:3], *ok, [p] * 3)


# ------------------------------------------------ engines ------------------------------------------------
_ENGINES = {}


def _engine(kind):
    """tiny: the default tiny geometry; ring / ring8: hidden 512 (the LDS-ring GEMV is live), fp16 / int8 decode weights, and a
    short context so that a decode reaches max_ctx."""
    if kind not in _ENGINES:
        if kind == "tiny":
            from tests.test_vqa_gpu import engine_for
            cfg = VQAConfig.tiny()
            _ENGINES[kind] = (engine_for(cfg, 0), cfg)
        else:
            cfg = VQAConfig.tiny(llm_hidden=512, llm_heads=4, llm_mlp=1024, max_ctx=64, decode_weight_bits=8 if kind == "ring8" else 0)
            eng = VqaEngine(cfg, 0)
            eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
            _ENGINES[kind] = (eng, cfg)
    return _ENGINES[kind]


def _prompts(n, seed, length=9):
    g = torch.Generator().manual_seed(seed)
    return [[1] + torch.randint(3, 300, (length - 1 + 2 * i,), generator=g).tolist() for i in range(n)]


def _check_tail(eng, cfg, lib, cuda, step, drafts):
    wanted = [(j, r) for j, s in enumerate(step) for r in range(len(s.rows))]
    groups = np.concatenate([[0], np.cumsum([len(s.rows) for s in step])])
    lg, am = eng.forward(step, wanted)
    xd = torch.from_numpy(lg).to(cuda)
    for prm in (None, [sampling_params(0.8, 50, 0.9, seed=5 + j, step=j) for j in range(len(wanted))]):
        acc, tok = eng.forward_verify(step, wanted, groups, drafts, prm)
        acc_o, tok_o = op_verify(lib, xd, groups, drafts, prm)
        assert acc.tolist() == acc_o.tolist() and tok.tolist() == tok_o.tolist()
        if prm is None:                                                   # greedy tokens are vstar_vqa_forward's arg-max of the row
            assert all(tok[r] in (-1, am[r]) for r in range(len(wanted))) and (tok[groups[:-1]] == am[groups[:-1]]).all()
    return am


@pytest.mark.parametrize("kind", ["tiny", "ring", "ring8"])
def test_engine_tail_equals_op_on_the_forward_logits(cuda, lib, kind):
    eng, cfg = _engine(kind)
    for n in (1, 3):
        prompts = _prompts(n, 40 + n)
        _, first = eng.forward([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [(i, -1) for i in range(n)], logits=False)
        # ragged draft lengths; the drafts of sequence 0 are the model's own continuation (found by a first call), the others random
        lens = [3, 0, 6][:n]
        g = torch.Generator().manual_seed(n)
        rows = [[int(first[i])] + torch.randint(3, 300, (lens[i],), generator=g).tolist() for i in range(n)]
        step = [Seq(rows[i], kv_slot=i, past_len=len(prompts[i])) for i in range(n)]
        drafts = sum([r[1:] + [-1] for r in rows], [])
        am = _check_tail(eng, cfg, lib, cuda, step, drafts)
        rows[0] = [rows[0][0]] + [int(t) for t in am[:3]]                # now a draft whose first token is right
        step = [Seq(rows[i], kv_slot=i, past_len=len(prompts[i])) for i in range(n)]
        drafts = sum([r[1:] + [-1] for r in rows], [])
        _check_tail(eng, cfg, lib, cuda, step, drafts)
        acc, _ = eng.forward_verify(step, [(j, r) for j, s in enumerate(step) for r in range(len(s.rows))],
                                    np.concatenate([[0], np.cumsum([len(s.rows) for s in step])]), drafts)
        assert acc[0] >= 1
    # error cases: another tail's order of rows, a bad draft, too long a group
    p = _prompts(1, 1)[0]
    eng.forward([Seq(p, kv_slot=0)], [(0, -1)], logits=False)
    st = [Seq([5, 6, 7], kv_slot=0, past_len=len(p))]
    for wanted, groups, draft in (([(0, 1), (0, 0), (0, 2)], [0, 3], [6, 7, -1]), ([(0, 0), (0, 1), (0, 2)], [0, 3], [6, cfg.llm_vocab, -1]),
                                  ([(0, 0), (0, 1), (0, 2)], [0, 2], [6, 7, -1])):
        with pytest.raises(_lib.VstarError):
            eng.forward_verify(st, wanted, groups, draft)
    with pytest.raises(_lib.VstarError):
        eng.forward_verify([Seq([5] * 17, kv_slot=0, past_len=len(p))], [(0, r) for r in range(17)], [0, 17], [5] * 16 + [-1])


def test_engine_tail_on_a_beam_reordered_slot(cuda, lib):
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    p = _prompts(1, 77)[0]
    llm.beam_decode([Seq(p, kv_slot=0)], [len(p)], [len(p)], 5, 3)      # slots 0 .. 2 are ancestral afterwards
    step = [Seq([9, 10, 11, 12], kv_slot=1, past_len=len(p) + 2)]
    _check_tail(eng, cfg, lib, cuda, step, [10, 11, 12, -1])
    # rejected rows are overwritten: the same call again, then a one-row step behind an accepted prefix, equal a fresh engine's
    lg_a, _ = eng.forward([Seq([9, 10], kv_slot=1, past_len=len(p) + 2)], [(0, 1)])
    eng.forward_verify(step, [(0, r) for r in range(4)], [0, 4], [10, 11, 12, -1])
    lg_b, _ = eng.forward([Seq([9, 10], kv_slot=1, past_len=len(p) + 2)], [(0, 1)])
    assert (lg_a == lg_b).all()


# ------------------------------------------------ speculative_decode ------------------------------------------------
def _host_loop(eng, cfg, prompts, max_new, d, draft_fn, slot0, choose=None, first=None):
    n = len(prompts)
    if first is None:
        _, first = eng.forward([Seq(p, kv_slot=slot0 + i) for i, p in enumerate(prompts)], [(i, -1) for i in range(n)], logits=False)

    def step_fn(batch):
        step = [Seq(rows, kv_slot=slot0 + i, past_len=pos) for i, rows, pos, _ in batch]
        lg, _ = eng.forward(step, [(j, r) for j, s in enumerate(step) for r in range(len(s.rows))])
        off = np.concatenate([[0], np.cumsum([len(s.rows) for s in step])])
        return [lg[off[j]:off[j + 1]] for j in range(len(step))]
    return O.spec_loop(step_fn, first, prompts, [len(p) for p in prompts], max_new, d, draft_fn, 2, cfg.llm_vocab, cfg.max_ctx,
                       cfg.max_rows, choose)


def _plain(llm, prompts, max_new, slot0=0, params=None):
    seqs = [Seq(p, kv_slot=slot0 + i) for i, p in enumerate(prompts)]
    if params is None:
        return llm.greedy_decode(seqs, [len(p) for p in prompts], max_new)
    return llm.sample_decode(seqs, [len(p) for p in prompts], max_new, params)


@pytest.mark.parametrize("kind", ["tiny", "ring"])
def test_speculative_decode_equals_host_loop_over_the_same_calls(cuda, kind):
    eng, cfg = _engine(kind)
    llm = VQA_LLM(cfg=cfg, engine=eng)
    for n in (1, 3):
        prompts = _prompts(n, 3 + n)
        max_new = 12 if kind == "tiny" else 80                           # ring: max_ctx = 64 ends the decode
        plain = _plain(llm, prompts, max_new)
        replay = ReplayDrafter(prompts, plain, cfg.llm_vocab, corrupt=0.35, seed=n)
        for d in (1, 3, 6):
            got = llm.speculative_decode([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [len(p) for p in prompts], prompts, max_new,
                                         d, None, replay)
            stats = dict(llm.spec_stats)
            ref, calls = _host_loop(eng, cfg, prompts, max_new, d, replay, 4)
            assert got == ref, (kind, n, d)
            assert stats["calls"] == calls + 1 and stats["tokens"] == sum(len(o) for o in got)
            assert 0 < stats["accepted"] <= stats["drafted"]
            agree = sum(a == b for g_, p_ in zip(got, plain) for a, b in zip(g_, p_)) / sum(len(p_) for p_ in plain)
            print(f"{kind} n = {n} d = {d}: {stats}, agreement with the stepwise greedy output {agree:.3f}")
            if kind == "ring":
                assert all(len(p) + len(o) == cfg.max_ctx for p, o in zip(prompts, got) if 2 not in o)      # stopped by the full context
        # sampled: the host loop draws with the oracle on the same calls' logits
        params = [sampling_params(0.8, 50, 0.9, seed=60 + i) for i in range(n)]
        dists = []

        def choose(i, t, lg, dr):
            res = O.verify_sampled(list(torch.from_numpy(lg)), dr, [(float(np.float32(0.8)), 50, 0.9, 60 + i, t + r, 0) for r in range(len(dr))])
            dists.append(res[2])
            return res
        got = llm.speculative_decode([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [len(p) for p in prompts], prompts, 10, 3,
                                     params, replay)
        first = eng.forward_sample([Seq(p, kv_slot=4 + i) for i, p in enumerate(prompts)], [(i, -1) for i in range(n)], params)
        ref, _ = _host_loop(eng, cfg, prompts, 10, 3, replay, 4, choose, first)
        if got != ref:
            print(f"sampled decode differs from the host loop; smallest boundary distance {min(dists):.2e}")
            assert min(dists) < U_EPS
        # d = 0 and the empty drafter are the plain decodes, token for token
        for d, fn in ((0, replay), (3, no_draft)):
            assert llm.speculative_decode([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [len(p) for p in prompts], prompts,
                                          max_new, d, None, fn) == plain
            assert llm.speculative_decode([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [len(p) for p in prompts], prompts,
                                          10, d, params, fn) == _plain(llm, prompts, 10, 0, params)


def test_call_counts_and_decisive_seed(cuda):
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    chosen = None
    for seed in range(24):
        p = _prompts(1, 500 + seed)
        plain = _plain(llm, p, 10)
        if 2 in plain[0][:-1] or len(plain[0]) < 10:
            continue
        # the stepwise run's logits: every top-1 / top-2 gap must exceed 10 x the noise of one logit under the 2e-3 rel-L2 bound the
        # decode tests hold — a perturbation e with |e|_2 <= 2e-3 |row|_2 spread over the V logits has the per-logit RMS
        # 2e-3 |row|_2 / sqrt(V)
        lg, _ = eng.forward([Seq(p[0], kv_slot=0)], [(0, -1)])
        gaps = []
        for t in range(10):
            top = np.sort(lg[0].astype(np.float64))[-2:]
            gaps.append((top[1] - top[0]) / (2e-3 * np.linalg.norm(lg[0].astype(np.float64)) / np.sqrt(cfg.llm_vocab)))
            if t < 9:
                lg, _ = eng.forward([Seq([plain[0][t]], kv_slot=0, past_len=len(p[0]) + t)], [(0, 0)])
        if chosen is None:
            chosen = (p, plain, min(gaps))
        if min(gaps) > 10:
            chosen = (p, plain, min(gaps))
            break
    p, plain, gap = chosen
    right = ReplayDrafter(p, plain, cfg.llm_vocab)
    got = llm.speculative_decode([Seq(p[0], kv_slot=0)], [len(p[0])], p, 10, 3, None, right)
    s = dict(llm.spec_stats)
    agree = sum(a == b for a, b in zip(got[0], plain[0])) / len(plain[0])
    print(f"replay drafter: {s}; smallest gap / noise bound {gap:.1f}; agreement with the stepwise greedy output {agree:.3f}")
    assert s["calls"] < s["tokens"]
    if gap > 10:
        assert got == plain
    wrong = ReplayDrafter(p, plain, cfg.llm_vocab, corrupt=1.0)
    got = llm.speculative_decode([Seq(p[0], kv_slot=0)], [len(p[0])], p, 10, 3, None, wrong)
    s = dict(llm.spec_stats)
    assert s["calls"] == s["tokens"] == len(got[0]) and s["accepted"] == 0 and s["drafted"] > 0


def test_engine_state_after_a_speculative_run(cuda):
    from PIL import Image
    cfg = VQAConfig.tiny()
    sd = random_state_dict(cfg, seed=0, dtype=torch.float16)
    fresh = VqaEngine(cfg, 0)
    fresh.load_state_dict(sd)
    eng, _ = _engine("tiny")
    a, b = VQA_LLM(cfg=cfg, engine=eng), VQA_LLM(cfg=cfg, engine=fresh)
    image = Image.fromarray(np.random.default_rng(9).integers(0, 256, (300, 420, 3), dtype=np.uint8))
    q = "What is in the picture?"
    a.free_form_batch([dict(image=image, question=q), dict(image=image, question="Describe it.")], 12, speculative=6,
                      draft_fn=lambda ids, k: [(7 * len(ids) + j) % 300 for j in range(k)])
    for llm in (a, b):
        llm.res = (llm.free_form_inference(image, q, max_new_tokens=8), list(llm.generated_ids[0]),
                   [float(x) for x in llm.option_losses(image, q, ["a cat", "two dogs"])],
                   llm.free_form_inference(image, q, max_new_tokens=6, num_beams=3), list(llm.generated_ids[0]))
    assert a.res == b.res


def test_public_keywords(cuda):
    from PIL import Image
    from vstar_amd import vqa
    from vstar_amd.api import load_pretrained_model
    cfg = VQAConfig.tiny()
    sd = random_state_dict(cfg, seed=0, dtype=torch.float16)
    tokenizer, model, image_processor, _ = load_pretrained_model("seal_vqa_7b", None, "seal_vqa_7bllava", cfg=cfg, state_dict=sd)
    llm = vqa.VQA_LLM(cfg=cfg, engine=model.engine)
    image = Image.fromarray(np.random.default_rng(5).integers(0, 256, (300, 420, 3), dtype=np.uint8))
    q = "What is in the picture? What is in the picture?"
    llm.free_form_inference(image, q, max_new_tokens=8)
    assert llm.spec_stats == {}                                          # speculative = 0: the plain path
    text = llm.free_form_inference(image, q, max_new_tokens=8, speculative=3)
    ids_spec = list(llm.generated_ids[0])
    assert isinstance(text, str) and 1 <= len(ids_spec) <= 8 and llm.spec_stats["tokens"] == len(ids_spec)
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), tokenizer)).unsqueeze(0)
    image_tensor = image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0]
    kw = dict(images=image_tensor.unsqueeze(0).half(), object_features=None, images_long=None, objects_long=None, max_new_tokens=8)
    out = model.generate(input_ids, prompt_lookup_num_tokens=3, **kw)
    assert out[0, input_ids.shape[1]:].tolist() == ids_spec
    llm.free_form_inference(image, q, temperature=0.8, max_new_tokens=8, seed=17, speculative=3)
    out = model.generate(input_ids, do_sample=True, temperature=0.8, seed=17, prompt_lookup_num_tokens=3, **kw)
    assert out[0, input_ids.shape[1]:].tolist() == list(llm.generated_ids[0])
    for bad in (dict(speculative=3, num_beams=2), dict(speculative=16), dict(speculative=-1), dict(speculative=1.5)):
        with pytest.raises(ValueError):
            llm.free_form_inference(image, q, max_new_tokens=4, **bad)
    with pytest.raises(ValueError):
        model.generate(input_ids, prompt_lookup_num_tokens=3, num_beams=2, **kw)
    with pytest.raises(ValueError):
        model.generate(input_ids, prompt_lookup_num_tokens=16, **kw)
