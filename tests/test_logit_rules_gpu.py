"""Logits rules on the MI355X (csrc/edit.hip): the edit op against the CPU oracle (tests/_logit_oracle.py), the
engine's edit stage against the op applied to the same call's unedited logits, and the decode drivers against host loops that edit
on the host.  Every test here needs symbols or keywords this feature adds."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _logit_oracle as O
from tests import _spec_oracle as SO
from tests.test_sampling_gpu import op_sample
from tests.test_spec_gpu import op_verify
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.logits import LogitRules
from vstar_amd.spec import ReplayDrafter
from vstar_amd.vqa import VQA_LLM, sampling_params
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

SENTINEL = 0x1234          # bits of the padding columns [vocab, ld): never written


def op_edit(lib, x_dev, plans, vocab=None):
    """vstar_vqa_op_edit in place on device rows x_dev [rows, ld], the first `vocab` (default ld) of each."""
    rows, ld = x_dev.shape
    off, tok, pen = LogitRules.pack(plans)
    dt = _lib.F16 if x_dev.dtype == torch.float16 else _lib.BF16
    _lib.check_vqa(lib.vstar_vqa_op_edit(ctypes.c_void_p(x_dev.data_ptr()), dt, rows, ld if vocab is None else vocab, ld,
                                         ctypes.c_void_p(off.ctypes.data), ctypes.c_void_p(tok.ctypes.data) if tok.size else None,
                                         ctypes.c_void_p(pen.ctypes.data)))


N_KINDS = 12


def _subset(rng, V, k):
    return sorted(set(int(t) for t in rng.choice(V, size=min(V, max(k, 1)), replace=False)))


def _case(kind, r, V, rng, dtype):
    """One row and its plan.  The kinds: 0 no lists, 1 penalty only, 2 ban only, 3 allow with one id, 4 allow with every id, 5 all
    three overlapping (allow-list of exactly the LDS capacity where V has room), 6 allowed entirely inside banned (an all -inf
    row), 7 lists containing 0 and V - 1 (allow-list one above the LDS capacity), 8 a penalised list of full length V over raw
    bit patterns (subnormals, NaNs, infinities, both zeros), 9 a banned list of full length V, 10 NaN / +-inf / +-0 logits, 11
    theta < 1 with an allow-list of half the vocabulary (searched through L2 once it exceeds the LDS capacity)."""
    x = (torch.from_numpy(rng.standard_normal(V).astype(np.float32)) * 4).to(dtype)
    everything = list(range(V))
    th_hi, th_lo = (1.05, 1.2, 1.3, 2.0, 1.0000001)[r % 5], 0.7
    if kind == 0:
        x[::5] = float("nan")
        return x, ([], 1.0, [], [])
    if kind == 1:
        return x, (_subset(rng, V, V // 3), th_hi, [], [])
    if kind == 2:
        return x, ([], 1.0, _subset(rng, V, V // 7), [])
    if kind == 3:
        return x, ([], 1.0, [], [int(rng.integers(0, V))])
    if kind == 4:
        return x, ([], 1.0, [], everything)
    if kind == 5:
        base = _subset(rng, V, 8192 if V > 9000 else V // 2)
        return x, (base[::2] + _subset(rng, V, 5), th_hi, base[::3] + _subset(rng, V, 3), base)
    if kind == 6:
        ban = _subset(rng, V, V // 2)
        return x, ([], 1.0, ban, ban[::2])
    if kind == 7:
        ends = [0, V - 1]
        return x, (ends + _subset(rng, V, 9), th_hi, ends, ends + _subset(rng, V, 8200 if V > 9000 else 4))
    if kind == 8:
        bits = (torch.arange(V, dtype=torch.int32) + 32768 * (r // N_KINDS) + 4096 * r) & 0xffff
        return bits.to(torch.int16).view(dtype), (everything, (th_lo, th_hi)[(r // N_KINDS) % 2], [], [])
    if kind == 9:
        return x, (_subset(rng, V, 3), th_hi, everything, [])
    if kind == 10:
        special = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 65504.0, -65504.0, 6e-8, -6e-8], dtype=dtype)
        x[torch.arange(V) % 3 == 0] = special[torch.arange((V + 2) // 3) % len(special)]
        return x, (everything[::2] + everything[1::6], th_hi, _subset(rng, V, 4), [])
    return x, (_subset(rng, V, V // 4), th_lo, _subset(rng, V, 6), _subset(rng, V, V // 2))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [1, 2, 320, 32001, 32769, 131075])
def test_op_against_oracle(cuda, lib, dtype, V):
    rng = np.random.default_rng(V)
    n = 5 * N_KINDS
    rows, plans = zip(*[_case(r % N_KINDS, r, V, rng, dtype) for r in range(n)])
    x = torch.stack(rows)
    ref = O.edit_rows(x, plans)
    assert bool(torch.isinf(ref[6]).all()) and (ref[6] < 0).all()              # kind 6: an all -inf row
    for ld in (V + 13, (V + 255) // 256 * 256):                                # unaligned rows; the engine's own stride
        buf = torch.full((n, ld), SENTINEL, dtype=torch.int16).view(dtype)
        buf[:, :V] = x
        xd = buf.to(cuda)
        op_edit(lib, xd, plans, vocab=V)
        got = xd.cpu()
        assert (got[:, V:].view(torch.int16) == SENTINEL).all(), ld
        for r in range(n):
            if not plans[r][0]:        # no arithmetic on the row: the bits themselves (a row without lists keeps its NaN payloads too)
                assert (got[r, :V].view(torch.int16) == ref[r].view(torch.int16)).all(), (ld, r, r % N_KINDS)
            else:                      # penalised: bit for bit, any NaN for a NaN (tests/_logit_oracle.same_bits)
                assert O.same_bits(got[r, :V], ref[r]), (ld, r, r % N_KINDS)


def test_op_rejects_bad_lists(cuda, lib):
    xd = torch.zeros(4, 16, dtype=torch.float16, device=cuda)
    op_edit(lib, xd, [([1], 1.2, [2], [3])] * 4)
    for plan in (([1], 0.0, [], []), ([1], float("nan"), [], []), ([16], 1.2, [], []), ([], 1.0, [-1], [])):
        with pytest.raises(_lib.VstarError):
            op_edit(lib, xd, [plan] * 4)


# ------------------------------------------------ engines ------------------------------------------------
_ENGINES = {}


def _engine(kind):
    """tiny: the default tiny geometry; q: the same with the block-scaled fp8 KV cache and int4 decode weights (the edit stage is
    independent of both)."""
    if kind not in _ENGINES:
        cfg = VQAConfig.tiny()
        if kind == "q":
            cfg = cfg.with_kv_bits(8).with_decode_bits(4)
        eng = VqaEngine(cfg, 0)
        eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
        _ENGINES[kind] = (eng, cfg)
    return _ENGINES[kind]


def _prompts(n, seed, length=9):
    g = torch.Generator().manual_seed(seed)
    return [[1] + torch.randint(3, 300, (length - 1 + 2 * i,), generator=g).tolist() for i in range(n)]


def _plans_for(n_rows, V, seed, am0):
    """Mixed plans; the rows with a banned list ban the unedited arg-max am0[j] too, so their arg-max has to move."""
    rng = np.random.default_rng(seed)
    plans = []
    for j in range(n_rows):
        kind = j % 5
        pen = _subset(rng, V, 40) if kind in (0, 2, 4) else []
        ban = sorted(set(_subset(rng, V, 9) + [int(am0[j])])) if kind in (1, 2, 4) else []
        allow = _subset(rng, V, 6) if kind == 4 else []
        plans.append((pen, (1.3, 0.7)[j % 2], ban, allow))
    plans[-1] = ([], 1.0, [], [])                                              # one row without lists
    return plans


@pytest.mark.parametrize("kind", ["tiny", "q"])
def test_engine_edit_stage_equals_op_on_the_same_logits(cuda, lib, kind):
    eng, cfg = _engine(kind)
    V = cfg.llm_vocab
    assert eng.logit_edit_capacity() == 256 * (cfg.max_ctx + 2048)
    for n in (1, 3):
        prompts = _prompts(n, 70 + n)
        pre = [Seq(p, kv_slot=i) for i, p in enumerate(prompts)]
        want0 = [(i, -1) for i in range(n)]
        lg_plain, am_plain = eng.forward(pre, want0)
        # a multi-row continuation, every row wanted: the verify call's shape
        rows = [[int(am_plain[i])] + [5 + i, 6, 7][:2 + i % 2] for i in range(n)]
        step = [Seq(rows[i], kv_slot=i, past_len=len(prompts[i])) for i in range(n)]
        wanted = [(j, r) for j, s in enumerate(step) for r in range(len(s.rows))]
        groups = np.concatenate([[0], np.cumsum([len(s.rows) for s in step])])
        lg0, am0 = eng.forward(step, wanted)
        plans = _plans_for(len(wanted), V, n, am0)
        edits = LogitRules.pack(plans)
        # ---- forward: the edited logits are the op on the unedited ones (and the oracle); the arg-max is theirs ----
        lg1, am1 = eng.forward(step, wanted, edits=edits)
        xd = torch.from_numpy(lg0).to(cuda)
        op_edit(lib, xd, plans)
        exp = xd.cpu()
        assert (torch.from_numpy(lg1).view(torch.int16) == exp.view(torch.int16)).all()
        assert O.same_bits(exp, O.edit_rows(torch.from_numpy(lg0), plans))
        assert am1.tolist() == [O.first_argmax(exp[j].float().numpy()) for j in range(len(wanted))]
        assert am1.tolist() != am0.tolist()                                    # the plans do move some arg-max
        assert (eng.forward(step, wanted, logits=False, edits=edits)[1] == am1).all()
        # ---- sample / verify tails see the edited rows ----
        prm = [sampling_params(0.8, 50, 0.9, seed=11 + j, step=j) for j in range(len(wanted))]
        assert eng.forward_sample(step, wanted, prm, edits=edits).tolist() == op_sample(lib, xd, prm)[0].tolist()
        drafts = sum([[int(am1[groups[j] + r]) if r % 2 == 0 else 4 for r in range(len(s.rows) - 1)] + [-1] for j, s in enumerate(step)], [])
        for p in (None, prm):
            acc, tok = eng.forward_verify(step, wanted, groups, drafts, p, edits=edits)
            acc_o, tok_o = op_verify(lib, xd, groups, drafts, p)
            assert acc.tolist() == acc_o.tolist() and tok.tolist() == tok_o.tolist()
        assert eng.forward_verify(step, wanted, groups, drafts, None, edits=edits)[0].max() >= 1
        # ---- empty lists = no edits; a plain call after edited ones gives the bits it gave before ----
        empty = LogitRules.pack([([], 1.0, [], [])] * len(wanted))
        lg2, am2 = eng.forward(step, wanted, edits=empty)
        lg3, am3 = eng.forward(step, wanted)
        for lg, am in ((lg2, am2), (lg3, am3)):
            assert (lg.view(np.int16) == lg0.view(np.int16)).all() and (am == am0).all()
        assert (eng.forward_sample(step, wanted, prm) == eng.forward_sample(step, wanted, prm, edits=empty)).all()
        lg4, am4 = eng.forward(pre, want0)
        assert (lg4.view(np.int16) == lg_plain.view(np.int16)).all() and (am4 == am_plain).all()


def test_engine_rejects_bad_edits_and_stays_usable(cuda, lib):
    eng, cfg = _engine("tiny")
    V = cfg.llm_vocab
    p = _prompts(1, 5)[0]
    seqs, want = [Seq(p, kv_slot=0)], [(0, -1), (0, -2)]
    lg0, am0 = eng.forward(seqs, want)
    ok = LogitRules.pack([([3], 1.2, [4], []), ([], 1.0, [], [7, 9])])
    cap = eng.logit_edit_capacity()
    big_off = np.array([0, 0, 0, cap + 1, cap + 1, cap + 1, cap + 1], np.int32)
    bad = {
        "over capacity": ((big_off, np.zeros(cap + 1, np.int32), np.ones(2, np.float32)), str(cap)),
        "id == vocab": (LogitRules.pack([([V], 1.2, [], []), ([], 1.0, [], [])]), "outside"),
        "theta 0": (LogitRules.pack([([3], 0.0, [], []), ([], 1.0, [], [])]), "finite and > 0"),
        "repeated id": ((np.array([0, 2, 2, 2, 2, 2, 2], np.int32), np.array([3, 3], np.int32), np.ones(2, np.float32)), "strictly"),
        "decreasing offset": ((np.array([0, 2, 1, 2, 2, 2, 2], np.int32), np.array([3, 5], np.int32), np.ones(2, np.float32)), "decrease"),
        "off[0] != 0": ((np.array([1, 2, 2, 2, 2, 2, 2], np.int32), np.array([3, 5], np.int32), np.ones(2, np.float32)), "off[0]"),
    }
    for name, (edits, msg) in bad.items():
        with pytest.raises(_lib.VstarError, match=msg.replace("[", r"\[").replace("]", r"\]")):
            eng.forward(seqs, want, edits=edits)
        with pytest.raises(_lib.VstarError):
            eng.forward_sample(seqs, want, sampling_params(0.8, 50, 0.9, seed=1), edits=edits)
    with pytest.raises(ValueError):                                            # plans for another number of rows
        eng.forward(seqs, want, edits=LogitRules.pack([([3], 1.2, [], [])]))
    # the row fault is the one reported when both are wrong
    with pytest.raises(_lib.VstarError, match="max_ctx"):
        eng.forward([Seq(p, kv_slot=0, past_len=cfg.max_ctx)], [(0, -1)], edits=LogitRules.pack([([V], 0.0, [], [])]))
    # the beam and scoring tails take no edits at the C ABI either: the Python face has no such parameter
    import inspect
    assert "edits" not in inspect.signature(VqaEngine.forward_beam).parameters
    assert "edits" not in inspect.signature(VqaEngine.forward_score).parameters
    lg1, am1 = eng.forward(seqs, want, edits=ok)
    assert O.same_bits(torch.from_numpy(lg1), O.edit_rows(torch.from_numpy(lg0), [([3], 1.2, [4], []), ([], 1.0, [], [7, 9])]))
    lg2, am2 = eng.forward(seqs, want)
    assert (lg2.view(np.int16) == lg0.view(np.int16)).all() and (am2 == am0).all()


# ------------------------------------------------ drivers ------------------------------------------------
def _image(seed):
    from PIL import Image
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (300, 420, 3), dtype=np.uint8))


QUESTIONS = ("What is in the picture?", "Describe it.", "Is the cat on the mat or is the cat on the mat?", "What colour is the bus?",
             "How many people are there?", "Where is the dog?")


def _prepare(llm, samples):
    """free_form_batch's own preparation: features into slots, rows, text ids."""
    seqs, lens, text = [], [], []
    fslot = 0
    for i, s in enumerate(samples):
        img_slots, obj_slots = llm._encode(s["image"], None, fslot)
        fslot += 1 + len(obj_slots)
        ids, rows = llm._question_rows(s["question"], img_slots, obj_slots, None, None)
        seqs.append(Seq(rows, kv_slot=i))
        lens.append(len(rows))
        text.append([t for t in ids if t >= 0])
    return seqs, lens, text


def _host_decode(llm, samples, max_new, rule_kw):
    """VQA_LLM._decode's loop over engine.forward(logits=True) WITHOUT edits: the oracle plans and edits on the host, the token is
    the first arg-max."""
    eng, cfg, eos = llm.engine, llm.cfg, llm.eos_token_id
    seqs, lens, text = _prepare(llm, samples)
    n = len(seqs)

    def pick(step, want, idx, out):
        lg, _ = eng.forward(step, want)
        x = torch.from_numpy(lg)
        plans = [O.plan(text[i] + out[i], len(out[i]), eos, batch_id=i, **rule_kw) for i in idx]
        return [O.first_argmax(O.edit_row(x[j], *plans[j]).float().numpy()) for j in range(len(idx))]

    out = [[] for _ in range(n)]
    cur = dict(enumerate(pick(seqs, [(i, -1) for i in range(n)], list(range(n)), out)))
    pos, live = list(lens), list(range(n))
    for _ in range(max_new):
        still = []
        for i in live:
            out[i].append(cur[i])
            if cur[i] != eos and pos[i] + 1 < cfg.max_ctx:
                still.append(i)
        live = still
        if not live or len(out[live[0]]) >= max_new:
            break
        nxt = pick([Seq([cur[i]], kv_slot=i, past_len=pos[i]) for i in live], [(j, 0) for j in range(len(live))], live, out)
        for j, i in enumerate(live):
            cur[i] = nxt[j]
            pos[i] += 1
    return out, text


def _new_bigram_repeats(text, out):
    """Generated tokens that complete a bigram already present in front of them (history = text ids + earlier output)."""
    h, bad = list(text), 0
    for t in out:
        seen = set(zip(h[:-1], h[1:]))
        bad += len(h) >= 1 and (h[-1], t) in seen
        h.append(t)
    return bad


ALLOWED5 = [7, 19, 33, 150, 301]
RULE_SETS = (
    dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
    dict(min_new_tokens=6, bad_words_ids=[[5], [7, 9]], suppress_tokens=[11, 12]),
    dict(allowed_tokens_fn=lambda b, h: ALLOWED5, repetition_penalty=1.2),
)


@pytest.mark.parametrize("n", [1, 3])
def test_free_form_batch_with_rules_equals_host_loop(cuda, n):
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    eos, max_new = llm.eos_token_id, 14
    # samples whose UNRULED greedy output repeats a bigram: otherwise the n-gram rule would have nothing to do
    picked = []
    for qi, q in enumerate(QUESTIONS):
        s = dict(image=_image(qi), question=q)
        llm.free_form_batch([s], max_new)
        _, _, text = _prepare(llm, [s])
        if _new_bigram_repeats(text[0], llm.generated_ids[0]) > 0:
            picked.append(s)
        if len(picked) == n:
            break
    assert len(picked) == n, "no sample whose unruled greedy output repeats a bigram: the bigram test would show nothing"
    for kw in RULE_SETS:
        llm.free_form_batch(picked, max_new, **kw)
        got = [list(o) for o in llm.generated_ids]
        ref, text = _host_decode(llm, picked, max_new, kw)
        assert got == ref, kw
        for i in range(n):
            if kw.get("no_repeat_ngram_size") == 2:
                assert _new_bigram_repeats(text[i], got[i]) == 0
            if kw.get("min_new_tokens"):
                assert eos not in got[i][:kw["min_new_tokens"]]
                assert not {5, 11, 12} & set(got[i])
            if "allowed_tokens_fn" in kw:
                assert set(got[i]) <= set(ALLOWED5)
    # all defaults: the plain call, token for token; and the single-sample face
    llm.free_form_batch(picked, max_new)
    plain = [list(o) for o in llm.generated_ids]
    llm.free_form_batch(picked, max_new, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    assert [list(o) for o in llm.generated_ids] == plain
    llm.free_form_inference(picked[0]["image"], picked[0]["question"], max_new_tokens=max_new, **RULE_SETS[0])
    if n == 1:
        assert list(llm.generated_ids[0]) == _host_decode(llm, picked[:1], max_new, RULE_SETS[0])[0][0]


@pytest.mark.parametrize("n", [1, 3])
def test_speculative_decode_with_rules_equals_host_loop_over_its_verify_calls(cuda, n):
    eng, cfg = _engine("tiny")
    llm = VQA_LLM(cfg=cfg, engine=eng)
    eos, V, max_new = llm.eos_token_id, cfg.llm_vocab, 12
    prompts = _prompts(n, 90 + n)
    lens = [len(p) for p in prompts]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4)
    rules = LogitRules(**kw)
    seqs = lambda slot0: [Seq(p, kv_slot=slot0 + i) for i, p in enumerate(prompts)]      # noqa: E731
    ruled = llm.greedy_decode(seqs(0), lens, max_new, rules, prompts)            # the stepwise ruled decode: what the drafter replays
    for i in range(n):
        assert _new_bigram_repeats(prompts[i], ruled[i]) == 0 and eos not in ruled[i][:4]
    replay = ReplayDrafter(prompts, ruled, V, corrupt=0.35, seed=n)
    for d in (1, 4):
        got = llm.speculative_decode(seqs(0), lens, prompts, max_new, d, None, replay, rules)
        stats = dict(llm.spec_stats)
        # host loop over the same calls: unedited logits from the engine, oracle plans + edits + greedy verify on the host
        lg, _ = eng.forward(seqs(4), [(i, -1) for i in range(n)])
        first = [O.first_argmax(O.edit_row(torch.from_numpy(lg)[i], *O.plan(prompts[i], 0, eos, batch_id=i, **kw)).float().numpy())
                 for i in range(n)]
        mine = [[t] for t in first]

        def step_fn(batch):
            step = [Seq(rows, kv_slot=4 + i, past_len=pos) for i, rows, pos, _ in batch]
            lg, _ = eng.forward(step, [(j, r) for j, s in enumerate(step) for r in range(len(s.rows))])
            off = np.concatenate([[0], np.cumsum([len(s.rows) for s in step])])
            return [lg[off[j]:off[j + 1]] for j in range(len(step))]

        def choose(i, t, lg, dr):
            base = list(prompts[i]) + mine[i]
            assert t == len(mine[i])
            x = torch.from_numpy(np.ascontiguousarray(lg))
            ed = [O.edit_row(x[r], *O.plan(base + dr[:r], len(mine[i]) + r, eos, batch_id=i, **kw)).float().numpy() for r in range(len(dr))]
            a, toks = SO.verify_greedy(ed, dr)
            new = toks[:a + 1]
            mine[i] += new[:new.index(eos) + 1] if eos in new else new
            return a, toks

        ref, calls = SO.spec_loop(step_fn, first, prompts, lens, max_new, d, replay, eos, V, cfg.max_ctx, cfg.max_rows, choose)
        assert got == ref, (n, d)
        assert stats["calls"] == calls + 1 and 0 < stats["accepted"] <= stats["drafted"]
        for i in range(n):
            assert _new_bigram_repeats(prompts[i], got[i]) == 0 and eos not in got[i][:4]
    # rules at their defaults: the plain speculative decode
    plain = llm.speculative_decode(seqs(0), lens, prompts, max_new, 3, None, replay)
    assert llm.speculative_decode(seqs(0), lens, prompts, max_new, 3, None, replay, LogitRules()) == plain
