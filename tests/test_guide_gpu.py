"""Guided decoding against a negative sequence on the MI355X (csrc/guide.hip): the kernel through its door against
the CPU oracle (tests/_guide_oracle.py) on exactly the cases of the CPU census, the door's refusals, the engine's guidance stage
against plain forwards plus the oracle, and the decode loop and public keywords against host replays.  Every test here needs an
export, a kernel or a keyword the feature adds."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import _guide_oracle as G
from tests import _logit_oracle as O
from tests import _logprob_oracle as L
from tests import _sampling_oracle as S
from tests import _score_oracle as SC
from tests.test_logit_rules_gpu import QUESTIONS, _image
from tests.test_sampling_gpu import U_EPS
from vstar_amd import _lib, vqa
from vstar_amd.config import VQAConfig
from vstar_amd.vqa import VQA_LLM, sampling_params
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
NO_CUT = np.float32(-np.inf)


def _dev(bits: np.ndarray, bf16: bool, cuda) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16 if bf16 else torch.float16).to(cuda)


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def door(lib, xd: torch.Tensor, vocab, cond, neg, scale, log_beta, rows=None, dtype=None) -> int:
    """vstar_vqa_guide_rows on the device tensor xd [rows, ld]; returns the return code."""
    c, u = np.ascontiguousarray(cond, np.int32), np.ascontiguousarray(neg, np.int32)
    sc, lb = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(log_beta, np.float32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    dt = (_lib.F16 if xd.dtype == torch.float16 else _lib.BF16) if dtype is None else dtype
    return lib.vstar_vqa_guide_rows(ctypes.c_void_p(xd.data_ptr()), dt, xd.shape[0] if rows is None else rows, vocab, xd.shape[1],
                                    len(c), p(c), p(u), p(sc), p(lb))


def excused(got: np.ndarray, want: np.ndarray, band: np.ndarray, alt: np.ndarray, what) -> int:
    """Criterion 1: the bits are the oracle's, except that an element inside the excuse band may hold the adjacent code and nothing
    else.  Returns how many did."""
    diff = got != want
    assert (~diff | (band & (got == alt))).all(), (what, int(diff.sum()), int((diff & ~band).sum()))
    return int(diff.sum())


# ------------------------------------------------ 1. the door against the oracle ------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", G.VOCABS)
def test_door_against_oracle(cuda, lib, V, bf16):
    n_adj = n_all = 0
    for name in "AB":
        x = G.scene(name, V, bf16)
        cache = {}
        ls = {r: G.log_softmax16(x[r, :V], bf16) for r in range(10) if np.isfinite(G.lse(G.to_f64(x[r, :V], bf16)))}
        for sc, lb in G.launches(name):
            want, band, alt = G.guide_rows(x, V, G.COND, G.NEG, sc, lb, bf16, lse_cache=cache)
            xd = _dev(x, bf16, cuda)
            assert door(lib, xd, V, G.COND, G.NEG, sc, lb) == 0, lib.vstar_vqa_last_error(None)
            got = _bits(xd)
            n_adj += excused(got, want, band, alt, (name, V, bf16, sc.tolist(), lb.tolist()))
            n_all += 5 * V
            # canaries, negative rows and unpaired rows: bit for bit what they were
            assert np.array_equal(got[:, V:], x[:, V:]) and np.array_equal(got[list(G.NEG) + [10, 11]], x[list(G.NEG) + [10, 11]])
            for p in range(5):
                c, u = G.COND[p], G.NEG[p]
                if lb[p] != NO_CUT or c not in ls or u not in ls:
                    continue
                fc, fu = np.isfinite(G.to_f64(x[c, :V], bf16)), np.isfinite(G.to_f64(x[u, :V], bf16))
                if sc[p] == 1:         # the once-rounded log_softmax of the conditional row
                    assert np.array_equal(got[c, :V][~band[c, :V]], ls[c][~band[c, :V]]), (name, p)
                if sc[p] == 0:         # ... of the negative row, wherever there is one to take
                    m = fc & fu & ~band[c, :V]
                    assert np.array_equal(got[c, :V][m], ls[u][m]), (name, p)
    print(f"guide door vs oracle V={V} bf16={bf16}: {n_adj} of {n_all} elements took the adjacent code")
    assert n_adj <= G.CAP * n_all


# ------------------------------------------------ 2. the door's refusals ------------------------------------------------
def test_door_refusals(cuda, lib):
    x = G.scene("A", 65, False)
    xd = _dev(x, False, cuda)
    ok = dict(cond=[0, 3], neg=[1, 2], scale=[1.5, 0.5], log_beta=[-np.inf, -1.0])

    def refused(msg, vocab=65, rows=None, dtype=None, **kw):
        a = {**ok, **kw}
        rc = door(lib, xd, vocab, a["cond"], a["neg"], a["scale"], a["log_beta"], rows=rows, dtype=dtype)
        err = lib.vstar_vqa_last_error(None).decode()
        assert rc == -1 and msg in err and err.startswith("vstar_vqa_guide_rows: "), (msg, rc, err)
        assert np.array_equal(_bits(xd), x)                # nothing was launched

    refused("cond_row and neg_row of a pair must differ", cond=[0, 2])            # the first rule of vstar_guide_check's chain
    refused("outside [0, rows)", cond=[0, 12])
    refused("outside [0, rows)", neg=[-1, 2])
    refused("outside [0, rows)", rows=3)
    refused("a row appears in two records", cond=[0, 1], neg=[1, 2])
    refused("a row appears in two records", neg=[1, 1])
    for bad in (-0.5, float("nan"), float("inf")):
        refused("the guidance scale must be finite and >= 0", scale=[1.5, bad])
    for bad in (0.5, float("nan")):
        refused("log_beta must be <= 0 (-inf = no plausibility cut) and not NaN", log_beta=[-np.inf, bad])      # the last rule
    refused("vocabulary size out of range", vocab=0)
    refused("dtype must be F16 or BF16", dtype=_lib.F32)
    refused("ld must be >= vocab", vocab=69)
    null = lib.vstar_vqa_guide_rows(None, _lib.F16, 12, 65, 68, 2, None, None, None, None)
    assert null == -1 and b"NULL" in lib.vstar_vqa_last_error(None)
    assert door(lib, xd, 65, **ok) == 0                    # the library stays usable
    want, band, alt = G.guide_rows(x, 65, ok["cond"], ok["neg"], ok["scale"], ok["log_beta"], False)
    excused(_bits(xd), want, band, alt, "after the refusals")


# ------------------------------------------------ 3. the engine ------------------------------------------------
_ENGINE = []


def _engine():
    if not _ENGINE:
        cfg = VQAConfig.tiny()
        eng = VqaEngine(cfg, 0)
        eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
        _ENGINE.append((eng, cfg))
    return _ENGINE[0]


def _prompts(n, seed, length=9):
    g = torch.Generator().manual_seed(seed)
    return [[1] + torch.randint(3, 300, (length - 1 + 2 * i,), generator=g).tolist() for i in range(n)]


def _lg_bits(lg: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(lg).view(np.uint16)


def test_engine_guidance_stage(cuda, lib):
    eng, cfg = _engine()
    V = cfg.llm_vocab
    pc, pu, p2 = _prompts(3, 21)
    # guidance=None is the call without the keyword
    lg0, am0 = eng.forward([Seq(pc, kv_slot=0), Seq(pu, kv_slot=1)], [(0, -1), (1, -1)])
    lg1, am1 = eng.forward([Seq(pc, kv_slot=0), Seq(pu, kv_slot=1)], [(0, -1), (1, -1)], guidance=None)
    assert np.array_equal(_lg_bits(lg0), _lg_bits(lg1)) and np.array_equal(am0, am1)
    tok0 = eng.forward_sample([Seq(pc, kv_slot=0)], [(0, -1)], sampling_params(0.8, 50, 0.9, seed=3))
    assert np.array_equal(tok0, eng.forward_sample([Seq(pc, kv_slot=0)], [(0, -1)], sampling_params(0.8, 50, 0.9, seed=3), guidance=None))
    # one pair against two plain forwards of the same sequences in fresh slots, and the oracle
    lc, _ = eng.forward([Seq(pc, kv_slot=2)], [(0, -1)])
    lu, _ = eng.forward([Seq(pu, kv_slot=3)], [(0, -1)])
    n_adj = 0
    for gamma, beta in ((1.5, 0.0), (3.0, 0.1), (0.0, 0.0), (1.0, 0.0)):
        with np.errstate(divide="ignore"):
            lb = np.float32(np.log(np.float64(beta)))
        lg, am = eng.forward([Seq(pc, kv_slot=0), Seq(pu, kv_slot=1)], [(0, -1), (1, -1)], guidance=([1], gamma, lb))
        assert lg.shape == (1, V) and am.shape == (1,)
        ref = G.guide_pair(_lg_bits(lc)[0], _lg_bits(lu)[0], gamma, lb, False)
        n_adj += excused(_lg_bits(lg)[0], ref.out, ref.band, ref.alt, ("engine", gamma, beta))
        assert int(am[0]) == G.first_argmax_bits(_lg_bits(lg)[0], False)
        none, am2 = eng.forward([Seq(pc, kv_slot=0), Seq(pu, kv_slot=1)], [(0, -1), (1, -1)], logits=False, guidance=([1], gamma, lb))
        assert none is None and np.array_equal(am, am2)
    assert n_adj <= 1
    # the negative slot's cache advanced by the same count: its K/V rows are those of the plain forward of the same sequence, and a
    # guided one-token step writes the next position of BOTH slots
    k1, k3 = eng.kv_rows(0, 1), eng.kv_rows(0, 3)
    assert np.abs(k3[:, :, :len(pu)]).max() > 0 and np.allclose(k1[:, :, :len(pu)], k3[:, :, :len(pu)], atol=2e-2, rtol=0)
    eng.forward([Seq([7], kv_slot=0, past_len=len(pc)), Seq([7], kv_slot=1, past_len=len(pu))], [(0, 0), (1, 0)], guidance=([1], 1.5, NO_CUT))
    eng.forward([Seq([7], kv_slot=3, past_len=len(pu))], [(0, 0)])
    k1, k3 = eng.kv_rows(0, 1), eng.kv_rows(0, 3)
    assert np.abs(k3[:, :, len(pu)]).max() > 0 and np.allclose(k1[:, :, len(pu)], k3[:, :, len(pu)], atol=2e-2, rtol=0)
    # an unguided output row (neg -1) keeps its logits; edits and log-probabilities see the guided row
    seqs3, want3 = [Seq(pc, kv_slot=0), Seq(p2, kv_slot=1), Seq(pu, kv_slot=4)], [(0, -1), (1, -1), (2, -1)]
    plain3, _ = eng.forward(seqs3, want3)
    lg, am = eng.forward(seqs3, want3, guidance=([2, -1], [1.5, 9.0], [NO_CUT, NO_CUT]))
    assert lg.shape == (2, V) and np.array_equal(_lg_bits(lg)[1], _lg_bits(plain3)[1])
    ref = G.guide_pair(_lg_bits(plain3)[0], _lg_bits(plain3)[2], 1.5, NO_CUT, False)
    excused(_lg_bits(lg)[0], ref.out, ref.band, ref.alt, "two output rows")
    from vstar_amd.logits import LogitRules
    plans = [([], 1.0, [int(am[0])], []), ([5, 9], 1.3, [], [])]
    lgE, amE, rec = eng.forward(seqs3, want3, guidance=([2, -1], [1.5, 9.0], [NO_CUT, NO_CUT]), edits=LogitRules.pack(plans), logprobs=3)
    expE = O.edit_rows(torch.from_numpy(lg.copy()), plans)
    assert O.same_bits(torch.from_numpy(lgE), expE) and int(amE[0]) != int(am[0])
    lp, rank, tt, tl = L.logprobs(expE, amE, 3)
    assert np.array_equal(rec.top_token, tt) and np.array_equal(rec.rank, rank) and SC.ulp_distance(rec.token_logprob, lp).max() <= 1


def test_engine_refuses_bad_guidance_and_stays_usable(cuda, lib):
    """Bad records are VSTAR_ERR_INVALID (-1) before any device work and the engine still serves a plain forward.  LlmCached::forward
    also refuses guidance on the beam, scoring, verify and contrast tails (guide_check names the tail), but the C ABI has guided entries
    for the arg-max and sampling tails only, so no call from outside the library can put guidance on those four: what is pinned here
    is that the Python face offers no such keyword."""
    eng, cfg = _engine()
    pc, pu, p2 = _prompts(3, 22)
    seqs, want = [Seq(pc, kv_slot=0), Seq(p2, kv_slot=1), Seq(pu, kv_slot=2)], [(0, -1), (1, -1), (2, -1)]
    lg0, am0 = eng.forward(seqs, want)
    bad = {
        "neg must be -1 (unguided) or an index into want in [n_out, n_want)": ([0, 2], 1.5, NO_CUT),
        "a negative row belongs to two output rows": ([2, 2], 1.5, NO_CUT),
        "belongs to no output row": ([-1, -1], 1.5, NO_CUT),
        "the guidance scale must be finite and >= 0": ([2, -1], [-1.0, 1.0], NO_CUT),
        "log_beta must be <= 0": ([2, -1], 1.5, [0.25, 0.0]),
    }
    for msg, g in bad.items():
        with pytest.raises(_lib.VstarError, match="error -1: .*" + msg.replace("[", r"\[").replace("(", r"\(").replace(")", r"\)")):
            eng.forward(seqs, want, guidance=g)
        with pytest.raises(_lib.VstarError, match="error -1"):
            eng.forward_sample(seqs, want, sampling_params(0.8, 50, 0.9, seed=1), guidance=g)
    for g in (([], 1.5, NO_CUT), ([3, -1, -1, -1], 1.5, NO_CUT)):          # n_out outside [1, n_want]: the Python face's own check
        with pytest.raises(ValueError):
            eng.forward(seqs, want, guidance=g)
    args, _keep = eng._rows_args(seqs, want)                                # ... and the C ABI's
    neg = np.int32([2, -1])
    one = np.float32([1.5, 1.5])
    gd = _lib.VqaGuidance(4, neg.ctypes.data, one.ctypes.data, one.ctypes.data)
    assert eng.lib.vstar_vqa_forward_guided(eng.handle, *args, None, None, ctypes.byref(gd), None, None) == -1
    assert b"n_out must be in [1, n_want]" in eng.lib.vstar_vqa_last_error(eng.handle)
    # the beam, scoring, verify and contrast tails have no guided entry at the C ABI, and the Python face no such keyword
    for fn in (VqaEngine.forward_beam, VqaEngine.forward_score, VqaEngine.forward_verify, VqaEngine.forward_contrast_begin,
               VqaEngine.forward_contrast_step):
        assert "guidance" not in inspect.signature(fn).parameters
    lg1, am1 = eng.forward(seqs, want)
    assert np.array_equal(_lg_bits(lg0), _lg_bits(lg1)) and np.array_equal(am0, am1)


# ------------------------------------------------ 4. the loop and the public keywords ------------------------------------------------
def _replay(eng, cfg, eos, pairs, tokens, gamma, log_beta, pick):
    """The host replay of a guided decode: plain forwards with logits over the same (sequence, negative sequence) pairs — pairs[i] =
    (rows, negative rows, slot, negative slot) — fed the tokens the device chose, the oracle's guided row of every step, and
    pick(i, t, guided row as an fp16 tensor) -> token.  Returns the picked tokens and the guided rows, per pair."""
    n = len(pairs)
    picks, rows_out = [[] for _ in range(n)], [[] for _ in range(n)]
    live = list(range(n))
    seqs = [Seq(list(pairs[i][0]), kv_slot=pairs[i][2]) for i in live] + [Seq(list(pairs[i][1]), kv_slot=pairs[i][3]) for i in live]
    want = [(j, -1) for j in range(2 * n)]
    pos = [[len(p[0]), len(p[1])] for p in pairs]
    t = 0
    while live:
        lg, _ = eng.forward(seqs, want)
        m = len(live)
        for j, i in enumerate(live):
            g = G.guide_pair(_lg_bits(lg)[j], _lg_bits(lg)[m + j], gamma, log_beta, False)
            row = torch.from_numpy(g.out.view(np.float16).copy())
            rows_out[i].append(row)
            picks[i].append(pick(i, t, row))
        t += 1
        live = [i for i in live if t < len(tokens[i])]
        seqs = [Seq([tokens[i][t - 1]], kv_slot=pairs[i][2], past_len=pos[i][0]) for i in live] + \
               [Seq([tokens[i][t - 1]], kv_slot=pairs[i][3], past_len=pos[i][1]) for i in live]
        want = [(j, 0) for j in range(2 * len(live))]
        for i in live:
            pos[i][0] += 1
            pos[i][1] += 1
    return picks, rows_out


def _pairs(llm, samples, negative_image=None, negative_question=None):
    """free_form_batch's own preparation of guided samples: features into slots, rows, negative rows, text ids."""
    eng = llm.engine
    pairs, text, fslot = [], [], 0
    for i, s in enumerate(samples):
        img_slots, obj_slots = llm._encode(s["image"], None, fslot)
        fslot += 1
        ids, rows = llm._question_rows(s["question"], img_slots, obj_slots, None, None)
        nids = ids if negative_question is None else llm._question_rows(negative_question, img_slots, obj_slots, None, None)[0]
        if negative_image is None:
            nrows = [t for t in nids if t >= 0]
        else:
            eng.encode_images(llm.image_processor.preprocess(negative_image, return_tensors="pt")["pixel_values"][0][None], fslot)
            nrows = eng.expand_ids(nids, [fslot], obj_slots, None, None)
            fslot += 1
        pairs.append((rows, nrows, 2 * i, 2 * i + 1))
        text.append([t for t in ids if t >= 0])
    return pairs, text


def _llm():
    eng, cfg = _engine()
    return VQA_LLM(cfg=cfg, engine=eng), eng, cfg


@pytest.mark.parametrize("neg", ["prior", "image", "question"])
@pytest.mark.parametrize("beta", [0.0, 0.1])
def test_free_form_guided_greedy_equals_host_replay(cuda, neg, beta):
    llm, eng, cfg = _llm()
    s = dict(image=_image(1), question=QUESTIONS[0])
    kw = dict(negative_image=_image(8)) if neg == "image" else dict(negative_question=QUESTIONS[3]) if neg == "question" else {}
    llm.free_form_inference(s["image"], s["question"], max_new_tokens=8, guidance_scale=1.5, plausibility_beta=beta, **kw)
    got = [list(llm.generated_ids[0])]
    assert 1 <= len(got[0]) <= 8
    with np.errstate(divide="ignore"):
        lb = np.float32(np.log(np.float64(beta)))
    pairs, _ = _pairs(llm, [s], **kw)
    assert (len(pairs[0][1]) < len(pairs[0][0])) == (neg != "image")
    picks, _ = _replay(eng, cfg, llm.eos_token_id, pairs, got, 1.5, lb, lambda i, t, row: O.first_argmax(row.float().numpy()))
    assert picks == got
    # guidance does something: the greedy decode of the same sample differs (or the test shows nothing)
    llm.free_form_inference(s["image"], s["question"], max_new_tokens=8)
    plain = list(llm.generated_ids[0])
    llm.free_form_inference(s["image"], s["question"], max_new_tokens=8, guidance_scale=1, **kw)      # 1 is off, as in HF
    assert list(llm.generated_ids[0]) == plain
    if neg == "prior" and beta == 0:
        assert plain != got[0]


def test_free_form_guided_with_rules_and_logprobs_equals_host_replay(cuda):
    from tests.test_logprob_gpu import check_against_oracle
    llm, eng, cfg = _llm()
    s = dict(image=_image(2), question=QUESTIONS[2])
    rule_kw = dict(repetition_penalty=1.3)
    llm.free_form_inference(s["image"], s["question"], max_new_tokens=8, guidance_scale=1.5, logprobs=3, **rule_kw)
    got, rec = [list(llm.generated_ids[0])], llm.generated_logprobs[0]
    pairs, text = _pairs(llm, [s])
    edited = []

    def pick(i, t, row):
        plan = O.plan(text[i] + got[i][:t], t, llm.eos_token_id, batch_id=i, **rule_kw)
        edited.append(O.edit_row(row, *plan))
        return O.first_argmax(edited[-1].float().numpy())
    picks, _ = _replay(eng, cfg, llm.eos_token_id, pairs, got, 1.5, NO_CUT, pick)
    assert picks == got and rec.token_logprob.shape == (len(got[0]),) and rec.top_token.shape == (len(got[0]), 3)
    check_against_oracle(rec, torch.stack(edited), got[0], 3, "guided + rules + logprobs")


def test_free_form_guided_sampled_equals_sampling_oracle(cuda):
    llm, eng, cfg = _llm()
    s = dict(image=_image(3), question=QUESTIONS[1])
    llm.free_form_inference(s["image"], s["question"], max_new_tokens=8, guidance_scale=1.5, temperature=0.8, top_p=0.9, seed=23)
    got = [list(llm.generated_ids[0])]
    pairs, _ = _pairs(llm, [s])
    refs = []

    def pick(i, t, row):
        refs.append(S.sample_row(row, float(np.float32(0.8)), 50, 0.9, S.uniform(23, t)))
        return refs[-1]["token"]
    picks, _ = _replay(eng, cfg, llm.eos_token_id, pairs, got, 1.5, NO_CUT, pick)
    off = [t for t in range(len(got[0])) if picks[0][t] != got[0][t]]
    assert all(refs[t]["u_dist"] < U_EPS or refs[t]["p_dist"] < 1e-6 for t in off) and len(off) <= 1, (picks, got)
    llm.free_form_inference(s["image"], s["question"], max_new_tokens=8, guidance_scale=1.5, temperature=0.8, top_p=0.9, seed=23)
    assert [list(llm.generated_ids[0])] == got


def test_free_form_batch_guided_equals_solo_runs(cuda):
    llm, eng, cfg = _llm()
    samples = [dict(image=_image(4 + i), question=QUESTIONS[i]) for i in range(3)]
    llm.free_form_batch(samples, 8, guidance_scale=1.5, plausibility_beta=0.1)
    batch = [list(o) for o in llm.generated_ids]
    for i, s in enumerate(samples):
        llm.free_form_inference(s["image"], s["question"], max_new_tokens=8, guidance_scale=1.5, plausibility_beta=0.1)
        assert list(llm.generated_ids[0]) == batch[i], i
    with pytest.raises(ValueError, match="KV slots"):
        llm.free_form_batch(samples * 2, 8, guidance_scale=1.5)


@pytest.mark.parametrize("negative", [None, "ids"])
def test_generate_guided_equals_host_replay(cuda, negative):
    from vstar_amd.api import LlavaSearchModel
    llm, eng, cfg = _llm()
    model = LlavaSearchModel(llm)
    image = _image(6)
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + QUESTIONS[4]), llm.tokenizer)).unsqueeze(0)
    pix = llm.image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0]
    neg_ids = None if negative is None else torch.tensor([[1, 17, 44, 102, 9]])
    kw = dict(images=pix.unsqueeze(0).half(), object_features=None, images_long=None, objects_long=None, max_new_tokens=8)
    out = model.generate(input_ids, guidance_scale=2, negative_prompt_ids=neg_ids, **kw)
    L0 = input_ids.shape[1]
    assert out.dim() == 2 and (out[:, :L0] == input_ids).all()
    got = [out[0, L0:].tolist()]
    ids, rows = model._rows(input_ids, kw["images"], None, None, None)
    nrows = [ids[-1]] if negative is None else neg_ids[0].tolist()       # HF: the prompt's last token alone starts the negative context
    picks, _ = _replay(eng, cfg, llm.eos_token_id, [(rows, nrows, 0, 1)], got, 2.0, NO_CUT, lambda i, t, row: O.first_argmax(row.float().numpy()))
    assert picks == got
    assert model.generate(input_ids, **kw)[0, L0:].tolist() == model.generate(input_ids, guidance_scale=1, **kw)[0, L0:].tolist()
