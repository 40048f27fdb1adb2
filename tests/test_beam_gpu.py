"""Beam search on the MI355X (csrc/beam.hip, the KV ancestry table, vstar_amd/beam.py): the select op against
the CPU oracle (tests/_beam_oracle.py), ancestry reorder against a physically copied cache, slot reuse, the VQA-LLM beam decode
against the oracle loop fed with the engine's own logits, and the public entry points."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _beam_oracle as O
from vstar_amd import _lib

pytestmark = pytest.mark.gpu
EOS_SCALE = 8.0


def op_select(lib, x_dev, scores, goff, n_cand, vocab=None, want_lp=True):
    rows, ld = x_dev.shape
    vocab = ld if vocab is None else vocab
    sc = np.ascontiguousarray(scores, np.float32)
    go = np.ascontiguousarray(goff, np.int32)
    ng = len(go) - 1
    cs, ct, cr = np.empty((ng, n_cand), np.float32), np.empty((ng, n_cand), np.int32), np.empty((ng, n_cand), np.int32)
    lp = np.empty((rows, vocab), np.float32) if want_lp else None
    dt = _lib.F16 if x_dev.dtype == torch.float16 else _lib.BF16
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None       # noqa: E731
    _lib.check_vqa(lib.vstar_vqa_op_beam_select(ctypes.c_void_p(x_dev.data_ptr()), dt, rows, vocab, ld, p(sc), ng, p(go), n_cand,
                                                p(cs), p(ct), p(cr), p(lp)))
    return cs, ct, cr, lp


def make_row(kind, V, g):
    x = torch.randn(V, generator=g) * 3
    if kind == "peaked":
        x = torch.randn(V, generator=g)
        x[int(torch.randint(0, V, (1,), generator=g))] += 15
    elif kind == "flat":
        x = torch.full((V,), 1.5)
    elif kind == "masked":
        m = torch.rand(V, generator=g) < 0.5
        x = torch.where(m, torch.where(torch.rand(V, generator=g) < 0.5, -float("inf"), -65504.0), x)
        x[0] = 2.0
    return x


def lp_matches_exact(lp_dev, x, dtype):
    """Device lp == float64-exact log_softmax rounded once to dtype, except within 1e-6 relative of a rounding midpoint."""
    x64 = x.double()
    ex = x64 - torch.logsumexp(x64, -1, keepdim=True)
    ref = O.round_once(ex, dtype).double()
    dev = torch.from_numpy(lp_dev).double()
    bad = ~((dev == ref) | (torch.isnan(dev) & torch.isnan(ref)))
    if not bad.any():
        return 0
    mid = (dev[bad] + ref[bad]) / 2
    assert ((ex[bad] - mid).abs() <= 1e-6 * ex[bad].abs()).all(), (dev[bad][:4], ref[bad][:4], ex[bad][:4])
    return int(bad.sum())


def test_op_against_oracle(cuda, lib):
    kinds = ("random", "peaked", "flat", "masked")
    n_cmp = n_mid = 0
    for dtype in (torch.float16, torch.bfloat16):
        for V in (2, 320, 32000, 32001, 131075):
            g = torch.Generator().manual_seed(V)
            for k in (1, 2, 4, 8, 16):
                if V >= 32000 and k in (2, 4):
                    continue
                groups = 2
                rows = [make_row(kinds[(r + k) % 4], V, g) for r in range(groups * k)]
                x = torch.stack(rows).to(dtype)
                scores = torch.randn(groups * k, generator=g) * 5
                scores[1::3] = -1e9                              # start rows
                if k >= 2:
                    scores[:k] = 1.0e4 + torch.randint(0, 3, (k,), generator=g).float()    # ties after the fp32 add
                ld = V + 5
                xd = torch.zeros(groups * k, ld, dtype=dtype)
                xd[:, :V] = x
                goff = [0, k, 2 * k]
                cs, ct, cr, lp = op_select(lib, xd.to(cuda), scores.numpy(), goff, 2 * k, vocab=V)
                n_mid += lp_matches_exact(lp, x.float(), dtype)
                lpt = torch.from_numpy(lp).to(dtype)
                for gi in range(groups):
                    sl = slice(goff[gi], goff[gi + 1])
                    s, t, r = O.candidates(lpt[sl], scores[sl].float(), 2 * k)
                    assert np.array_equal(s.numpy().view(np.int32), cs[gi].view(np.int32)), (dtype, V, k, gi, s, cs[gi])
                    assert t.tolist() == ct[gi].tolist() and r.tolist() == cr[gi].tolist(), (dtype, V, k, gi)
                    n_cmp += 1
    print(f"beam select vs oracle: {n_cmp} groups bit-identical; {n_mid} lp at a rounding midpoint")


def test_op_tie_rule_and_errors(cuda, lib):
    # every token of a -1e9 row collapses onto one score: the lowest flat indices win
    x = torch.randn(3, 320).half()
    cs, ct, cr, _ = op_select(lib, x.to(cuda), [-1e9] * 3, [0, 3], 6)
    s, t, r = O.candidates(O.log_probs(x), torch.full((3,), -1e9), 6)
    assert ct[0].tolist() == t.tolist() and cr[0].tolist() == r.tolist()
    assert len(set(cs[0].tolist())) <= 2
    # repeated rows (the start of a search): candidates of beam 0 first
    y = torch.randn(1, 320).half().repeat(4, 1)
    cs, ct, cr, _ = op_select(lib, y.to(cuda), [0, -1e9, -1e9, -1e9], [0, 4], 8)
    s, t, r = O.candidates(O.log_probs(y), torch.tensor([0, -1e9, -1e9, -1e9]), 8)
    assert (cr[0] == 0).all() and ct[0].tolist() == t.tolist() and r.tolist() == [0] * 8
    xd = torch.zeros(2, 8, dtype=torch.float16, device=cuda)
    for args in (([0, 0], [0, 2], 33), ([0, 0], [0, 1], 2), ([0, float("nan")], [0, 2], 2), ([0, 0], [0, 2], 17)):
        with pytest.raises(_lib.VstarError):
            op_select(lib, xd, *args)
    with pytest.raises(_lib.VstarError):                        # V = 1: 2k candidates > k x V
        op_select(lib, torch.zeros(2, 1, dtype=torch.float16, device=cuda), [0, -1e9], [0, 2], 4)


# ------------------------------------------------ the engine ------------------------------------------------
_ENG = {}


def _engine(max_slots=24):
    """A tiny VQA engine of its own (fresh slots), its lm_head EOS row scaled so that hypotheses finish mid-run."""
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa_engine import VqaEngine
    from vstar_amd.weights import random_state_dict
    if max_slots not in _ENG:
        cfg = VQAConfig.tiny(max_slots=max_slots)
        sd = random_state_dict(cfg, seed=3, dtype=torch.float16)
        sd["lm_head.weight"][2] = (sd["lm_head.weight"][2].float() * EOS_SCALE).half()
        eng = VqaEngine(cfg, 0)
        eng.load_state_dict(sd)
        _ENG[max_slots] = (eng, cfg)
    return _ENG[max_slots]


def _prompt(eng, seed=31, n_text=40):
    g = torch.Generator().manual_seed(seed)
    eng.encode_images(torch.randn(1, 3, 224, 224, generator=g), 0)
    ids = [1] + torch.randint(3, 300, (n_text,), generator=g).tolist()
    ids[2] = -200
    return eng.expand_ids(ids, [0], [], None, None)


@pytest.mark.parametrize("k", [2, 8])
def test_ancestry_equals_physical_copy(cuda, k):
    from vstar_amd.vqa_engine import Seq
    eng, cfg = _engine()
    rows = _prompt(eng)
    P = len(rows)
    A, M, S = list(range(k)), list(range(k, 2 * k)), list(range(2 * k, 3 * k))     # ancestral, mirror, scratch
    la, _ = eng.forward([Seq(rows, kv_slot=A[0])], [(0, -1)])
    lm, _ = eng.forward([Seq(rows, kv_slot=M[0])], [(0, -1)])
    assert np.array_equal(la.view(np.uint16), lm.view(np.uint16))
    eng.kv_reorder(A[1:], [A[0]] * (k - 1), 0, P)
    for b in range(1, k):
        eng.kv_copy(M[b], M[0], 0, P)
    rng = np.random.default_rng(k)
    pos = P
    schedule = []
    for step in range(7):
        toks = rng.integers(3, 300, k).tolist()
        la, _ = eng.forward([Seq([toks[b]], kv_slot=A[b], past_len=pos) for b in range(k)], [(b, 0) for b in range(k)])
        lm, _ = eng.forward([Seq([toks[b]], kv_slot=M[b], past_len=pos) for b in range(k)], [(b, 0) for b in range(k)])
        assert np.array_equal(la.view(np.uint16), lm.view(np.uint16)), (k, step)
        pos += 1
        if step % 3 == 0:
            par = list(reversed(range(k)))                     # swaps
        elif step % 3 == 1:
            par = [0] * (k // 2) + list(range(k - k // 2))     # one parent feeds several children; the last beams drop out
        else:
            par = rng.integers(0, k, k).tolist()
        schedule.append(par)
        eng.kv_reorder(A, [A[p] for p in par], 0, pos)
        for b in range(k):
            eng.kv_copy(S[b], M[par[b]], 0, pos)
        for b in range(k):
            eng.kv_copy(M[b], S[b], 0, pos)
    # a multi-row continuation of the ancestral slots (the non-fused cached path)
    cont = [rng.integers(3, 300, 3).tolist() for _ in range(k)]
    la, _ = eng.forward([Seq(cont[b], kv_slot=A[b], past_len=pos) for b in range(k)], [(b, t) for b in range(k) for t in range(3)])
    lm, _ = eng.forward([Seq(cont[b], kv_slot=M[b], past_len=pos) for b in range(k)], [(b, t) for b in range(k) for t in range(3)])
    assert np.array_equal(la.view(np.uint16), lm.view(np.uint16))
    pos += 3
    # one call that continues the ancestral beams AND forks a plain prefix into a slot (the fork reads through the table too):
    # the call equals, bit for bit, the same call on the physically copied slots, and the fork's logits equal the same fork alone.
    # (The beams alone are a single-row call: it takes the fused split-KV kernels, whose fp32 sums run in another order than the
    # un-fused kernel's of the mixed call — equal bits across the two are no property of the kernels, only the house logits tolerance.)
    fork = rng.integers(3, 300, 3).tolist()
    toks = rng.integers(3, 300, k).tolist()
    want = [(b, 0) for b in range(k)] + [(k, t) for t in range(3)]
    la, _ = eng.forward([Seq([toks[b]], kv_slot=A[b], past_len=pos) for b in range(k)] + [Seq(fork, kv_slot=S[0], past_len=pos,
                        prefix_slot=M[0])], want)
    lm, _ = eng.forward([Seq([toks[b]], kv_slot=M[b], past_len=pos) for b in range(k)] + [Seq(fork, kv_slot=S[1], past_len=pos,
                        prefix_slot=M[0])], want)
    ls, _ = eng.forward([Seq([toks[b]], kv_slot=M[b], past_len=pos) for b in range(k)], [(b, 0) for b in range(k)])
    lf, _ = eng.forward([Seq(fork, kv_slot=S[1], past_len=pos, prefix_slot=M[0])], [(0, t) for t in range(3)])
    assert np.array_equal(la.view(np.uint16), lm.view(np.uint16))
    assert np.array_equal(la[k:].view(np.uint16), lf.view(np.uint16))
    d, s = la[:k].astype(np.float64) - ls.astype(np.float64), ls.astype(np.float64)
    assert np.linalg.norm(d) <= 1e-3 * np.linalg.norm(s)
    # forking FROM a reordered slot is refused (its positions are scattered over other slots)
    with pytest.raises(_lib.VstarError):
        eng.forward([Seq([5], kv_slot=A[1], past_len=pos, prefix_slot=A[0])], [(0, 0)])


def test_ancestry_without_split_kv(cuda):
    """The ancestry test with VSTAR_DECODE_SPLIT_KV=0 (read once per process): k = 2 then takes the fused ANC kernel too."""
    import os
    import subprocess
    import sys
    if os.environ.get("VSTAR_DECODE_SPLIT_KV") == "0":
        pytest.skip("already the split-off process")
    env = dict(os.environ, VSTAR_DECODE_SPLIT_KV="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-m", "pytest", "-q", "-p", "no:cacheprovider",
                        "tests/test_beam_gpu.py::test_ancestry_equals_physical_copy"], cwd=root, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_beam_search_then_option_scoring_and_forks(cuda):
    """Beam search leaves its slots reordered; the evaluation's next calls on the same engine — multiple_choices_inference /
    option_losses and a forked LlavaSearchModel.__call__ — fork INTO those slots and must equal the same calls on a fresh
    engine."""
    from vstar_amd import vqa
    from vstar_amd.api import LlavaSearchModel
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa_engine import VqaEngine
    from vstar_amd.weights import random_state_dict
    llm, cfg = _llm()
    cfg2 = VQAConfig.tiny(max_slots=24)
    sd = random_state_dict(cfg2, seed=3, dtype=torch.float16)
    sd["lm_head.weight"][2] = (sd["lm_head.weight"][2].float() * EOS_SCALE).half()
    fresh_eng = VqaEngine(cfg2, 0)
    fresh_eng.load_state_dict(sd)
    fresh = vqa.VQA_LLM(cfg=cfg2, engine=fresh_eng)
    img, q = _image(1), QUESTIONS[2]
    options = ["red", "The mug is blue.", "green and white", "yellow"]
    llm.free_form_inference(img, q, num_beams=8, max_new_tokens=6)             # slots 0 .. 7 reordered
    a = llm.option_losses(img, q, options)
    b = fresh.option_losses(img, q, options)
    assert [x.view(torch.int16).item() for x in a] == [x.view(torch.int16).item() for x in b]
    assert llm.multiple_choices_inference(img, q, options) == fresh.multiple_choices_inference(img, q, options)
    outs = []
    for m in (llm, fresh):
        m.free_form_inference(img, q, num_beams=4, max_new_tokens=4)
        model = LlavaSearchModel(m)
        ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), m.tokenizer)).unsqueeze(0)
        pix = m.image_processor.preprocess(img, return_tensors="pt")["pixel_values"][0].unsqueeze(0).half()
        out_q = model(ids, use_cache=True, images=pix, object_features=None)
        opt = torch.tensor([[5, 6, 7, 8]])
        out_o = model(input_ids=opt, use_cache=True, past_key_values=out_q.past_key_values)
        outs.append((out_q.logits[0, -1:].clone(), out_o.logits[0].clone()))
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
    assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16))


def test_reordered_slot_reuse(cuda):
    from vstar_amd.vqa_engine import Seq
    eng, cfg = _engine()
    rows = _prompt(eng, seed=5)
    P = len(rows)
    eng.forward([Seq(rows, kv_slot=0)], [(0, -1)])
    eng.kv_reorder([1, 2], [0, 0], 0, P)
    eng.forward([Seq([7], kv_slot=1, past_len=P), Seq([8], kv_slot=2, past_len=P)], [(0, 0), (1, 0)])
    eng.kv_reorder([1, 2], [2, 1], 0, P + 1)

    def greedy(slot):
        lg, nx = eng.forward([Seq(rows, kv_slot=slot)], [(0, -1)])
        out = [lg]
        for t in range(6):
            lg, nx = eng.forward([Seq([int(nx[0])], kv_slot=slot, past_len=P + t)], [(0, 0)])
            out.append(lg)
        return np.stack(out)
    a, b = greedy(1), greedy(cfg.max_slots - 1)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


class _Recorder:
    """Records every forward_beam of the engine (with the logits rows) during a decode."""

    def __init__(self, eng):
        self.eng, self.calls = eng, []

    def __enter__(self):
        orig = type(self.eng).forward_beam

        def fb(seqs, want, scores, goff, n_cand, logits=False):
            out = orig(self.eng, seqs, want, scores, goff, n_cand, logits=True)
            self.calls.append(out)
            return out
        self.eng.forward_beam = fb
        return self

    def __exit__(self, *a):
        del self.eng.forward_beam


class _Diverged(Exception):
    pass


def replay(calls, k, prompt_len, eos, max_new, **kw):
    """The oracle loop fed with the recorded logits: at every step the oracle's candidates must be the device's (else the
    rank-2k boundary must be within 1e-6: excused, comparison stops).  Returns (oracle output or None, excused, finished)."""
    trace = []
    finished = 0

    def check(t):
        nonlocal finished
        lp, bsc, (s, tok, row) = trace[t]
        cs, ct, cr, _ = calls[t]
        if not (np.array_equal(s.numpy().view(np.int32), cs[0].view(np.int32)) and tok.tolist() == ct[0].tolist()
                and row.tolist() == cr[0].tolist()):
            assert O.boundary_gap(lp, bsc, 2 * k) < 1e-6, (t, s, cs[0], tok, ct[0], row, cr[0])
            raise _Diverged()
        finished += int(sum(1 for r in range(k) if int(tok[r]) == eos))

    def fn(hist):
        t = len(trace)
        if t:
            check(t - 1)
        assert t < len(calls), "the oracle runs longer than the device"
        return torch.from_numpy(calls[t][3].copy())
    try:
        out = O.beam_search(fn, k, prompt_len, eos, max_new, trace=trace, **kw)
        check(len(trace) - 1)
    except _Diverged:
        return None, 1, finished
    assert len(trace) == len(calls), (len(trace), len(calls))
    return out, 0, finished


def _llm():
    from vstar_amd.vqa import VQA_LLM
    eng, cfg = _engine()
    return VQA_LLM(cfg=cfg, engine=eng), cfg


def _image(seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, (300, 420, 3), dtype=np.uint8))


def _prompt_len(llm, q):
    from vstar_amd import vqa
    return len(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), llm.tokenizer))


QUESTIONS = ("What is in the picture?", "Describe it.", "What colour is the mug on the table?")


@pytest.mark.parametrize("k", [2, 4])
def test_free_form_beam_equals_oracle(cuda, k):
    llm, cfg = _llm()
    excused = finished = compared = 0
    for qi, q in enumerate(QUESTIONS):
        for max_new in (5, 24):
            img = _image(qi)
            with _Recorder(llm.engine) as rec:
                text = llm.free_form_inference(img, q, num_beams=k, max_new_tokens=max_new)
            got = list(llm.generated_ids[0])
            ref, exc, fin = replay(rec.calls, k, _prompt_len(llm, q), llm.eos_token_id, max_new)
            excused += exc
            finished += fin
            if ref is not None:
                assert got == ref[0], (k, q, max_new, got, ref[0])
                compared += 1
            assert isinstance(text, str)
    print(f"beam k={k}: {compared} decodes equal to the oracle, {excused} excused at the rank-2k boundary, "
          f"{finished} hypotheses finished mid-run")
    assert excused <= 1 and finished > 0


def test_free_form_batch_beams(cuda):
    llm, cfg = _llm()
    samples = [dict(image=_image(i), question=q) for i, q in enumerate(QUESTIONS)]
    texts = llm.free_form_batch(samples, max_new_tokens=12, num_beams=4)
    batch = [list(x) for x in llm.generated_ids]
    for i, s in enumerate(samples):
        one = llm.free_form_inference(s["image"], s["question"], num_beams=4, max_new_tokens=12)
        assert one == texts[i] and list(llm.generated_ids[0]) == batch[i], i
    with pytest.raises(ValueError):
        llm.free_form_batch(samples * 3, max_new_tokens=4, num_beams=4)        # 36 beams > 24 slots
    with pytest.raises(NotImplementedError):
        llm.free_form_inference(samples[0]["image"], QUESTIONS[0], temperature=0.7, num_beams=2)


def test_generate_num_beams(cuda):
    from vstar_amd import vqa
    from vstar_amd.api import LlavaSearchModel
    llm, cfg = _llm()
    model = LlavaSearchModel(llm)
    q = QUESTIONS[0]
    img = _image(0)
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), llm.tokenizer)).unsqueeze(0)
    pix = llm.image_processor.preprocess(img, return_tensors="pt")["pixel_values"][0].unsqueeze(0).half()
    kw = dict(images=pix, object_features=None, images_long=None, objects_long=None, max_new_tokens=10, use_cache=True)
    out = model.generate(input_ids, num_beams=4, **kw)
    assert out.shape[0] == 1 and (out[:, :input_ids.shape[1]] == input_ids).all()
    llm.free_form_inference(img, q, num_beams=4, max_new_tokens=10)
    assert out[0, input_ids.shape[1]:].tolist() == list(llm.generated_ids[0])
    for extra in (dict(num_return_sequences=3), dict(early_stopping=True), dict(early_stopping="never", length_penalty=2.0)):
        with _Recorder(llm.engine) as rec:
            o = model.generate(input_ids, num_beams=4, **kw, **extra)
        ref, exc, _ = replay(rec.calls, 4, input_ids.shape[1], llm.eos_token_id, 10, **extra)
        if ref is not None:
            assert [r[input_ids.shape[1]:] for r in o.tolist()] == ref, extra
        assert o.shape[0] == extra.get("num_return_sequences", 1) and (o[:, :input_ids.shape[1]] == input_ids).all()
    with pytest.raises(NotImplementedError):
        model.generate(input_ids, do_sample=True, temperature=0.8, num_beams=2, **kw)
    with pytest.raises(ValueError):
        model.generate(input_ids, num_beams=cfg.max_slots + 1, **kw)


def test_engine_rejects_bad_beam_arguments(cuda):
    from vstar_amd.vqa_engine import Seq
    eng, cfg = _engine()
    rows = _prompt(eng, seed=8)
    s = [Seq(rows, kv_slot=0)]
    for scores, goff, nc in (([0, 0], [0, 1], 4), ([0, 0], [0, 2], 33), ([0, float("nan")], [0, 2], 4), ([0, 0], [0, 1, 3], 2)):
        with pytest.raises(_lib.VstarError):
            eng.forward_beam(s, [(0, -1), (0, -1)], scores, goff, nc)
    for dst, src, lo, hi in (([1, 1], [0, 0], 0, 10), ([cfg.max_slots], [0], 0, 10), ([1], [0], 0, cfg.max_ctx + 1), ([1], [0], 5, 4)):
        with pytest.raises(_lib.VstarError):
            eng.kv_reorder(dst, src, lo, hi)
    with pytest.raises(_lib.VstarError):
        eng.kv_copy(1, 1, 0, 10)
