"""min-p, typical-p and the epsilon / eta cutoffs of the sampled decode on the MI355X (csrc/sample_core.hpp): the
op against the CPU oracle (tests/_warp_oracle.py) bit for bit, properties that need no oracle, the band typical-p leaves, the
draw's distribution, and the engine / decode paths built on it.

Margins.  A row may differ from the oracle only where the oracle's smallest comparison margin is below W.MARGIN = 1e-5 — derived,
not measured: the device masses carry up to 2^-23 relative error (fp32 expf, then the 2^-40 rounding), |l| <= 28.4 wherever a mass
is non-zero, so E_p[l] and H are good to about 3.4e-6 nats; 1e-5 covers that and the 1e-6 of the top-p boundary.  Draws keep U_EPS =
1e-5.  At most 0.1 % of the rows may be excused; tests/test_warp_oracle.py checks on the CPU that the cases leave that room."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sampling_oracle as S
from tests import _warp_cases as C
from tests import _warp_oracle as W
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.vqa import VQA_LLM, _with_step, sampling_params, warper_params
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu
U_EPS = 1e-5


def _dt(x):
    return _lib.F16 if x.dtype == torch.float16 else _lib.BF16


def _warpers(ws, rows):
    if ws is None:
        return None, None
    arr = (_lib.VqaWarpers * rows)(*ws)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def op_sample_warp(lib, x_dev, params, warpers, vocab=None, mask=True):
    """vstar_vqa_op_sample_warp on device rows x_dev [rows, ld]: (tokens, u, n_kept, kept mask bool [rows, vocab] or None)."""
    rows, ld = x_dev.shape
    vocab = ld if vocab is None else vocab
    assert x_dev.is_cuda and len(params) == rows and (warpers is None or len(warpers) == rows)
    prm = (_lib.VqaSampling * rows)(*params)
    _keep, wp = _warpers(warpers, rows)
    tok, u, nk = np.empty(rows, np.int32), np.empty(rows, np.float32), np.empty(rows, np.int32)
    km = np.empty((rows, vocab), np.uint8) if mask else None
    _lib.check_vqa(lib.vstar_vqa_op_sample_warp(ctypes.c_void_p(x_dev.data_ptr()), _dt(x_dev), rows, vocab, ld, ctypes.cast(prm, ctypes.c_void_p),
                                                wp, ctypes.c_void_p(tok.ctypes.data), ctypes.c_void_p(u.ctypes.data),
                                                ctypes.c_void_p(nk.ctypes.data), ctypes.c_void_p(km.ctypes.data) if mask else None))
    return tok, u, nk, (km.astype(bool) if mask else None)


def op_verify_warp(lib, x_dev, groups, draft, params, warpers, vocab=None):
    """vstar_vqa_op_verify_warp: (n_accept [n_groups], tokens [rows])."""
    rows, ld = x_dev.shape
    vocab = ld if vocab is None else vocab
    go, dr = np.ascontiguousarray(groups, np.int32), np.ascontiguousarray(draft, np.int32)
    prm = (_lib.VqaSampling * rows)(*params)
    _keep, wp = _warpers(warpers, rows)
    acc, tok = np.empty(len(go) - 1, np.int32), np.empty(rows, np.int32)
    _lib.check_vqa(lib.vstar_vqa_op_verify_warp(ctypes.c_void_p(x_dev.data_ptr()), _dt(x_dev), rows, vocab, ld, ctypes.c_void_p(go.ctypes.data),
                                                len(go) - 1, ctypes.c_void_p(dr.ctypes.data), ctypes.cast(prm, ctypes.c_void_p), wp,
                                                ctypes.c_void_p(acc.ctypes.data), ctypes.c_void_p(tok.ctypes.data)))
    return acc, tok


# ------------------------------------------------ the op against the oracle ------------------------------------------------
_TALLY = {}      # (dtype, V) -> (rows, excused) of the cases compared so far


def _compare(cuda, lib, dtype_name, V):
    """One (dtype, vocabulary) of the op test, compared once: (rows, rows excused by their margin)."""
    if (dtype_name, V) in _TALLY:
        return _TALLY[(dtype_name, V)]
    cases, ref = C.cases(dtype_name, V), C.reference(dtype_name, V)
    ld = V + 13                                  # a row stride that is not the vocabulary
    excused = 0
    for c0 in range(0, len(cases), 96):
        cs = cases[c0:c0 + 96]
        x = torch.zeros(len(cs), ld, dtype=C.DTYPES[dtype_name])
        x[:, :V] = torch.stack([c[0] for c in cs])
        params = [sampling_params(t, k, p, seed=seed, step=C.STEP, stream=3 * seed) for _, t, k, p, _, seed in cs]
        tok, u, nk, km = op_sample_warp(lib, x.to(cuda), params, [_lib.VqaWarpers(**w) for *_, w, _ in cs], vocab=V)
        for j, (_, t, k, p, w, seed) in enumerate(cs):
            r = ref[c0 + j]
            what = (dtype_name, V, c0 + j, t, k, p, w)
            assert float(u[j]) == S.uniform(seed, C.STEP, 3 * seed), what
            assert nk[j] == km[j].sum(), what
            if not np.array_equal(km[j], r["keep"]):
                diff = np.flatnonzero(km[j] != r["keep"])
                print(f"kept set differs: {what}, {diff.size} tokens, first {diff[:4]}, device {int(nk[j])} oracle {r['n_kept']}, margin {r['margin']:.3g}")
                assert r["margin"] < W.MARGIN, what
                excused += 1
                continue
            assert nk[j] == r["n_kept"], what
            if tok[j] != r["token"]:
                print(f"token differs: {what}, device {int(tok[j])} oracle {r['token']}, u_dist {r['u_dist']:.3g}")
                assert r["u_dist"] < U_EPS, what
                excused += 1
    _TALLY[(dtype_name, V)] = (len(cases), excused)
    print(f"{dtype_name} V={V}: {len(cases)} rows, {excused} excused")
    return _TALLY[(dtype_name, V)]


@pytest.mark.parametrize("V", C.VOCABS)
@pytest.mark.parametrize("dtype_name", list(C.DTYPES))
def test_op_against_oracle(cuda, lib, dtype_name, V):
    _compare(cuda, lib, dtype_name, V)


def test_op_against_oracle_excuse_budget(cuda, lib):
    """At most 0.1 % of all rows of the cases above were excused (a case that has not run yet runs here)."""
    tally = [_compare(cuda, lib, d, V) for d in C.DTYPES for V in C.VOCABS]
    rows, excused = (sum(v[i] for v in tally) for i in (0, 1))
    print(f"op vs oracle: {rows} rows, {excused} excused")
    assert excused <= 0.001 * rows


def test_op_all_off_and_null_are_the_plain_op(cuda, lib):
    g = torch.Generator().manual_seed(3)
    for V in (320, 32001, 40000):
        x = (torch.randn(8, V, generator=g) * 2).half().to(cuda)
        params = [sampling_params(0.9, [0, 50][r % 2], [1.0, 0.9][(r // 2) % 2], seed=r, step=r) for r in range(8)]
        prm = (_lib.VqaSampling * 8)(*params)
        tok, u, nk = np.empty(8, np.int32), np.empty(8, np.float32), np.empty(8, np.int32)
        _lib.check_vqa(lib.vstar_vqa_op_sample(ctypes.c_void_p(x.data_ptr()), _lib.F16, 8, V, V, ctypes.cast(prm, ctypes.c_void_p),
                                               ctypes.c_void_p(tok.ctypes.data), ctypes.c_void_p(u.ctypes.data), ctypes.c_void_p(nk.ctypes.data)))
        for ws in (None, [_lib.VqaWarpers(**C.OFF)] * 8):
            for mask in (False, True):
                t2, u2, n2, km = op_sample_warp(lib, x, params, ws, mask=mask)
                assert (t2 == tok).all() and (u2 == u).all() and (n2 == nk).all()
                assert km is None or (km.sum(1) == nk).all()


def test_op_rejects_bad_values_naming_the_field(cuda, lib):
    x = torch.zeros(1, 8, dtype=torch.float16, device=cuda)
    p = [sampling_params(1.0, 0, None)]
    bad = [("min_p", float("nan")), ("min_p", -0.1), ("min_p", 1.5), ("typical_p", 0.0), ("typical_p", -1.0), ("typical_p", float("nan")),
           ("epsilon_cutoff", 1.0), ("epsilon_cutoff", -1e-3), ("eta_cutoff", 1.0), ("eta_cutoff", float("nan"))]
    for field, v in bad:
        w = _lib.VqaWarpers(**{**C.OFF, field: v})
        with pytest.raises(_lib.VstarError, match=field):
            op_sample_warp(lib, x, p, [w])
        with pytest.raises(_lib.VstarError, match=field):
            op_verify_warp(lib, x, [0, 1], [-1], p, [w])
    op_sample_warp(lib, x, p, [_lib.VqaWarpers(min_p=1.0, typical_p=5.0, epsilon_cutoff=0.0, eta_cutoff=0.999)])


# ------------------------------------------------ the band ------------------------------------------------
def _band_row(V=4096):
    """Two dominant tokens and a long flat tail that holds most of the mass: the mean log-score lies in the tail, so typical-p
    drops the arg-max (and the runner-up)."""
    x = torch.zeros(V)
    x[5], x[9] = 6.0, 5.5
    return x.half()


def test_band_drops_the_argmax_in_draw_and_verify(cuda, lib):
    x = _band_row()
    V = x.numel()
    w = dict(C.OFF, typical_p=0.5)
    ref = W.warp_row(x, 1.0, 0, 1.0, 0.5, **w)
    assert not ref["keep"][5] and not ref["keep"][9] and ref["n_kept"] == V - 2 and ref["margin"] > 1e-3      # the construction
    xd = x[None].expand(250, V).contiguous().to(cuda)
    wr = [_lib.VqaWarpers(**w)] * 250
    for launch in range(8):                      # 2000 seeded draws
        params = [sampling_params(1.0, 0, None, seed=99, step=launch * 250 + r) for r in range(250)]
        tok, _, nk, km = op_sample_warp(lib, xd, params, wr, mask=launch == 0)
        assert (nk == V - 2).all() and not np.isin(tok, (5, 9)).any()
        if km is not None:
            assert (km == ref["keep"][None]).all()
        # as a draft the dropped arg-max is never accepted; a kept draft sometimes is, and then it is the row's token
        groups = np.arange(0, 251, 2)            # 125 groups of two rows: [draft, -1]
        draft = np.tile(np.array([5, -1], np.int32), 125)
        acc, vt = op_verify_warp(lib, xd, groups, draft, params, wr)
        assert (acc == 0).all() and not np.isin(vt[vt >= 0], (5, 9)).any()
    # without the warper the same draft is accepted now and then (the test above is not vacuous)
    acc, _ = op_verify_warp(lib, xd, groups, draft, params, None)
    assert acc.sum() > 0


# ------------------------------------------------ the distribution ------------------------------------------------
def _chi_square(counts, q, n):
    scipy_stats = pytest.importorskip("scipy.stats")
    assert counts[q == 0].sum() == 0
    exp = q * n
    big = exp >= 5
    obs = np.append(counts[big], counts[~big].sum())
    ex = np.append(exp[big], exp[~big].sum())
    if ex[-1] == 0:
        obs, ex = obs[:-1], ex[:-1]
    stat, pval = scipy_stats.chisquare(obs, ex)
    print(f"chi-square over {len(obs)} bins, {n} draws: stat {stat:.1f}, p {pval:.4f}")
    assert pval > 1e-4                           # the level of test_sampling_gpu.test_draw_distribution_chi_square


def test_draw_and_verify_distribution_chi_square_under_typical_p(cuda, lib):
    g = torch.Generator().manual_seed(21)
    V = 200
    x = (torch.randn(V, generator=g) * 2).half()
    w = dict(C.OFF, typical_p=0.7)
    ref = W.warp_row(x, 0.8, 0, 1.0, 0.5, **w)
    assert ref["margin"] > W.MARGIN and 1 < ref["n_kept"] < V
    q = ref["q"]
    xd = x[None].expand(256, V).contiguous().to(cuda)
    wr = [_lib.VqaWarpers(**w)] * 256
    y = int(np.argmax(q))                        # the draft of the verify half: the likeliest kept token
    groups, draft = np.arange(0, 257, 2), np.tile(np.array([y, -1], np.int32), 128)
    counts, vcounts, n, nv = np.zeros(V, np.int64), np.zeros(V, np.int64), 0, 0
    for launch in range(79):                     # 20224 draws, rows differing only in `step`
        params = [sampling_params(0.8, 0, None, seed=1234, step=launch * 256 + r) for r in range(256)]
        tok, _, nk, _ = op_sample_warp(lib, xd, params, wr, mask=False)
        assert (nk == ref["n_kept"]).all()
        np.add.at(counts, tok, 1)
        n += 256
        acc, vt = op_verify_warp(lib, xd, groups, draft, params, wr)      # the first row of every group: P(token = y) = m_y / Z
        first = vt[0::2]
        assert ((first == y) == (acc == 1)).all()
        np.add.at(vcounts, first, 1)
        nv += 128
    _chi_square(counts, q, n)
    _chi_square(vcounts, q, nv)


# ------------------------------------------------ the engine ------------------------------------------------
_ENGINES = {}


def _engine(kind):
    """tiny: the default tiny geometry; q: the same with int4 decode weights and the block-scaled fp8 KV cache."""
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


WARP = dict(min_p=0.02, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=6e-4)


def _edits_for(n_rows, V):
    from vstar_amd.logits import LogitRules
    rules = LogitRules(repetition_penalty=1.3, bad_words_ids=[[7], [11]])
    return LogitRules.pack([rules.plan(list(range(3, 40)), 0, 2, j) for j in range(n_rows)]), rules


@pytest.mark.parametrize("kind", ["tiny", "q"])
def test_engine_calls_equal_the_ops_on_the_same_logits(cuda, lib, kind):
    eng, cfg = _engine(kind)
    V = cfg.llm_vocab
    prompts = _prompts(3, 50)
    pre = [Seq(p, kv_slot=i) for i, p in enumerate(prompts)]
    want = [(i, -1) for i in range(3)]
    w = warper_params(**WARP)
    params = [sampling_params(0.9, 50, 0.95, seed=70 + i, step=2) for i in range(3)]
    plain = eng.forward_sample(pre, want, params)
    for with_edits in (False, True):
        for lp in (None, 3):
            edits, _ = _edits_for(3, V) if with_edits else (None, None)
            lg, _ = eng.forward(pre, want)                                   # the unedited logits of the same call
            xd = torch.from_numpy(lg).to(cuda)
            if with_edits:
                off, tok, pen = edits
                _lib.check_vqa(lib.vstar_vqa_op_edit(ctypes.c_void_p(xd.data_ptr()), _lib.F16, 3, V, V, ctypes.c_void_p(off.ctypes.data),
                                                     ctypes.c_void_p(tok.ctypes.data), ctypes.c_void_p(pen.ctypes.data)))
            t_op, _, nk, _ = op_sample_warp(lib, xd, params, [w] * 3, mask=False)
            got = eng.forward_sample(pre, want, params, edits=edits, logprobs=lp, warpers=w)
            rec = None
            if lp is not None:
                got, rec = got
                unwarped = eng.forward_sample(pre, want, params, edits=edits, logprobs=lp)[1]
                # (§8.9: the log-probabilities stay those of the un-warped row: the top-n lists do not depend on the warpers)
                assert np.array_equal(rec.top_token, unwarped.top_token) and np.array_equal(rec.top_logprob, unwarped.top_logprob)
            assert got.tolist() == t_op.tolist(), (kind, with_edits, lp)
            assert (nk < 50).any()                                           # the warpers did cut something
            # the verify tail: every sequence continues with [its token, two drafts]
            step = [Seq([int(got[i]), 5 + i, 9], kv_slot=i, past_len=len(prompts[i])) for i in range(3)]
            wanted = [(i, r) for i in range(3) for r in range(3)]
            groups, draft = [0, 3, 6, 9], [5, 9, -1, 6, 9, -1, 7, 9, -1]
            vp = [_with_step(params[i], 3 + r) for i in range(3) for r in range(3)]
            ved, _ = _edits_for(9, V) if with_edits else (None, None)
            lg, _ = eng.forward(step, wanted)
            xd = torch.from_numpy(lg).to(cuda)
            if with_edits:
                off, tok, pen = ved
                _lib.check_vqa(lib.vstar_vqa_op_edit(ctypes.c_void_p(xd.data_ptr()), _lib.F16, 9, V, V, ctypes.c_void_p(off.ctypes.data),
                                                     ctypes.c_void_p(tok.ctypes.data), ctypes.c_void_p(pen.ctypes.data)))
            a_op, t_op = op_verify_warp(lib, xd, groups, draft, vp, [w] * 9)
            res = eng.forward_verify(step, wanted, groups, draft, vp, edits=ved, logprobs=lp, warpers=w)
            assert res[0].tolist() == a_op.tolist() and res[1].tolist() == t_op.tolist(), (kind, with_edits, lp)
    # all-off records and warpers=None are the plain call; a plain call after warped ones gives its old bits
    off_rec = _lib.VqaWarpers(**C.OFF)
    assert eng.forward_sample(pre, want, params, warpers=off_rec).tolist() == plain.tolist()
    assert eng.forward_sample(pre, want, params, warpers=None).tolist() == plain.tolist()
    assert eng.forward_sample(pre, want, params).tolist() == plain.tolist()
    # bad values fail before any device work and leave the engine usable
    for field, v in (("min_p", 2.0), ("typical_p", 0.0), ("epsilon_cutoff", 1.0), ("eta_cutoff", float("nan"))):
        with pytest.raises(_lib.VstarError, match=field):
            eng.forward_sample(pre, want, params, warpers=_lib.VqaWarpers(**{**C.OFF, field: v}))
    assert eng.forward_sample(pre, want, params).tolist() == plain.tolist()


def _llm():
    eng, cfg = _engine("tiny")
    return VQA_LLM(cfg=cfg, engine=eng), eng, cfg


def _samples(n):
    from PIL import Image
    rng = np.random.default_rng(9)
    image = Image.fromarray(rng.integers(0, 256, (300, 420, 3), dtype=np.uint8))
    qs = ["What is in the picture?", "Describe it.", "Where is the cup?"]
    return [dict(image=image, question=qs[i % 3]) for i in range(n)]


def test_min_p_one_and_epsilon_near_one_are_the_greedy_decode(cuda):
    llm, _, _ = _llm()
    samples = _samples(2)
    llm.free_form_batch(samples, max_new_tokens=8)
    greedy = [list(x) for x in llm.generated_ids]
    for kw in (dict(min_p=1.0), dict(epsilon_cutoff=0.999999)):
        llm.free_form_batch(samples, max_new_tokens=8, temperature=1, top_k=0, seed=5, **kw)
        assert [list(x) for x in llm.generated_ids] == greedy, kw
    # temperature 0 ignores the warpers, as it ignores top_p
    llm.free_form_batch(samples, max_new_tokens=8, typical_p=0.2, min_p=0.5)
    assert [list(x) for x in llm.generated_ids] == greedy
    with pytest.raises(ValueError):
        llm.free_form_batch(samples, max_new_tokens=8, temperature=1, typical_p=0.0)


@pytest.mark.parametrize("kw", [dict(min_p=0.3), dict(typical_p=0.5), dict(epsilon_cutoff=0.01), dict(eta_cutoff=0.05)], ids=lambda k: next(iter(k)))
def test_every_sampled_token_satisfies_its_stage_rule(cuda, kw):
    """Recomputed from the engine's own logits of each step: the rule of the one active stage, with the oracle's margins as slack."""
    llm, eng, cfg = _llm()
    s = _samples(1)[0]
    llm.free_form_inference(s["image"], s["question"], temperature=1.0, top_k=0, max_new_tokens=10, seed=11, **kw)
    ids = list(llm.generated_ids[0])
    img_slots, _ = llm._encode(s["image"], None, 0)
    _, rows = llm._question_rows(s["question"], img_slots, [], None, None)
    lg, _ = eng.forward([Seq(rows, kv_slot=1)], [(0, -1)])
    cut = 0
    for t, tok in enumerate(ids):
        sc = S.scaled_scores(torch.from_numpy(lg[0]), 1.0)
        keep, mg = W.warp(sc, np.ones(sc.size, bool), **kw)
        cut += int(keep.sum() < sc.size)
        m = W.fixed_masses(sc)
        Z = m.sum()
        if "min_p" in kw:
            assert m[tok] >= 0.3 * m.max() * (1 - W.MARGIN)
        elif "epsilon_cutoff" in kw:
            assert m[tok] >= 0.01 * Z * (1 - W.MARGIN) or tok == int(np.argmax(sc))
        else:
            assert keep[tok] or W.margin(mg) < W.MARGIN, (t, tok)
        if t + 1 < len(ids):
            lg, _ = eng.forward([Seq([tok], kv_slot=1, past_len=len(rows) + t)], [(0, 0)])
    assert cut > 0                               # the stage did restrict the draws


def test_speculative_decode_with_typical_p_equals_op_verify_on_its_calls(cuda, lib):
    """Every verify call `speculative_decode(..., typical_p=...)` makes is replayed on other KV slots with the logits brought back;
    op_verify_warp on those logits must return the call's accepted counts and tokens."""
    llm, eng, cfg = _llm()
    n, max_new = 2, 10
    prompts = _prompts(n, 90)
    lens = [len(p) for p in prompts]
    params = [sampling_params(0.7, 50, None, seed=40 + i) for i in range(n)]
    kw = dict(typical_p=0.6, min_p=0.01)
    w = warper_params(**kw)
    seqs = lambda s0: [Seq(p, kv_slot=s0 + i) for i, p in enumerate(prompts)]      # noqa: E731
    ref = llm.sample_decode(seqs(0), lens, max_new, params, **kw)                  # the drafter replays the plain sampled decode

    def drafter(ids, k):
        for i in range(n):
            if ids[:lens[i]] == prompts[i]:
                done = len(ids) - lens[i]
                guess = ref[i][done:done + k]
                return [g if j != 1 else (g + 1) % cfg.llm_vocab for j, g in enumerate(guess)]      # the second draft is wrong
        return []

    calls = []
    real = eng.forward_verify

    def spy(step, wanted, groups, draft, prm=None, **rest):
        out = real(step, wanted, groups, draft, prm, **rest)
        calls.append((step, wanted, list(groups), list(draft), prm, rest, out))
        return out

    eng.forward_verify = spy
    try:
        got = llm.speculative_decode(seqs(0), lens, prompts, max_new, 3, params, drafter, **kw)
    finally:
        del eng.forward_verify
    assert calls and llm.spec_stats["drafted"] > 0
    # the first tokens: the plain warped draw of the prefill
    assert [g[0] for g in got] == [r[0] for r in ref]
    eng.forward(seqs(2), [(i, -1) for i in range(n)], logits=False)                # the prompts into slots 2, 3
    for step, wanted, groups, draft, prm, rest, out in calls:
        assert rest.get("warpers") is not None
        mirror = [Seq(s.rows, kv_slot=s.kv_slot + 2, past_len=s.past_len) for s in step]
        lg, _ = eng.forward(mirror, wanted)
        a_op, t_op = op_verify_warp(lib, torch.from_numpy(lg).to(cuda), groups, draft, prm, [w] * len(wanted))
        assert out[0].tolist() == a_op.tolist() and out[1].tolist() == t_op.tolist()
    for i in range(n):
        assert 1 <= len(got[i]) <= max_new


def test_generate_takes_the_warpers(cuda):
    from vstar_amd import vqa
    from vstar_amd.api import load_pretrained_model
    cfg = VQAConfig.tiny()
    sd = random_state_dict(cfg, seed=0, dtype=torch.float16)
    tokenizer, model, image_processor, _ = load_pretrained_model("seal_vqa_7b", None, "seal_vqa_7bllava", cfg=cfg, state_dict=sd)
    llm = vqa.VQA_LLM(cfg=cfg, engine=model.engine)
    s = _samples(1)[0]
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + s["question"]), tokenizer)).unsqueeze(0)
    image_tensor = image_processor.preprocess(s["image"], return_tensors="pt")["pixel_values"][0]
    kw = dict(images=image_tensor.unsqueeze(0).half(), object_features=None, images_long=None, objects_long=None, num_beams=1,
              max_new_tokens=6, use_cache=True)
    greedy = model.generate(input_ids, do_sample=False, **kw)
    out = model.generate(input_ids, do_sample=True, temperature=1.0, top_k=0, min_p=1.0, seed=3, **kw)
    assert out.tolist() == greedy.tolist()
    out = model.generate(input_ids, do_sample=True, temperature=0.8, typical_p=0.5, eta_cutoff=1e-3, seed=17, **kw)
    llm.free_form_inference(s["image"], s["question"], temperature=0.8, typical_p=0.5, eta_cutoff=1e-3, max_new_tokens=6, seed=17)
    assert out[0, input_ids.shape[1]:].tolist() == list(llm.generated_ids[0])
    assert model.generate(input_ids, do_sample=False, typical_p=0.5, **kw).tolist() == greedy.tolist()
    with pytest.raises(ValueError):
        model.generate(input_ids, do_sample=True, temperature=0.8, epsilon_cutoff=1.0, **kw)
