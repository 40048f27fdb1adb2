"""The CPU side of guided decoding: the oracle of the guidance kernel (tests/_guide_oracle.py) against the installed
transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor and against a literal restatement of the plausibility rule, the census of
the excuse band over every case the GPU door test uses, the combination checker of the public keywords, and the three new names of
the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _guide_oracle as G
from vstar_amd import _lib
from vstar_amd.vqa import check_guidance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_rounding_and_saturation():
    rng = np.random.default_rng(0)
    d = np.concatenate([rng.normal(0, 30, 20000), rng.normal(0, 1e-3, 2000), [0.0, -0.0, 65519.99, 65520.0, -1e9, 1e300, -1e300]])
    # values a hair off fp16 midpoints: rounding to fp32 first and then to fp16 would go wrong, one rounding does not
    h = rng.normal(0, 30, 4000).astype(np.float16)
    mid = (h.astype(np.float64) + np.nextafter(h, np.float16(np.inf)).astype(np.float64)) / 2
    d = np.concatenate([d, mid, mid * (1 + 1e-12), mid * (1 - 1e-12)])
    with np.errstate(over="ignore"):
        direct = d.astype(np.float16)                       # numpy rounds a double to half once
    direct = np.where(np.isinf(direct), np.copysign(np.float16(65504), direct), direct).astype(np.float16)
    assert np.array_equal(G.round16(d, False), direct.view(np.uint16))
    # bf16: against exact integer arithmetic on the double's value — the two neighbours and the tie rule
    got = G.to_f64(G.round16(d, True), True)
    lo = G.to_f64(G._step(G.round16(d, True), np.zeros(d.shape, bool)), True)
    hi = G.to_f64(G._step(G.round16(d, True), np.ones(d.shape, bool)), True)
    fin = np.abs(d) < 3.38e38
    assert (np.abs(got - d)[fin] <= np.abs(lo - d)[fin]).all() and (np.abs(got - d)[fin] <= np.abs(hi - d)[fin]).all()
    assert G.to_f64(G.round16(np.float64([1e300, -1e300]), True), True).tolist() == [float(np.float32(3.3895313892515355e38)), -float(np.float32(3.3895313892515355e38))]
    assert G.round16(np.float64([70000.0, -70000.0]), False).tolist() == [0x7bff, 0xfbff]


class _Out(dict):
    logits = property(lambda self: self["logits"])


def _hf_guided(xc: np.ndarray, xu: np.ndarray, gamma: float) -> np.ndarray:
    """transformers' processor on float64 tensors, the negative logits served by a stub model."""
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    neg = torch.from_numpy(xu)[None, None]

    def model(input_ids, **kw):
        return _Out(logits=neg.expand(1, input_ids.shape[1], -1))
    proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(gamma, model, unconditional_ids=torch.tensor([[1, 2, 3]]))
    return proc(torch.tensor([[5, 6]]), torch.from_numpy(xc)[None])[0].numpy()


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", [2, 65, 1000, 32001])
def test_unrounded_values_equal_transformers_in_float64(V, bf16):
    rng = np.random.default_rng(V + bf16)
    for kc, ku in (("random", "random"), ("peaked", "random"), ("flat", "peaked"), ("random", "flat")):
        bc, bu = G._row(kc, V, rng, bf16), G._row(ku, V, rng, bf16)
        for gamma in (0.0, 0.5, 1.5, 3.0):          # (at gamma == 1 the HF class returns log_softmax without the arithmetic)
            ours = G.guide_pair(bc, bu, gamma, -np.inf, bf16).g
            hf = _hf_guided(G.to_f64(bc, bf16), G.to_f64(bu, bf16), gamma)
            assert np.isfinite(ours).all()
            assert (np.abs(ours - hf) <= 1e-12 * np.maximum(1.0, np.abs(ours))).all(), (kc, ku, gamma)
        one = G.guide_pair(bc, bu, 1.0, -np.inf, bf16).g
        ls = torch.log_softmax(torch.from_numpy(G.to_f64(bc, bf16)), -1).numpy()
        assert (np.abs(one - ls) <= 1e-12 * np.maximum(1.0, np.abs(one))).all()


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
def test_plausibility_rule_equals_its_literal_restatement(bf16):
    checked = 0
    for seed in range(40):
        rng = np.random.default_rng(seed)
        V = int(rng.integers(2, 3000))
        bc, bu = G._row(("random", "peaked", "masked")[seed % 3], V, rng, bf16), G._row("random", V, rng, bf16)
        beta = (0.1, 0.5, 0.01, 1.0)[seed % 4]
        x = G.to_f64(bc, bf16)
        p = np.exp(x - G.lse(x))
        with np.errstate(divide="ignore"):
            margin = np.abs(np.log(p) - np.log(p.max()) - np.log(beta))
        if beta < 1 and (margin <= 1e-6).any():
            continue                                  # an element within 1e-6 of the boundary: the restatement does not decide it
        keep = (p >= beta * p.max()) if beta < 1 else (x == x.max())
        res = G.guide_pair(bc, bu, 1.5, np.float32(np.log(beta)), bf16)
        assert np.array_equal(~np.isnan(res.g), keep & np.isfinite(x)), (seed, beta)
        assert keep[np.argmax(x)]                      # the row maximum always stays
        checked += 1
    assert checked >= 30


def test_non_finite_operands_and_the_identities():
    inf, nan = np.inf, np.nan
    for bf16 in (False, True):
        ninf = 0x8000 | G.inf_bits(bf16)
        b = lambda *v: G.from_f64(np.float64(v), bf16)       # noqa: E731
        xc, xu = b(1.0, -inf, 0.5, 2.0), b(0.0, 1.0, -inf, 1.0)
        r = G.guide_pair(xc, xu, 1.5, -inf, bf16)
        ls = G.log_softmax16(xc, bf16)
        assert r.out[1] == ninf and r.out[2] == ls[2] and np.isfinite(r.g[[0, 2, 3]]).all()
        for bad in (b(1.0, nan, 0.5, 2.0), b(-inf, -inf, -inf, -inf), b(1.0, inf, 0.5, 2.0)):
            assert (G.guide_pair(bad, xu, 1.5, -inf, bf16).out == ninf).all()           # a non-finite lse on either side
            assert (G.guide_pair(b(1.0, 0.0, 0.5, 2.0), bad, 1.5, -inf, bf16).out == ninf).all()
        # saturation: finite operands never give an infinity
        big = -3.0e38 if bf16 else -60000.0
        r = G.guide_pair(b(big, 0.0, 0.0, 0.0), b(0.0, 0.0, 0.0, 0.0), 3.0, -inf, bf16)
        assert r.out[0] == ninf - 1 and np.isfinite(r.g[0])
        # the plausibility boundary, built exactly
        lo = G.to_f64(G._step(b(2.0), np.array([False])), bf16)[0]
        r = G.guide_pair(b(4.0, 2.0, lo, 3.0), b(0.0, 0.0, 0.0, 0.0), 1.5, G.BOUNDARY_LOG_BETA, bf16)
        assert r.out[1] != ninf and r.out[2] == ninf and r.out[0] != ninf
        # gamma == 1 / gamma == 0 outside the band: the once-rounded log_softmax of the conditional / negative row
        rng = np.random.default_rng(3)
        bc, bu = G._row("random", 4000, rng, bf16), G._row("peaked", 4000, rng, bf16)
        one, zero = G.guide_pair(bc, bu, 1.0, -inf, bf16), G.guide_pair(bc, bu, 0.0, -inf, bf16)
        assert np.array_equal(one.out[~one.band], G.log_softmax16(bc, bf16)[~one.band]) and one.band.sum() <= 1
        assert np.array_equal(zero.out, G.log_softmax16(bu, bf16))


@pytest.mark.parametrize("bf16", [False, True], ids=["f16", "bf16"])
@pytest.mark.parametrize("V", G.VOCABS)
def test_excuse_band_census(V, bf16):
    """Every scene and launch of the GPU door test: the elements whose float64 value lies within the excuse band of a rounding
    midpoint are at most 1 in 10^4 of the elements computed — the condition under which the GPU test may excuse them."""
    n_band = n_all = 0
    for name in "AB":
        x = G.scene(name, V, bf16)
        cache = {}
        for sc, lb in G.launches(name):
            y, band, alt = G.guide_rows(x, V, G.COND, G.NEG, sc, lb, bf16, lse_cache=cache)
            n_band += int(band.sum())
            n_all += 5 * V
            assert np.array_equal(y[:, V:], x[:, V:]) and np.array_equal(y[list(G.NEG) + [10, 11]], x[list(G.NEG) + [10, 11]])
            assert (alt[band] != y[band]).all() and np.array_equal(alt[~band], y[~band])
    print(f"census V={V} bf16={bf16}: {n_band} of {n_all} elements in the band")
    assert n_band <= G.CAP * n_all, (n_band, n_all)


def test_scenes_hold_what_the_door_test_needs():
    for bf16 in (False, True):
        ninf = 0x8000 | G.inf_bits(bf16)
        x = G.scene("B", 1000, bf16)
        sat = False
        for sc, lb in G.launches("B"):
            y, _, _ = G.guide_rows(x, 1000, G.COND, G.NEG, sc, lb, bf16)
            assert (y[G.COND[0], :1000] == ninf).all() and (y[G.COND[1], :1000] == ninf).all()      # the NaN row, the all -inf negative
            sat = sat or y[G.COND[2], 0] == ninf - 1
            assert lb[4] == np.float32(-2.0) and y[G.COND[4], 1] != ninf and y[G.COND[4], 2] == ninf and y[G.COND[4], 0] != ninf
        assert sat
        assert {float(g) for sc, _ in G.launches("A") for g in sc} == set(G.GAMMAS) and len(G.launches("A")) == 15


def test_combination_checker():
    assert check_guidance(None) is None and check_guidance(1) is None and check_guidance(1.0, 0.3, negative_given=True) is None
    g, lb = check_guidance(1.5)
    assert g == 1.5 and lb == -np.inf
    assert check_guidance(2, 0.1)[1] == float(np.float32(np.log(0.1))) and check_guidance(0, 1)[1] == 0.0
    for bad in (-0.5, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="guidance_scale"):
            check_guidance(bad)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="plausibility_beta"):
            check_guidance(1.5, bad)
    with pytest.raises(ValueError, match="negative"):
        check_guidance(None, negative_given=True)
    with pytest.raises(ValueError, match="plausibility_beta"):
        check_guidance(None, 0.5)
    with pytest.raises(NotImplementedError, match="num_beams"):
        check_guidance(1.5, num_beams=2)
    with pytest.raises(NotImplementedError, match="speculative"):
        check_guidance(1.5, speculative=3)
    with pytest.raises(NotImplementedError, match="penalty_alpha"):
        check_guidance(1.5, penalty_alpha=0.6)
    assert check_guidance(1.5, penalty_alpha=0) is not None and check_guidance(1, num_beams=4) is None


def test_public_keywords_reach_the_checker_before_any_engine_work():
    """free_form_batch / generate validate the combination first: an object without an engine is enough to see the refusals."""
    import inspect
    from types import SimpleNamespace
    from vstar_amd.api import LlavaSearchModel
    from vstar_amd.config import VQAConfig
    from vstar_amd.vqa import VQA_LLM
    llm = VQA_LLM.__new__(VQA_LLM)
    llm.cfg, llm.engine = VQAConfig.tiny(), None
    img = object()
    for kw, exc in ((dict(guidance_scale=-1), ValueError), (dict(guidance_scale=1.5, plausibility_beta=2), ValueError),
                    (dict(negative_question="what?"), ValueError), (dict(negative_image=img), ValueError),
                    (dict(guidance_scale=1.5, num_beams=2), NotImplementedError), (dict(guidance_scale=1.5, speculative=2), NotImplementedError),
                    (dict(guidance_scale=1.5, penalty_alpha=0.5, top_k=4), NotImplementedError)):
        with pytest.raises(exc):
            llm.free_form_inference(img, "q", **kw)
    with pytest.raises(ValueError, match="KV slots"):
        llm.free_form_batch([dict(image=img, question="q")] * (llm.cfg.max_slots // 2 + 1), guidance_scale=1.5)
    model = LlavaSearchModel.__new__(LlavaSearchModel)
    model._llm, model.engine, model.cfg = llm, None, llm.cfg
    ids = torch.tensor([[1, 5, 6]])
    for kw, exc in ((dict(guidance_scale=float("nan")), ValueError), (dict(negative_prompt_ids=ids), ValueError),
                    (dict(guidance_scale=2, num_beams=2), NotImplementedError), (dict(guidance_scale=2, prompt_lookup_num_tokens=2), NotImplementedError),
                    (dict(guidance_scale=2, penalty_alpha=0.5, top_k=4), NotImplementedError)):
        with pytest.raises(exc):
            model.generate(ids, **kw)
    for fn in (VQA_LLM.free_form_inference, VQA_LLM.free_form_batch):
        assert {"guidance_scale", "negative_question", "negative_image", "plausibility_beta"} <= set(inspect.signature(fn).parameters)
    assert {"guidance_scale", "negative_prompt_ids"} <= set(inspect.signature(LlavaSearchModel.generate).parameters)


def test_the_three_new_names_are_declared_bound_and_exported(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vstar_vqa.h")).read(), flags=re.S)
    for name in ("vstar_vqa_forward_guided", "vstar_vqa_forward_sample_guided", "vstar_vqa_guide_rows"):
        assert re.search(r"\b" + name + r"\s*\(", src) and name in _lib.EXPORTS_VQA and hasattr(lib, name), name
    assert "_op_" not in "vstar_vqa_guide_rows"
    import ctypes
    assert ctypes.sizeof(_lib.VqaGuidance) == 32 and _lib.VqaGuidance.neg.offset == 8
