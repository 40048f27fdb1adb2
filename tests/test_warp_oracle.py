"""CPU side of the further warpers: the oracle (tests/_warp_oracle.py) against the installed transformers'
warpers, the Python validation, the ABI record and exports, the way the keywords reach the engine, and the excuse budget of the
GPU op test (tests/test_warp_gpu.py), counted on the very cases it runs."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sampling_oracle as S
from tests import _warp_cases as C
from tests import _warp_oracle as W
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.vqa import VQA_LLM, warper_params
from vstar_amd.vqa_engine import VqaEngine

STAGES = (("min_p", 0.05), ("typical_p", 0.9), ("epsilon_cutoff", 3e-4), ("eta_cutoff", 3e-4))


def _hf(name, value):
    from transformers.generation import logits_process as L
    return {"min_p": L.MinPLogitsWarper, "typical_p": L.TypicalLogitsWarper, "epsilon_cutoff": L.EpsilonLogitsWarper,
            "eta_cutoff": L.EtaLogitsWarper}[name](value)


def _hf_keep(x: torch.Tensor, keep0: np.ndarray, stages) -> np.ndarray:
    """The kept set of HF's warpers, chained in the given order, on the float32 row x restricted to keep0."""
    scores = x.clone()[None]
    scores[0, torch.from_numpy(~keep0)] = -float("inf")
    ids = torch.zeros(1, 1, dtype=torch.long)
    for name, value in stages:
        scores = _hf(name, value)(ids, scores)
    return torch.isfinite(scores[0]).numpy()


def _tie_free_row(V, g, scale):
    while True:
        x = torch.randn(V, generator=g) * scale
        if x.unique().numel() == V:
            return x


@pytest.mark.parametrize("chain", [(s,) for s in STAGES] + [STAGES], ids=[s[0] for s in STAGES] + ["all_four"])
def test_oracle_equals_transformers_warpers(chain):
    pytest.importorskip("transformers")
    g = torch.Generator().manual_seed(len(chain) * 7 + len(chain[0][0]))
    checked = excused = 0
    for V in (12, 50, 333, 2000):
        for rep in range(12):
            x = _tie_free_row(V, g, (1.0, 2.0, 3.0)[rep % 3])
            s = x.double().numpy()
            top_k, top_p = ((0, 1.0), (50, 0.9))[rep % 2]
            keep0, p_dist = S.kept(s, top_k, top_p)
            keep, mg = W.warp(s, keep0, **dict(chain))
            if min(W.margin(mg), p_dist * 10) < W.MARGIN:
                excused += 1
                continue
            assert np.array_equal(keep, _hf_keep(x, keep0, chain)), (chain, V, rep)
            assert keep.any() and not (keep & ~keep0).any()
            checked += 1
    print(f"{[c[0] for c in chain]}: {checked} rows equal, {excused} excused")
    assert excused <= 2 and checked >= 40


def test_oracle_stage_rules_on_a_hand_row():
    # p = (0.5, 0.25, 0.125, 0.0625, 0.0625): l = ln p - ln 0.5
    s = np.log(np.array([0.5, 0.25, 0.125, 0.0625, 0.0625]))
    all_ = np.ones(5, bool)
    assert W.warp(s, all_, min_p=0.3)[0].tolist() == [True, True, False, False, False]
    assert W.warp(s, all_, epsilon_cutoff=0.1)[0].tolist() == [True, True, True, False, False]
    # H = 1.875 bits = 1.2997 nats: -ln p = (0.69, 1.39, 2.08, 2.77, 2.77) -> d = (0.61, 0.09, 0.78, 1.47, 1.47)
    k, mg = W.warp(s, all_, typical_p=0.5)
    assert k.tolist() == [True, True, False, False, False]         # 0.25, then 0.5: the mass in front of the third is 0.75
    assert W.warp(s, all_, typical_p=0.2)[0].tolist() == [False, True, False, False, False]      # the band leaves the arg-max out
    assert W.warp(s, all_, typical_p=0.9)[0].tolist() == [True, True, True, True, True]          # both ties at 1.47 stay
    assert mg["typical_d"] > 0.1 and mg["typical_mass"] > 0.2
    # eta = min(0.2, sqrt(0.2) * exp(-1.2997)) = 0.1219
    assert W.warp(s, all_, eta_cutoff=0.2)[0].tolist() == [True, True, True, False, False]
    # a cutoff above every probability keeps the largest score
    assert W.warp(s, all_, epsilon_cutoff=0.9)[0].tolist() == [True, False, False, False, False]
    # epsilon after a band that dropped the arg-max keeps the band's own maximum
    assert W.warp(s, all_, typical_p=0.2, epsilon_cutoff=0.999)[0].tolist() == [False, True, False, False, False]


def test_warper_params_validation():
    assert warper_params() is None and warper_params(0, 1.0, 0.0, 0) is None and warper_params(typical_p=3.0) is None
    w = warper_params(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=6e-4)
    assert (w.min_p, w.typical_p, w.epsilon_cutoff, w.eta_cutoff) == tuple(float(np.float32(v)) for v in (0.05, 0.9, 3e-4, 6e-4))
    w = warper_params(min_p=1.0)
    assert (w.min_p, w.typical_p, w.epsilon_cutoff, w.eta_cutoff) == (1.0, 1.0, 0.0, 0.0)
    for bad in (dict(min_p=-0.1), dict(min_p=1.01), dict(min_p=float("nan")), dict(typical_p=0.0), dict(typical_p=-1),
                dict(typical_p=float("nan")), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-1e-3), dict(eta_cutoff=1.0),
                dict(eta_cutoff=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(bad))):
            warper_params(**bad)


def test_warpers_struct_layout_and_exports(lib):
    W_ = _lib.VqaWarpers
    assert ctypes.sizeof(W_) == 16 and ctypes.sizeof(_lib.VqaSampling) == 32
    assert [(n, getattr(W_, n).offset) for n, _ in W_._fields_] == [("min_p", 0), ("typical_p", 4), ("epsilon_cutoff", 8), ("eta_cutoff", 12)]
    for name in ("vstar_vqa_forward_sample_warp", "vstar_vqa_forward_verify_warp", "vstar_vqa_op_sample_warp", "vstar_vqa_op_verify_warp"):
        assert name in _lib.EXPORTS_VQA and hasattr(lib, name)
    assert len(lib.vstar_vqa_forward_sample_warp.argtypes) == len(lib.vstar_vqa_forward_sample_logprobs.argtypes) + 1
    assert len(lib.vstar_vqa_op_sample_warp.argtypes) == len(lib.vstar_vqa_op_sample.argtypes) + 2


class _StubEngine(VqaEngine):
    """Records what the decode loops hand to forward_sample / forward_verify; every draw is EOS, so a decode is one call."""

    def __init__(self, cfg):
        self.cfg, self.calls, self.handle = cfg, [], None

    def encode_images(self, pixels, first_slot=0):
        pass

    def forward_sample(self, seqs, want, params, edits=None, logprobs=None, warpers=None):
        self.calls.append(("sample", len(want), warpers))
        return np.full(len(want), 2, np.int32)

    def forward_verify(self, step, wanted, groups, draft, params=None, edits=None, logprobs=None, warpers=None):
        self.calls.append(("verify", len(wanted), warpers))
        return np.zeros(len(groups) - 1, np.int32), np.full(len(wanted), 2, np.int32)

    def forward(self, seqs, want, logits=True, edits=None, logprobs=None):
        self.calls.append(("greedy", len(want), None))
        return None, np.full(len(want), 2, np.int32)


def _fields(w):
    return None if w is None else tuple(round(float(getattr(w, n)), 7) for n, _ in _lib.VqaWarpers._fields_)


def test_keywords_reach_the_engine():
    from PIL import Image
    from vstar_amd import vqa
    from vstar_amd.api import LlavaSearchModel
    cfg = VQAConfig.tiny()
    eng = _StubEngine(cfg)
    llm = VQA_LLM(cfg=cfg, engine=eng)
    assert llm.eos_token_id == 2
    image = Image.fromarray(np.zeros((64, 64, 3), np.uint8))
    q = "What is it?"
    # free_form_inference / free_form_batch
    llm.free_form_inference(image, q, temperature=0.8, typical_p=0.9, seed=1)
    assert eng.calls[-1][0] == "sample" and _fields(eng.calls[-1][2]) == (0.0, 0.9, 0.0, 0.0)
    llm.free_form_batch([dict(image=image, question=q)] * 2, temperature=0.8, min_p=0.05, epsilon_cutoff=3e-4, eta_cutoff=6e-4, seed=1)
    assert eng.calls[-1][:2] == ("sample", 2) and _fields(eng.calls[-1][2]) == (0.05, 1.0, 3e-4, 6e-4)
    # all off: the plain call (no record at all); greedy ignores them
    llm.free_form_inference(image, q, temperature=0.8, typical_p=1.0, min_p=0.0, seed=1)
    assert eng.calls[-1] == ("sample", 1, None)
    llm.free_form_inference(image, q, typical_p=0.5)
    assert eng.calls[-1] == ("greedy", 1, None)
    # LlavaSearchModel.generate under HF's names: swallowed by **unused before
    model = LlavaSearchModel(llm)
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), llm.tokenizer)).unsqueeze(0)
    kw = dict(images=torch.zeros(1, 3, cfg.clip_image_size, cfg.clip_image_size), max_new_tokens=4)
    model.generate(input_ids, do_sample=True, temperature=0.8, typical_p=0.9, seed=1, **kw)
    assert eng.calls[-1][0] == "sample" and _fields(eng.calls[-1][2]) == (0.0, 0.9, 0.0, 0.0)
    model.generate(input_ids, do_sample=True, temperature=0.8, min_p=0.05, seed=1, **kw)
    assert _fields(eng.calls[-1][2]) == (0.05, 1.0, 0.0, 0.0)
    model.generate(input_ids, do_sample=False, typical_p=0.9, **kw)
    assert eng.calls[-1] == ("greedy", 1, None)
    with pytest.raises(ValueError, match="typical_p"):
        model.generate(input_ids, do_sample=True, temperature=0.8, typical_p=0.0, **kw)
    # the speculative path: the prefill's draw and every verify call carry the record
    eng.calls.clear()
    eng.forward_sample = lambda seqs, want, params, edits=None, logprobs=None, warpers=None: (
        eng.calls.append(("sample", len(want), warpers)), np.full(len(want), 5, np.int32))[1]
    llm.free_form_inference(image, q, temperature=0.8, eta_cutoff=1e-3, speculative=2, max_new_tokens=3, seed=1)
    kinds = [c[0] for c in eng.calls]
    assert kinds[0] == "sample" and "verify" in kinds and all(_fields(c[2]) == (0.0, 1.0, 0.0, 1e-3) for c in eng.calls)


def test_gpu_op_test_excuse_budget():
    """The rows of tests/test_warp_gpu.py::test_op_against_oracle — the very seeds, shapes and parameters — whose smallest oracle
    margin is below the limit are at most 0.1 % of all rows (the cap tests/test_sampling_gpu.py applies to its excuses)."""
    rows = low = 0
    for dn in C.DTYPES:
        for V in C.VOCABS:
            ref = C.reference(dn, V)
            rows += len(ref)
            low += sum(r["margin"] < W.MARGIN for r in ref)
    print(f"{rows} rows, {low} with a margin below {W.MARGIN}")
    assert rows >= 2000 and low <= 0.001 * rows
