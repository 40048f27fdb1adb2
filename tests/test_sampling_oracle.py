"""Sampled decoding, CPU side: the Philox stream, the oracle's kept sets against the transformers warpers, the C-ABI record and
the exported entry points (the library loads on a GPU-less host)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sampling_oracle as S
from vstar_amd import _lib


def test_philox_known_answers():
    # Random123 known-answer vectors of philox4x32_10
    assert S.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    ones = 0xFFFFFFFF
    assert S.philox4x32_10([ones] * 4, [ones, ones]) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    u = S.uniform(0, 0)
    assert u == (0x6627E8D5 >> 8) * 2.0 ** -24 and 0 <= u < 1 and float(np.float32(u)) == u


def test_sampling_record_layout():
    assert ctypes.sizeof(_lib.VqaSampling) == 32
    offs = {n: getattr(_lib.VqaSampling, n).offset for n, _ in _lib.VqaSampling._fields_}
    assert offs == {"temperature": 0, "top_k": 4, "top_p": 8, "step": 12, "seed": 16, "stream": 24}


def test_library_exports_the_sampling_entry_points(lib):
    for name in ("vstar_vqa_forward_sample", "vstar_vqa_op_sample"):
        assert name in _lib.EXPORTS_VQA
        assert hasattr(lib, name), name


def test_sampling_params_validation():
    from vstar_amd.vqa import sampling_params
    p = sampling_params(0.7, None, None, seed=(1 << 64) + 5, stream=3, step=9)
    assert (p.top_k, p.top_p, p.seed, p.stream, p.step) == (0, 1.0, 5, 3, 9)
    assert abs(p.temperature - 0.7) < 1e-7
    for bad in (dict(temperature=0), dict(temperature=-1), dict(temperature=1, top_k=-1), dict(temperature=1, top_p=float("nan"))):
        with pytest.raises(ValueError):
            sampling_params(**bad)


def _hf_kept(s32: torch.Tensor, top_k, top_p):
    from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper
    x = s32[None].clone()
    if top_k:
        x = TopKLogitsWarper(top_k=min(top_k, x.shape[1]))(None, x)
    if top_p is not None and top_p < 1:
        x = TopPLogitsWarper(top_p=top_p)(None, x)
    return torch.isfinite(x[0]).numpy()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_oracle_kept_sets_equal_the_transformers_warpers(dtype):
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import TemperatureLogitsWarper
    g = torch.Generator().manual_seed(3)
    checked = skipped = 0
    for r in range(300):
        V = int(torch.randint(2, 1500, (1,), generator=g))
        x = (torch.randn(V, generator=g) * float(torch.rand(1, generator=g) * 4 + 0.5)).to(dtype)
        t = [0.3, 0.7, 1.0, 2.0][r % 4]
        top_k = [0, 1, 5, 50, V + 3][r % 5]
        top_p = [None, 0.9, 0.5, 0.0, 0.97][(r // 5) % 5]
        s = S.scaled_scores(x, t)
        keep, dist = S.kept(s, top_k, top_p)
        # step 1 is HF's temperature warper in fp32, rounded to the storage type
        hf_scores = TemperatureLogitsWarper(float(np.float32(t)))(None, x.float()[None])[0].to(dtype)
        assert np.array_equal(hf_scores.double().numpy(), s)
        low = s[keep].min()
        if dist < 1e-5 or (top_p is not None and top_p < 1 and (s == low).sum() > 1 and keep.sum() < V):
            skipped += 1                 # a top-p boundary tie or a numerically ambiguous boundary: the documented deviation
            continue
        hf = _hf_kept(torch.from_numpy(s).float(), top_k, top_p)
        assert (hf == keep).all(), (r, V, t, top_k, top_p, int(hf.sum()), int(keep.sum()))
        checked += 1
    print(f"{checked} rows compared, {skipped} boundary-tie rows skipped")
    assert checked >= 150


def test_oracle_tie_rule():
    x = torch.tensor([1.0, 3.0, 3.0, 3.0, 2.0, 0.0], dtype=torch.float16)
    keep, _ = S.kept(S.scaled_scores(x, 1.0), 2, None)
    assert keep.tolist() == [False, True, True, True, False, False]       # every tie at the k-th value
    keep, _ = S.kept(S.scaled_scores(x, 1.0), 0, 0.0)
    assert keep.tolist() == [False, True, True, True, False, False]       # top_p = 0 keeps the maximal score's ties
    # mass above the tied pair {4, 5} is 0.5 < 0.6: the whole tie is kept, the 0.1 tail is not
    y = torch.log(torch.tensor([0.1, 0.5, 0.05, 0.05, 0.15, 0.15], dtype=torch.float64)).to(torch.float16)
    keep, _ = S.kept(S.scaled_scores(y, 1.0), 0, 0.6)
    assert keep.tolist() == [False, True, False, False, True, True]
