"""The scoring oracle (tests/_score_oracle.py) on the CPU: hand-worked rows, and its loss pinned against the
expression `VQA_LLM.option_losses` uses today, torch.nn.functional.cross_entropy(logits.float(), ids).to(float16).  Also the
public surface of the feature: the C-ABI symbols and the Python methods exist."""
import math

import numpy as np
import torch

from tests import _score_oracle as S


def test_hand_worked_rows():
    inf = float("inf")
    # one-hot: all the mass on the target
    x = torch.full((1, 7), -inf)
    x[0, 3] = 0.0
    nll, rank, lse, _ = S.score(x, [3])
    assert float(nll[0]) == 0.0 and int(rank[0]) == 0 and float(lse[0]) == 0.0
    # flat: nll = log V, nothing is greater than the target
    for V in (1, 2, 320, 32001):
        nll, rank, _, _ = S.score(torch.zeros(1, V), [V - 1])
        assert float(nll[0]) == float(np.float32(math.log(V))) and int(rank[0]) == 0
    # a -inf target: +inf, every finite logit ranks above it
    x = torch.tensor([[1.0, -inf, 2.0, -inf]])
    nll, rank, _, _ = S.score(x, [1])
    assert float(nll[0]) == inf and int(rank[0]) == 2
    # NaN logits: NaN
    nll, _, _, _ = S.score(torch.tensor([[1.0, float("nan"), 2.0]]), [0])
    assert math.isnan(float(nll[0]))
    # one row wanted twice with different targets: same lse, nll differ by the logit difference
    row = torch.tensor([0.5, -1.25, 3.0, 0.0])
    nll, rank, lse, nll64 = S.score(torch.stack([row, row]), [2, 1])
    assert float(lse[0]) == float(lse[1]) and abs(float(nll64[1] - nll64[0]) - 4.25) < 1e-12
    assert rank.tolist() == [0, 3]
    # ties do not count: rank = number of STRICTLY greater logits
    x = torch.tensor([[1.0, 2.0, 2.0, 3.0]]).repeat(4, 1)
    assert S.score(x, [0, 1, 2, 3])[1].tolist() == [3, 1, 1, 0]
    # two-element row by hand: lse = log(e^0 + e^-1)
    nll, _, _, _ = S.score(torch.tensor([[0.0, -1.0]]), [1])
    assert float(nll[0]) == float(np.float32(math.log(1 + math.exp(-1)) + 1))


def test_loss_reduction_and_helpers():
    v = np.asarray([0.1, 0.2, 0.7], np.float32)
    want = np.float16(np.float32((float(v[0]) + float(v[1]) + float(v[2])) / 3))
    assert S.loss(v).dtype == torch.float16 and float(S.loss(v)) == float(want)
    from vstar_amd.vqa import VQA_LLM
    assert VQA_LLM.nll_loss(v).dtype == torch.float16 and float(VQA_LLM.nll_loss(v)) == float(want)
    one = np.float32(1.0)
    assert S.ulp_distance([one, np.nan, np.inf, one], [np.nextafter(one, np.float32(2)), np.nan, np.inf, np.inf]).tolist()[:3] == [1, 0, 0]
    assert S.ulp_distance([one], [np.inf])[0] > 1
    assert S.ulp_distance([np.float32(-0.0)], [np.float32(0.0)])[0] == 0
    # fp16 neighbours 1 and 1 + 2^-10: the midpoint is 1 + 2^-11
    assert S.near_fp16_midpoint(1 + 2.0 ** -11 + 1e-7, 5e-7) and not S.near_fp16_midpoint(1 + 2.0 ** -11 + 1e-5, 5e-7)
    assert S.near_fp16_midpoint(1 - 2.0 ** -12 - 1e-7, 5e-7)


def test_loss_pinned_against_cross_entropy():
    """fp16(fp32(mean_double(nll))) == cross_entropy(fp32 log-softmax).to(fp16) unless the float64 mean lies within
    4 * 2^-23 * max(1, max|lse|) of an fp16 rounding midpoint; at most 2 % of the losses may use that excuse."""
    from vstar_amd.vqa import VQA_LLM
    g = torch.Generator().manual_seed(20)
    n_all = n_mid = 0
    for V, reps in ((320, 10), (32001, 3)):
        for scale in (1.0, 4.0, 12.0):
            for n in range(1, 13):
                for _ in range(reps):
                    lg = (torch.randn(n, V, generator=g) * scale).half()
                    ids = torch.randint(0, V, (n,), generator=g)
                    ref = torch.nn.functional.cross_entropy(lg.float(), ids).to(torch.float16)
                    nll, _, lse, nll64 = S.score(lg, ids)
                    assert float(VQA_LLM.nll_loss(nll.numpy())) == float(S.loss(nll.numpy()))      # the production reduction
                    verdict = S.losses_agree(S.loss(nll.numpy()), ref, nll64, lse)
                    assert verdict != "differ", (V, scale, n, float(S.loss(nll.numpy())), float(ref))
                    n_all += 1
                    n_mid += verdict == "midpoint"
    print(f"oracle vs cross_entropy: {n_all} losses, {n_mid} excused by the midpoint band")
    assert n_mid <= 0.02 * n_all


def test_public_surface():
    """The feature's entry points exist (binding list, header, Python methods) — none of them does on the parent commit."""
    import os
    from vstar_amd import _lib
    from vstar_amd.vqa import VQA_LLM
    from vstar_amd.vqa_engine import VqaEngine
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vstar_vqa.h")).read()
    for sym in ("vstar_vqa_forward_score", "vstar_vqa_op_score"):
        assert sym in _lib.EXPORTS_VQA and sym + "(" in header
    assert callable(VqaEngine.forward_score)
    for name in ("score_continuations", "option_losses_batch", "multiple_choices_batch"):
        assert callable(getattr(VQA_LLM, name))
    assert float(VQA_LLM.nll_loss(np.asarray([0.25, 0.75], np.float32))) == 0.5
