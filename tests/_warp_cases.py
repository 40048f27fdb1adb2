"""The rows, parameters and oracle results of the warper op test (tests/test_warp_gpu.py), shared with the CPU test that checks
its excuse budget (tests/test_warp_oracle.py): the very seeds, shapes and parameters, built once per (dtype, vocabulary)."""
from __future__ import annotations

import functools

import torch

from tests import _sampling_oracle as S
from tests import _warp_oracle as W

VOCABS = (1, 2, 320, 32001, 32769, 131075)      # LDS-cached rows (<= 32768, 32001 = the real vocabulary) and streamed ones
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
KINDS = ("random", "peaked", "flat", "masked", "levels")      # levels: six distinct scores, so every comparison meets large ties
SPECIAL = ("nan", "plus_inf", "all_minus_inf", "all_nan")
STEP = 7

OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
ALONE = (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=3e-4))
ALL4 = dict(min_p=0.02, typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=6e-4)
# typical_p = 0.999999 asks whether the mass of everything but the farthest tokens is below (1 - 1e-6) Z: the oracle can answer that
# to the margin of 1e-5 only where the farthest tokens carry more than 1.1e-5 of the mass, which no row of 131075 distinct scores
# does.  That set therefore runs on the rows whose scores tie in a few levels (flat, levels), at every size; all others on every kind.
NEARLY_ALL = dict(typical_p=0.999999)
EXTREME = (dict(min_p=1.0), dict(typical_p=1e-6), NEARLY_ALL, dict(epsilon_cutoff=0.999999))
# (top_k, top_p, warpers): each warper alone, all four, each (and all four) after top-k 50 / top-p 0.9, the extreme values
PARAM_SETS = ([(0, 1.0, w) for w in ALONE] + [(0, 1.0, ALL4)] + [(50, 0.9, w) for w in ALONE] + [(50, 0.9, ALL4)]
              + [(0, 1.0, w) for w in EXTREME])


def make_row(kind: str, V: int, g: torch.Generator, dtype) -> torch.Tensor:
    x = torch.randn(V, generator=g) * 3
    if kind == "peaked":
        x = torch.randn(V, generator=g)
        x[int(torch.randint(0, V, (1,), generator=g))] += 15
    elif kind == "flat":
        x = torch.full((V,), 1.5)
    elif kind == "masked":                      # runs of -inf (and of the most negative finite number)
        m = torch.rand(V, generator=g) < 0.5
        x = torch.where(m, torch.where(torch.rand(V, generator=g) < 0.5, -float("inf"), -65504.0), x)
        if V > 1:
            x[0] = 2.0
    elif kind == "levels":
        x = torch.randint(0, 6, (V,), generator=g).float() * 1.5
    elif kind == "nan":
        x[torch.rand(V, generator=g) < 0.3] = float("nan")
    elif kind == "plus_inf":
        x[int(torch.randint(0, V, (1,), generator=g))] = float("inf")
    elif kind == "all_minus_inf":
        x = torch.full((V,), -float("inf"))
    elif kind == "all_nan":
        x = torch.full((V,), float("nan"))
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def cases(dtype_name: str, V: int):
    """[(row tensor [V], temperature, top_k, top_p, warpers dict (all four fields), seed)] of one (dtype, vocabulary)."""
    dtype = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(1000 * V + (dtype_name == "bf16"))
    out = []
    for rep in range(4 if V <= 320 else 1):      # (small rows are cheap: more of them)
        for pi, (k, p, w) in enumerate(PARAM_SETS):
            for kind in KINDS:
                if w is NEARLY_ALL and kind not in ("flat", "levels"):
                    continue
                out.append((make_row(kind, V, g, dtype), (1.0, 0.7)[(pi + rep) % 2], k, p, {**OFF, **w}, 5000 + len(out)))
    for kind in SPECIAL:
        for k, p, w in ((0, 1.0, ALL4), (50, 0.9, ALL4), (0, 1.0, ALONE[1]), (0, 1.0, ALONE[3])):
            out.append((make_row(kind, V, g, dtype), 1.0, k, p, {**OFF, **w}, 5000 + len(out)))
    return out


@functools.lru_cache(maxsize=None)
def reference(dtype_name: str, V: int):
    """The oracle's result (tests/_warp_oracle.warp_row) for every case of `cases`, computed once."""
    return [W.warp_row(x, t, k, p, S.uniform(seed, STEP, 3 * seed), **w) for x, t, k, p, w, seed in cases(dtype_name, V)]
