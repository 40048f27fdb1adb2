"""CPU oracle of the log-probability stage (csrc/logprob.hip), restating its contract in float64 torch:
    lse_r     = max + log(sum exp(x_i - max))                    (double; exactly tests/_score_oracle.score's)
    lp_r      = float32(x[t_r] - lse_r)                          (one rounding; -inf token -> -inf, NaN -> NaN)
    rank_r    = #{i : x_i > x[t_r]}
    top_r     = the n = min(n_top, V) largest elements under (value descending, index ascending) — a stable sort, -0 == +0, a NaN
                sorts as -inf — with top_lp = float32(x[i] - lse_r); entries [n, n_top) are -1 / NaN
    t_r < 0   : the row is not read: lp NaN, rank -1, top_tok -1, top_lp NaN
The tests allow the fp32 neighbour (1 ulp) on the float outputs for the device's exp / log in double, as tests/test_score_gpu.py
does (tests/_score_oracle.ulp_distance); the integer outputs are exact."""
import numpy as np
import torch

from tests import _score_oracle as S


def logprobs(logits: torch.Tensor, tokens, n_top: int):
    """logits [rows, V] (any float dtype), tokens [rows] -> (lp float32 [rows], rank int32 [rows], top_tok int32 [rows, n_top],
    top_lp float32 [rows, n_top]) as numpy arrays."""
    x = logits.double()
    rows, V = x.shape
    t = torch.as_tensor(tokens, dtype=torch.long)
    live = t >= 0
    tc = t.clamp(min=0)
    _, rank, lse, nll64 = S.score(x, tc)
    lp = (-nll64).float().numpy().copy()                 # x[t] - lse: the negation is exact, the rounding symmetric
    rank = rank.numpy().copy()
    n = min(n_top, V)
    top_tok = np.full((rows, n_top), -1, np.int32)
    top_lp = np.full((rows, n_top), np.nan, np.float32)
    if n:
        key = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x)
        order = torch.sort(key, dim=-1, descending=True, stable=True).indices[:, :n]
        top_tok[:, :n] = order.numpy()
        top_lp[:, :n] = (x.gather(-1, order) - lse[:, None]).float().numpy()
    dead = ~live.numpy()
    lp[dead] = np.nan
    rank[dead] = -1
    top_tok[dead] = -1
    top_lp[dead] = np.nan
    return lp, rank, top_tok, top_lp
