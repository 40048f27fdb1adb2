"""CPU oracle of the scoring tail (csrc/score.hip), restating its contract in float64 torch:
    lse_j  = max + log(sum exp(x_i - max))                      (double)
    nll_j  = float32(lse_j - x[t_j])                            (one rounding; -inf target -> +inf, NaN -> NaN)
    rank_j = #{i : x_i > x[t_j]}
    loss   = fp16(fp32(sum_double(nll) / n))                    (the per-token values in token order)
and the two allowances the tests use: the fp32 neighbour (1 ulp) for device exp/log, and the fp16 rounding-midpoint band
against torch's fp32 cross_entropy."""
import numpy as np
import torch


def score(logits: torch.Tensor, targets):
    """logits [rows, V] (any float dtype), targets [rows] -> (nll float32 [rows], rank int32 [rows], lse float64, nll float64)."""
    x = logits.double()
    t = torch.as_tensor(targets, dtype=torch.long)
    m = x.max(-1, keepdim=True).values
    lse = (m + torch.log(torch.exp(x - m).sum(-1, keepdim=True)))[:, 0]
    xt = x.gather(-1, t[:, None])[:, 0]
    nll64 = lse - xt
    rank = (x > xt[:, None]).sum(-1).to(torch.int32)
    return nll64.float(), rank, lse, nll64


def loss(nll) -> torch.Tensor:
    """fp16(fp32(sum_double(nll) / n)), the values added in token order."""
    acc = 0.0
    vals = [float(v) for v in np.asarray(nll, np.float32)]
    for v in vals:
        acc += v
    return torch.tensor(np.float16(np.float32(acc / len(vals))))


def ulp_distance(a, b) -> np.ndarray:
    """Distance in fp32 steps between two float32 arrays; 0 where both are NaN or the same infinity, a large number where
    only one of them is not finite."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    fin = np.isfinite(a) & np.isfinite(b)

    def key(v):      # monotone integer image of the floats
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    return np.where(same, 0, np.where(fin, d, 1 << 40))


def band(lse) -> float:
    """Half-width of the midpoint band: a few fp32 ulps of the largest intermediate of torch's fp32 log-softmax."""
    return 4.0 * 2.0 ** -23 * max(1.0, float(torch.as_tensor(lse).abs().max()))


def near_fp16_midpoint(mean64: float, width: float) -> bool:
    """Is the float64 value within `width` of a midpoint between two neighbouring fp16 values?"""
    h = np.float16(mean64)
    if not np.isfinite(h):
        return False
    for other in (np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(-np.inf))):
        if np.isfinite(other) and abs(mean64 - (float(h) + float(other)) / 2) <= width:
            return True
    return False


def losses_agree(loss_a, loss_b, nll64, lse) -> str:
    """'equal', 'midpoint' (different fp16 values, excused by the band) or 'differ'."""
    a, b = np.float16(float(loss_a)), np.float16(float(loss_b))
    if a == b or (np.isnan(a) and np.isnan(b)):
        return "equal"
    mean64 = float(torch.as_tensor(nll64, dtype=torch.float64).sum() / len(nll64))
    return "midpoint" if near_fp16_midpoint(mean64, band(lse)) else "differ"
