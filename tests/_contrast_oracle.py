"""CPU oracle of contrastive search (csrc/contrast.hip), restating the contract of include/vstar_vqa.h in float64
numpy, independently of the kernels:
    penalty       pen_c = max_{j < L} cos(h_c, Hs[j]) with exact float64 dot products and norms; a zero-norm row on either side gives
                  cosine 0 (the stated deviation from HF, which yields NaN)
    score_select  score_c = (1 - alpha) * p_c - alpha * pen_c in float64, evaluated as written with the float32 alpha widened first;
                  the winner is the largest score, the lowest c on a tie
    topk_probs    the k largest elements of a logits row under (value descending, index ascending) — a stable sort, -0 == +0, a NaN
                  sorts as -inf — with p = float32(exp(x - lse)), lse = max + log(sum exp(x - max)) in float64
    contrastive_search  HF 4.31's loop over any model_fn(tokens) -> (hidden rows of the new tokens, logits row of the last one)
and, for the two values the kernels promise BIT FOR BIT, the fixed fp32 order of csrc/contrast.hpp:
    row_sum32     the ROW ORDER: lane l of 64 owns the pieces (of 8 elements) l, l + 64, ...; it adds its terms in float32, piece by
                  piece, element by element; the 64 lane sums meet in the xor butterfly 32, 16, 8, 4, 2, 1
    rnorm32       float32(1) / sqrt(row_sum32(h * h)), both correctly rounded; 0 for an all-zero row
The tests allow the derived fp32 bound on the penalties and the fp32 neighbour on the probabilities; the picks are exact."""
import numpy as np


def _f64(a):
    return np.asarray(a, np.float64)


def penalty(cand, hist):
    """cand [m, H], hist [L, H] (L >= 1) -> pen float64 [m].  One matrix-vector product per candidate: equal candidates get equal
    penalties, bit for bit, wherever they stand in the group."""
    c, h = _f64(cand), _f64(hist)
    nh = np.sqrt((h * h).sum(-1))
    pen = np.empty(len(c), np.float64)
    for i, ci in enumerate(c):
        ni = np.sqrt((ci * ci).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            cos = (h @ ci) / (ni * nh)
        cos[(nh == 0) | (ni == 0)] = 0.0
        pen[i] = cos.max()
    return pen


def score_select(prob, pen, alpha):
    """prob [m], pen [m], alpha -> (the winner's index, score float64 [m]); each operation rounded on its own, as numpy does."""
    a = np.float64(np.float32(alpha))
    score = (np.float64(1.0) - a) * _f64(prob) - a * _f64(pen)
    best = 0
    for c in range(1, len(score)):
        if score[c] > score[best]:
            best = c
    return best, score


def topk_probs(row, k):
    """row [V] -> (tokens int32 [k], probabilities float32 [k])."""
    x = _f64(row)
    key = np.where(np.isnan(x), -np.inf, x) + 0.0                 # (+ 0.0: -0 -> +0)
    order = np.argsort(-key, kind="stable")[:k]
    mx = np.max(key)
    lse = mx + np.log(np.exp(x - mx).sum())
    return order.astype(np.int32), np.exp(x[order] - lse).astype(np.float32)


def row_sum32(terms):
    """terms float32 [..., H] (H % 8 == 0) -> their float32 sums [...] in the ROW ORDER of csrc/contrast.hpp."""
    t = np.asarray(terms, np.float32)
    lead = t.shape[:-1]
    pieces = t.reshape(lead + (-1, 8))
    acc = np.zeros(lead + (64,), np.float32)
    for p0 in range(0, pieces.shape[-2], 64):
        blk = pieces[..., p0:p0 + 64, :]
        n = blk.shape[-2]
        for e in range(8):
            acc[..., :n] = acc[..., :n] + blk[..., e]             # float32 adds, one per lane
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lanes ^ o]
    return acc[..., 0]


def rnorm32(rows):
    """The reciprocal norms of stored 16-bit rows [..., H] as the kernels compute them, bit for bit (the squares are exact in
    float32): float32 [...]."""
    h = np.asarray(rows, np.float32)
    sq = np.asarray(row_sum32(h * h), np.float32)
    with np.errstate(divide="ignore"):
        rn = np.float32(1.0) / np.sqrt(sq)
    return np.where(sq > 0, rn, np.float32(0.0)).astype(np.float32)[()]


def contrastive_search(model_fn, prompt, alpha, k, max_new, eos=None):
    """HF 4.31 contrastive_search + _ranking_fast for one sequence.  model_fn(tokens) -> (hidden float [len(tokens), H], logits [V])
    of the whole sequence `tokens`: the final-norm hidden row of every position and the logits row of the last one.  Returns the
    generated tokens (at most max_new; it stops behind eos)."""
    seq = list(prompt)
    hidden, logits = model_fn(seq)
    hist = [np.asarray(r, np.float64) for r in hidden]
    out = []
    for _ in range(max_new):
        tok, prob = topk_probs(logits, k)
        cands = [model_fn(seq + [int(t)]) for t in tok]
        pen = penalty(np.stack([_f64(h[-1]) for h, _ in cands]), np.stack(hist))
        s, _ = score_select(prob, pen, alpha)
        seq.append(int(tok[s]))
        out.append(int(tok[s]))
        hist.append(np.asarray(cands[s][0][-1], np.float64))
        logits = cands[s][1]
        if eos is not None and out[-1] == eos:
            break
    return out
