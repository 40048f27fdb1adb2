"""CPU oracle of beam search: an independent torch restatement of HF 4.31 `beam_search` + `BeamSearchScorer` (DESIGN.md §8.2,
rules 1-8), written from the 4.31 loop and kept apart from the production scorer (vstar_amd/beam.py).

    logits_fn(histories) -> [k, V] logits of the k running beams (histories: the generated ids of each beam)

Scores: lp = log_softmax(logits) rounded to the logits' dtype (`exact=True`: the log-sum-exp in float64, as the device does;
False: torch's fp32 log_softmax, as 4.31 does), s = beam_score + float(lp) in fp32.  Candidates: top 2k of s over k x V, ties to
the smaller flat index."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch


def round_once(d: torch.Tensor, dtype) -> torch.Tensor:
    """float64 -> dtype with ONE round-to-nearest-even: via float32 rounded to odd (exact for 16-bit targets)."""
    d = d.double()
    f = d.float()
    if dtype == torch.float32:
        return f
    inexact = (f.double() != d) & ~torch.isnan(d)
    b = f.view(torch.int32).clone()
    b = torch.where(inexact & (f.double().abs() > d.abs()), b - 1, b)
    b = torch.where(inexact, b | 1, b)
    return b.view(torch.float32).to(dtype)


def log_probs(logits: torch.Tensor, exact: bool = True) -> torch.Tensor:
    """[rows, V] logits (fp16 / bf16 / fp32) -> lp in the same dtype."""
    if exact:
        x = logits.double()
        return round_once(x - torch.logsumexp(x, dim=-1, keepdim=True), logits.dtype)
    return torch.log_softmax(logits.float(), dim=-1).to(logits.dtype)


def candidates(lp: torch.Tensor, beam_scores: torch.Tensor, n_cand: int):
    """Top n_cand of s = beam_score + lp over the flattened [k, V], sorted by (s desc, flat index asc): (s, token, row)."""
    k, V = lp.shape
    if n_cand > k * V:
        raise ValueError("n_cand > k * V")
    s = (beam_scores.float()[:, None] + lp.float()).reshape(-1)
    order = torch.sort(s, descending=True, stable=True).indices[:n_cand]
    return s[order], order % V, torch.div(order, V, rounding_mode="floor")


def boundary_gap(lp: torch.Tensor, beam_scores: torch.Tensor, n_cand: int) -> float:
    """|s_(n) - s_(n+1)| at the rank-n boundary (inf when there is no (n+1)-th): where a tiny lp difference may swap a candidate."""
    s = torch.sort((beam_scores.float()[:, None] + lp.float()).reshape(-1), descending=True).values
    return float("inf") if s.numel() <= n_cand else float(s[n_cand - 1] - s[n_cand])


def beam_search(logits_fn: Callable[[List[List[int]]], torch.Tensor], num_beams: int, prompt_len: int, eos: int,
                max_new_tokens: int, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                exact: bool = True, trace: Optional[list] = None) -> List[List[int]]:
    """The whole 4.31 loop for ONE sample; returns the generated ids of the num_return_sequences best hypotheses (finalize's
    EOS append / EOS padding included).  trace (optional) receives per step (lp, beam_scores, (s, tok, row))."""
    k = num_beams
    max_length = prompt_len + max_new_tokens
    hist: List[List[int]] = [[] for _ in range(k)]
    scores = torch.full((k,), -1e9, dtype=torch.float32)
    scores[0] = 0.0
    hyps: List[tuple] = []          # (score, ids)
    worst = 1e9
    done = False

    def add(ids, length, sum_lp):
        nonlocal worst
        sc = sum_lp / (length ** length_penalty)
        if len(hyps) < k or sc > worst:
            hyps.append((sc, list(ids)))
            if len(hyps) > k:
                order = sorted((h[0], i) for i, h in enumerate(hyps))
                del hyps[order[0][1]]
                worst = order[1][0]
            else:
                worst = min(sc, worst)

    def is_done(best, cur_len):
        if len(hyps) < k:
            return False
        if early_stopping is True:
            return True
        if early_stopping == "never" and length_penalty > 0.0:
            return worst >= best / max_length ** length_penalty
        return worst >= best / cur_len ** length_penalty

    while True:
        logits = logits_fn(hist)
        lp = log_probs(logits, exact)
        s, tok, row = candidates(lp, scores, 2 * k)
        if trace is not None:
            trace.append((lp, scores.clone(), (s, tok, row)))
        cur_len = prompt_len + len(hist[0])
        nh, ns = [], []
        for rank in range(2 * k):
            t, b, sc = int(tok[rank]), int(row[rank]), s[rank]
            if t == eos:
                if rank < k:
                    add(hist[b], cur_len, float(sc))
            else:
                nh.append(hist[b] + [t])
                ns.append(sc)
            if len(nh) == k:
                break
        assert len(nh) == k
        done = done or is_done(float(s.max()), cur_len)
        hist, scores = nh, torch.stack(ns).float()
        if done or len(hist[0]) >= max_new_tokens:
            break
    if not done:
        for b in range(k):
            add(hist[b], prompt_len + len(hist[b]), float(scores[b]))
    ranked = sorted(hyps, key=lambda h: h[0])
    best = [ranked.pop()[1] for _ in range(num_return_sequences)]
    lens = [prompt_len + len(h) for h in best]
    width = min(max(lens) + 1, max_length)
    out = []
    for h, n in zip(best, lens):
        r = list(h) + ([eos] if n < width else [])
        out.append(r + [eos] * (width - prompt_len - len(r)))
    return out


def scripted(table: Sequence[Sequence[Sequence[float]]], dtype=torch.float32):
    """logits_fn replaying per-step [k, V] logits rows (for hand-worked cases)."""
    it = iter(table)

    def fn(_hist):
        return torch.tensor(next(it), dtype=dtype)
    return fn
