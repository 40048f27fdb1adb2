"""CPU oracle of the verify tail of speculative decoding (csrc/spec.hip) and of the decode loop built on it.

Greedy: a row's choice is the engine's arg-max rule (first index of the largest number; NaN and -inf never win; 0 when nothing
does).  Sampled: the kept set, masses and Philox stream of tests/_sampling_oracle.py; a draft x is accepted iff it is kept and
u_a * Z < m_x (u_a: Philox stream + 1), otherwise the token is the plain inverse-CDF draw over the kept set without x.
`verify_int` is the same rule on integer masses and 24-bit uniforms, exactly as the kernel evaluates it."""
from __future__ import annotations

import numpy as np
import torch

from tests import _sampling_oracle as S


def greedy_choice(row) -> int:
    v = np.asarray(row, np.float64)
    ok = v > -3.0e38                       # NaN compares false; -inf (and bf16 values below -3e38) never win
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (v == v[ok].max()))[0])


def finish(choices, flags):
    """The group rule: (n_accept, tokens) from the per-row choices and accept flags (the last row is never compared)."""
    a = 0
    while a < len(choices) - 1 and flags[a]:
        a += 1
    return a, [int(c) if j <= a else -1 for j, c in enumerate(choices)]


def verify_greedy(logits, draft):
    ch = [greedy_choice(r) for r in logits]
    return finish(ch, [c == int(x) for c, x in zip(ch, draft)])


def sampled_row(x: torch.Tensor, t: float, top_k: int, top_p, seed: int, step: int, stream: int, draft: int):
    """One row: dict(token, accept, dist) — dist = the smallest relative distance of a decision to its boundary (the accept
    threshold, a prefix-mass boundary of the draw, the top-p cut)."""
    s = S.scaled_scores(x, t)
    keep, p_dist = S.kept(s, top_k, top_p)
    w = S.masses(s) * keep
    Z = w.sum()
    u = S.uniform(seed, step, stream)
    if draft < 0:
        tok, u_dist = S.draw(s, keep, u)
        return dict(token=tok, accept=False, dist=min(u_dist, p_dist))
    ua = S.uniform(seed, step, stream + 1)
    a_dist = abs(ua * Z - w[draft]) / Z
    if keep[draft] and ua * Z < w[draft]:
        return dict(token=int(draft), accept=True, dist=min(a_dist, p_dist))
    keep2 = keep.copy()
    keep2[draft] = False
    tok, u_dist = S.draw(s, keep2, u)
    return dict(token=tok, accept=False, dist=min(a_dist, u_dist * (w.sum() - w[draft] * keep[draft]) / Z, p_dist))


def verify_sampled(rows, draft, prm):
    """rows: fp16 / bf16 tensors of one group; prm[j] = (t, top_k, top_p, seed, step, stream).  (n_accept, tokens, min dist over
    the rows that decide the result)."""
    res = [sampled_row(r, *p, int(x)) for r, x, p in zip(rows, draft, prm)]
    a, toks = finish([r["token"] for r in res], [r["accept"] for r in res])
    return a, toks, min(r["dist"] for r in res[:a + 1])


def verify_int(m, x: int, ua24: int, u24: int):
    """The kernel's integer rule on masses m (Python ints, 0 = not kept): (token, accepted)."""
    Z = sum(m)
    if x >= 0 and ((ua24 * Z) >> 24) < m[x]:
        return x, True
    Zp = Z - (m[x] if x >= 0 else 0)
    target, acc = (u24 * Zp) >> 24, 0
    for i, mi in enumerate(m):
        if i == x or mi == 0:
            continue
        acc += mi
        if acc > target:
            return i, False
    raise AssertionError("no token drawn")


def count_below(t: int, Z: int) -> int:
    """#{u24 in [0, 2^24) : floor(u24 * Z / 2^24) < t} for integers 0 <= t <= Z, Z > 0: closed form."""
    return min(1 << 24, -((-t << 24) // Z))


def first_token_distribution(m, x: int):
    """P(token = y) over all 2^24 x 2^24 pairs (u_a, u) under verify_int, as exact fractions of 2^48 (floats)."""
    Z = sum(m)
    n_acc = count_below(m[x], Z) if x >= 0 else 0
    Zp = Z - (m[x] if x >= 0 else 0)
    p = np.zeros(len(m))
    if x >= 0:
        p[x] = n_acc / 2.0 ** 24
    pre = 0
    for i, mi in enumerate(m):
        if i == x or mi == 0:
            continue
        p[i] += (1 - n_acc / 2.0 ** 24) * (count_below(pre + mi, Zp) - count_below(pre, Zp)) / 2.0 ** 24
        pre += mi
    return p


def spec_loop(step_fn, first, ids, pos, max_new, d, draft_fn, eos, vocab, max_ctx, max_rows=256, choose=None):
    """The speculative decode loop of VQA_LLM.speculative_decode over step_fn([(sequence, rows, past_len, the text ids in front of
    the rows)]) -> one logits array [len(rows), vocab] per entry.  choose(i, token index of row 0, logits rows, draft) -> (n_accept, tokens); default greedy.
    Returns (outputs, number of step_fn calls)."""
    n = len(first)
    out = [[int(first[i])] for i in range(n)]
    pos = list(pos)
    choose = choose or (lambda i, t, lg, dr: verify_greedy(lg, dr))
    calls = 0

    def alive(i):
        return out[i][-1] != eos and len(out[i]) < max_new and pos[i] + 1 < max_ctx

    live = [i for i in range(n) if alive(i)]
    while live:
        spare = min(max_rows, 256) - len(live)
        batch, drafts = [], []
        for i in live:
            k = min(d, max_new - len(out[i]) - 1, max_ctx - pos[i] - 2, max(spare, 0))
            guess = []
            if k > 0:
                for t in list(draft_fn(list(ids[i]) + out[i], k))[:k]:
                    if not 0 <= int(t) < vocab:
                        break
                    guess.append(int(t))
            spare -= len(guess)
            batch.append((i, [out[i][-1]] + guess, pos[i], list(ids[i]) + out[i][:-1]))
            drafts.append(guess + [-1])
        logits = step_fn(batch)
        calls += 1
        for (i, rows, _, _), lg, dr in zip(batch, logits, drafts):
            a, toks = choose(i, len(out[i]), lg, dr)[:2]
            new = toks[:a + 1]
            pos[i] += a + 1
            if eos in new:
                new = new[:new.index(eos) + 1]
            out[i] += new
        live = [i for i in live if alive(i)]
    return out, calls


def plain_loop(logits_fn, prompt, max_new, eos, max_ctx=1 << 30):
    """The stepwise greedy loop over a pure logits_fn(ids) -> next-token logits (VQA_LLM._decode's stop rule)."""
    ids, out = list(prompt), []
    while True:
        out.append(greedy_choice(logits_fn(ids)))
        ids.append(out[-1])
        if out[-1] == eos or len(out) >= max_new or len(ids) >= max_ctx:
            return out
