"""CPU oracle of the logits-edit stage (csrc/edit.hip) and of `LogitRules.plan` (vstar_amd/logits.py): a numpy /
torch-CPU restatement written from the contract, not from the code under test.  No transformers import here: the comparison with
HF's classes lives in tests/test_logit_rules_oracle.py.

Edit of one row x (torch fp16 / bf16 tensor, [V]) with lists (penalised, theta, banned, allowed):
  1. penalised t:  x[t] = T(f32(x[t]) < 0 ? f32(x[t]) * f32(theta) : f32(x[t]) / f32(theta))   (IEEE fp32, one RNE rounding to T)
  2. banned t:     x[t] = -inf
  3. allowed non-empty:  x[t] = -inf for every t not in it
"""
import numpy as np
import torch


def penalise(x: torch.Tensor, theta: float) -> torch.Tensor:
    """Step 1 on every element of x (fp16 / bf16): fp32 arithmetic with theta rounded to fp32, one rounding to x's type."""
    f = x.to(torch.float32)
    th = torch.tensor(np.float32(theta), dtype=torch.float32)
    return torch.where(f < 0, f * th, f / th).to(x.dtype)


def edit_row(x: torch.Tensor, pen, theta, ban, allow) -> torch.Tensor:
    y = x.clone()
    if len(pen):
        idx = torch.as_tensor(sorted(set(int(t) for t in pen)), dtype=torch.long)
        y[idx] = penalise(x[idx], theta)
    if len(ban):
        y[torch.as_tensor(sorted(set(int(t) for t in ban)), dtype=torch.long)] = float("-inf")
    if len(allow):
        keep = torch.zeros(x.shape[0], dtype=torch.bool)
        keep[torch.as_tensor(sorted(set(int(t) for t in allow)), dtype=torch.long)] = True
        y[~keep] = float("-inf")
    return y


def edit_rows(x: torch.Tensor, plans) -> torch.Tensor:
    """x [rows, V]; plans[j] = (penalised, theta, banned, allowed)."""
    return torch.stack([edit_row(x[j], *plans[j]) for j in range(x.shape[0])])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equality of two 16-bit float tensors, except that any NaN equals any NaN (IEEE leaves the payload of an
    arithmetic NaN to the implementation; the contract says 'NaN stays NaN')."""
    ai, bi = a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool((na == nb).all() and (ai[~na] == bi[~nb]).all())


def plan(history, n_generated, eos_id, *, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=(), min_new_tokens=0,
         suppress_tokens=(), allowed_tokens_fn=None, batch_id=0):
    """The lists of the row that follows `history` (ids < 0 — image / object placeholders — are no tokens and are left out)."""
    h = [t for t in history if t >= 0]
    pen = set(h) if repetition_penalty != 1.0 else set()
    ban = set(suppress_tokens)
    n = no_repeat_ngram_size
    if n > 0:
        # every n-gram of the history whose first n - 1 tokens are the history's last n - 1 tokens bans its last token
        grams = [tuple(h[i:i + n]) for i in range(len(h) - n + 1)]
        tail = tuple(h[len(h) - n + 1:]) if n > 1 else ()
        for gram in grams:
            if gram[:-1] == tail:
                ban.add(gram[-1])
    for w in bad_words_ids:
        w = list(w)
        if len(w) == 1:
            if w[0] != eos_id:
                ban.add(w[0])
        elif len(w) <= len(h) and h[-(len(w) - 1):] == w[:-1]:
            ban.add(w[-1])
    if n_generated < min_new_tokens and eos_id is not None:
        ban.add(eos_id)
    allow = set()
    if allowed_tokens_fn is not None:
        allow = set(int(t) for t in allowed_tokens_fn(batch_id, list(h)))
        if not allow:
            raise ValueError("empty allow list")
    return sorted(pen), float(repetition_penalty), sorted(ban), sorted(allow)


def first_argmax(x) -> int:
    """argmax_rows_lp's rule: the first index of the largest number; NaN and -inf never win; 0 when nothing does."""
    x = np.asarray(x, np.float32)
    ok = ~np.isnan(x) & (x > -np.inf)
    if not ok.any():
        return 0
    m = x[ok].max()
    return int(np.flatnonzero(ok & (x == m))[0])
