"""Drafters of the speculative decode (`VQA_LLM.speculative_decode`).

A drafter is any `draft_fn(ids, d) -> list[int]`: `ids` are the sequence's un-expanded text ids (the prompt's input ids with the
<image> / <object> placeholders left out) followed by the tokens generated so far, `d` the number of draft tokens wanted; it
returns at most `d` guesses for the tokens that follow (fewer, or none, is fine).  Drafts are never trusted: the verify tail
(csrc/spec.hip) keeps only the prefix the model itself would have produced.  Host code, no model."""
from __future__ import annotations

from typing import Callable, List, Sequence

MAX_DRAFT = 15          # rows of one verify group: the current token + at most 15 drafts (VSTAR_VERIFY_MAX_GROUP)

DraftFn = Callable[[Sequence[int], int], List[int]]


def prompt_lookup_draft(ids: Sequence[int], d: int, max_ngram: int = 3) -> List[int]:
    """Prompt lookup (our own rule, not HF's `prompt_lookup_num_tokens` matcher): for n = max_ngram, ..., 1 take the last n ids
    as the suffix, find its most recent earlier occurrence that ends before the suffix starts (no overlap), and return the up to
    `d` ids that follow that occurrence.  The first n with a match wins; [] when nothing matches."""
    ids = list(ids)
    L = len(ids)
    if d <= 0:
        return []
    for n in range(min(max_ngram, L // 2), 0, -1):
        suffix = ids[L - n:]
        for s in range(L - 2 * n, -1, -1):          # the occurrence [s, s + n) ends at or before L - n
            if ids[s:s + n] == suffix:
                return ids[s + n:s + n + d]
    return []


def no_draft(ids: Sequence[int], d: int) -> List[int]:
    """The empty drafter: every step is a plain one-row decode step."""
    return []


class ReplayDrafter:
    """Proposes the continuation of a known output (benchmarks and tests): `targets[i]` is the token list sequence i is expected
    to generate after its prompt `prompts[i]`.  A share `corrupt` of the positions (chosen by a hash of the position, so the same
    on every call) is proposed wrong — (token + 1) % vocab — which fixes the acceptance rate: 0.0 = every draft right, 1.0 =
    every draft wrong."""

    def __init__(self, prompts: Sequence[Sequence[int]], targets: Sequence[Sequence[int]], vocab: int, corrupt: float = 0.0,
                 seed: int = 0):
        self.items = [(list(p), list(t)) for p, t in zip(prompts, targets)]
        self.vocab, self.corrupt, self.seed = int(vocab), float(corrupt), int(seed)

    def _wrong(self, pos: int) -> bool:
        if self.corrupt <= 0:
            return False
        h = (pos * 2654435761 + self.seed * 40503 + 12345) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 2246822519) & 0xFFFFFFFF
        h ^= h >> 13
        return (h & 0xFFFF) < self.corrupt * 65536.0

    def __call__(self, ids: Sequence[int], d: int) -> List[int]:
        ids = list(ids)
        for p, t in self.items:
            done = len(ids) - len(p)
            if done >= 0 and ids[:len(p)] == p and ids[len(p):] == t[:done]:
                return [(tok + 1) % self.vocab if self._wrong(done + j) else tok for j, tok in enumerate(t[done:done + d])]
        return []
