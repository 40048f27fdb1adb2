"""`LogitRules` — HF generate's logits-processor list as the three token lists per row that the engine's edit stage applies on
the device (csrc/edit.hip): a penalised list with one theta (repetition_penalty), a banned list
(no_repeat_ngram_size, bad_words_ids, min_new_tokens, suppress_tokens) and an allowed list (prefix_allowed_tokens_fn).

The device applies, per row: the penalty to every penalised id, then -inf to every banned id, then -inf to every id outside a
non-empty allowed list.  HF chains one class per rule in the order generate() builds them; under these semantics the order does
not change the result: the penalty only rescales finite values of ids that stay finite, every other rule only writes -inf, and
-inf is absorbing (a penalised -inf stays -inf: -inf * theta = -inf for theta > 0).  tests/test_logit_rules_oracle.py checks this
against the chained HF classes, bit for bit.

History.  `history` is the sequence's TEXT ids in order — the prompt with the <image> / <object> placeholders (ids < 0) left out —
followed by what it has generated: what the speculative drafter sees (VQA_LLM.speculative_decode).  The reference cannot express a
multimodal prompt here at all (HF's gather would index the logits with -200), so this is a definition, not a parity claim: image
and object features are no tokens, are never penalised and never take part in an n-gram or a bad-word prefix; the text on either
side of a placeholder is adjacent.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

Plan = Tuple[List[int], float, List[int], List[int]]


class LogitRules:
    def __init__(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, bad_words_ids=None, min_new_tokens: int = 0,
                 suppress_tokens=None, allowed_tokens_fn: Optional[Callable[[int, List[int]], Sequence[int]]] = None):
        """The constructor validates as HF's classes do: repetition_penalty > 0 (1.0 = off), no_repeat_ngram_size and
        min_new_tokens integers >= 0 (0 = off), bad_words_ids a non-empty list of non-empty lists of ids >= 0 (or None)."""
        if isinstance(repetition_penalty, bool) or not isinstance(repetition_penalty, (int, float)) or not repetition_penalty > 0 \
                or repetition_penalty == float("inf"):
            raise ValueError(f"`repetition_penalty` has to be a strictly positive finite float, but is {repetition_penalty!r}")
        for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError(f"`{name}` has to be an integer >= 0, but is {v!r}")
        if bad_words_ids is not None:
            if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
                raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids!r}")
            for w in bad_words_ids:
                if not isinstance(w, (list, tuple)) or len(w) == 0 or any(
                        isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0 for t in w):
                    raise ValueError(f"each entry of `bad_words_ids` has to be a non-empty list of ids >= 0, but is {bad_words_ids!r}")
        if suppress_tokens is not None and any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or t < 0 for t in suppress_tokens):
            raise ValueError(f"`suppress_tokens` has to be a list of ids >= 0, but is {suppress_tokens!r}")
        if allowed_tokens_fn is not None and not callable(allowed_tokens_fn):
            raise ValueError("`allowed_tokens_fn` has to be callable: (batch_id, history ids) -> allowed ids")
        self.repetition_penalty = float(repetition_penalty)
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)
        self.bad_words_ids = [[int(t) for t in w] for w in bad_words_ids] if bad_words_ids is not None else []
        self.min_new_tokens = int(min_new_tokens)
        self.suppress_tokens = sorted({int(t) for t in suppress_tokens}) if suppress_tokens is not None else []
        self.allowed_tokens_fn = allowed_tokens_fn

    @property
    def active(self) -> bool:
        """False when every rule is at its default: no edits are built and the engine calls are the plain ones."""
        return bool(self.repetition_penalty != 1.0 or self.no_repeat_ngram_size or self.bad_words_ids or self.min_new_tokens
                    or self.suppress_tokens or self.allowed_tokens_fn is not None)

    def plan(self, history: Sequence[int], n_generated: int, eos_id: Optional[int], batch_id: int = 0) -> Plan:
        """The edits of the row that chooses the token behind `history` (text ids, placeholders left out, generated tokens
        appended; see the module docstring), `n_generated` of which are generated: (penalised, theta, banned, allowed), sorted
        de-duplicated int lists.
          penalty     once per distinct history token (RepetitionPenaltyLogitsProcessor)
          n-gram      every t that would complete an n-gram already in history (NoRepeatNGramLogitsProcessor)
          bad words   a single-token word always (unless it is [eos_id], which HF filters out); a multi-token word no longer than
                      the history bans its last token when history ends with its prefix (NoBadWordsLogitsProcessor)
          EOS         banned while n_generated < min_new_tokens (MinNewTokensLengthLogitsProcessor)
          suppress    always banned (SuppressTokensLogitsProcessor)
          allowed     allowed_tokens_fn(batch_id, history); an empty list raises (PrefixConstrainedLogitsProcessor)"""
        h = [int(t) for t in history if int(t) >= 0]
        pen = sorted(set(h)) if self.repetition_penalty != 1.0 else []
        ban = set(self.suppress_tokens)
        n = self.no_repeat_ngram_size
        if n == 1:
            ban.update(h)
        elif n == 2 and len(h) >= 2:
            last = h[-1]
            ban.update(b for a, b in zip(h, h[1:]) if a == last)
        elif n and len(h) >= n:              # every window whose first n - 1 tokens are the history's last n - 1 bans its last token
            prefix = tuple(h[len(h) - (n - 1):])
            for w in zip(*[h[j:len(h) - n + 1 + j] for j in range(n)]):
                if w[:-1] == prefix:
                    ban.add(w[-1])
        for w in self.bad_words_ids:
            if len(w) == 1:
                if eos_id is None or w[0] != eos_id:
                    ban.add(w[0])
            elif len(w) <= len(h) and h[len(h) - (len(w) - 1):] == w[:-1]:
                ban.add(w[-1])
        if eos_id is not None and n_generated < self.min_new_tokens:
            ban.add(int(eos_id))
        allowed: List[int] = []
        if self.allowed_tokens_fn is not None:
            allowed = sorted({int(t) for t in self.allowed_tokens_fn(batch_id, list(h))})
            if not allowed:
                raise ValueError(f"`allowed_tokens_fn` returned an empty list for batch ID {batch_id}: the constraint is unsatisfiable")
        return pen, self.repetition_penalty, sorted(ban), allowed

    @staticmethod
    def pack(plans: Sequence[Plan]):
        """The CSR arrays of one engine call, one plan per wanted row in order: (off int32 [3 n + 1], tok int32 [off[-1]], penalty
        float32 [n]) — vstar_vqa_logit_edits (include/vstar_vqa.h).  The lists are sorted and de-duplicated here too, so plans
        built by hand pack to valid arrays; id range and theta are checked by the engine (vstar_edit_check)."""
        off = np.zeros(3 * len(plans) + 1, np.int32)
        parts, pen = [], np.ones(len(plans), np.float32)
        total = 0
        for j, (p, theta, b, a) in enumerate(plans):
            for l, ids in enumerate((p, b, a)):
                ids = np.unique(np.asarray(list(ids), np.int64))
                if ids.size and (ids[0] < -2 ** 31 or ids[-1] >= 2 ** 31):
                    raise ValueError("token ids must fit in int32")
                parts.append(ids.astype(np.int32))
                total += ids.size
                if total >= 2 ** 31:
                    raise ValueError("too many token ids for one call")
                off[3 * j + l + 1] = total
            pen[j] = theta
        tok = np.concatenate(parts) if parts else np.zeros(0, np.int32)
        return off, np.ascontiguousarray(tok, np.int32), pen


def rules_from_kwargs(repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0, suppress_tokens=None,
                      allowed_tokens_fn=None) -> Optional[LogitRules]:
    """The public keywords of free_form_inference / free_form_batch / generate -> LogitRules (validated), or None when every one is
    at its default (no edits are built: the calls are the plain ones)."""
    r = LogitRules(1.0 if repetition_penalty is None else repetition_penalty, no_repeat_ngram_size or 0, bad_words_ids,
                   min_new_tokens or 0, suppress_tokens, allowed_tokens_fn)
    return r if r.active else None


BEAM_RULES_MESSAGE = ("logits rules (repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_new_tokens, suppress_tokens, "
                      "allowed_tokens_fn) with num_beams > 1 are not implemented: HF applies the processors to the log-softmax "
                      "output in beam search, using the log-sum-exp of the unedited row, which editing the logits ahead of the "
                      "on-device beam select would not reproduce")
