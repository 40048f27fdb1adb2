"""Host side of beam search: HF 4.31 `BeamSearchScorer` / `BeamHypotheses` (rules 4-8 of the contract) over
the candidates the device select (csrc/beam.hip) returns, one `BeamSearch` per sample.

Lengths are those of HF's `input_ids`: the UN-expanded prompt ids (one id per <image> / <object> placeholder) plus the tokens
generated so far — not the KV positions, which count every feature row of an image."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

EarlyStopping = Union[bool, str]
START_SCORE = -1e9          # beam_scores[:, 1:] of HF 4.31 beam_search


class BeamHypotheses:
    """transformers 4.31 generation/beam_search.py::BeamHypotheses: the k best finished hypotheses of one sample."""

    def __init__(self, num_beams: int, length_penalty: float, early_stopping: EarlyStopping, max_length: Optional[int]):
        self.num_beams = num_beams
        self.length_penalty = length_penalty
        self.early_stopping = early_stopping
        self.max_length = max_length
        self.beams: List[Tuple[float, List[int]]] = []
        self.worst_score = 1e9

    def __len__(self) -> int:
        return len(self.beams)

    def add(self, hyp: List[int], length: int, sum_logprobs: float) -> None:
        """hyp: the generated ids of the hypothesis; length: its full un-expanded length (prompt ids + hyp)."""
        score = sum_logprobs / (length ** self.length_penalty)
        if len(self) < self.num_beams or score > self.worst_score:
            self.beams.append((score, list(hyp)))
            if len(self) > self.num_beams:
                ranked = sorted([(s, i) for i, (s, _) in enumerate(self.beams)])
                del self.beams[ranked[0][1]]
                self.worst_score = ranked[1][0]
            else:
                self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs: float, cur_len: int) -> bool:
        if len(self) < self.num_beams:
            return False
        if self.early_stopping is True:
            return True
        if self.early_stopping is False:
            return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty
        if self.length_penalty > 0.0:             # "never"
            return self.worst_score >= best_sum_logprobs / self.max_length ** self.length_penalty
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty


class BeamSearch:
    """One sample's beam search state: k running beams (generated ids, fp32 cumulative scores), the finished hypotheses.

    step protocol: the device select returns the sample's 2k candidates (score, token, parent beam) sorted by rank;
    `process` turns them into the next k running beams and returns each new beam's parent, so the caller can reorder the KV
    ancestry and feed the new tokens."""

    def __init__(self, num_beams: int, prompt_len: int, eos_token_id: int, max_length: int, length_penalty: float = 1.0,
                 early_stopping: EarlyStopping = False):
        if early_stopping not in (True, False, "never"):
            raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        self.k = num_beams
        self.prompt_len = prompt_len
        self.eos = eos_token_id
        self.max_length = max_length
        self.hyps = BeamHypotheses(num_beams, length_penalty, early_stopping, max_length)
        self.tokens: List[List[int]] = [[] for _ in range(num_beams)]
        self.scores = np.full(num_beams, START_SCORE, np.float32)
        self.scores[0] = 0.0
        self.done = False

    @property
    def cur_len(self) -> int:
        """Un-expanded length of every running beam (HF input_ids.shape[-1])."""
        return self.prompt_len + len(self.tokens[0])

    def process(self, cand_scores: Sequence[float], cand_tokens: Sequence[int], cand_beams: Sequence[int]) -> List[int]:
        """BeamSearchScorer.process for this sample: cand_* are the 2k candidates in rank order.  Returns the parent of each of
        the k new running beams (their tokens and scores are now in self.tokens / self.scores)."""
        cur_len = self.cur_len
        new_tokens: List[List[int]] = []
        new_scores: List[np.float32] = []
        parents: List[int] = []
        for rank, (s, t, b) in enumerate(zip(cand_scores, cand_tokens, cand_beams)):
            s, t, b = np.float32(s), int(t), int(b)
            if t == self.eos:
                if rank >= self.k:
                    continue
                self.hyps.add(self.tokens[b], cur_len, float(s))
            else:
                new_tokens.append(self.tokens[b] + [t])
                new_scores.append(s)
                parents.append(b)
            if len(parents) == self.k:
                break
        if len(parents) < self.k:
            raise ValueError(f"beam search: {len(cand_scores)} candidates left fewer than {self.k} running beams")
        self.tokens = new_tokens
        self.scores = np.asarray(new_scores, np.float32)
        best = float(np.max(np.asarray(cand_scores, np.float32)))
        self.done = self.done or self.hyps.is_done(best, cur_len)
        return parents

    def finalize(self, num_return_sequences: int = 1) -> List[List[int]]:
        """BeamSearchScorer.finalize: the generated ids (after the prompt) of the num_return_sequences best hypotheses, each
        with EOS appended below the common length and padded with EOS (4.31 with pad_token_id unset)."""
        if num_return_sequences > self.k:
            raise ValueError("num_return_sequences must be <= num_beams")
        if not self.done:
            for b in range(self.k):
                self.hyps.add(self.tokens[b], self.cur_len, float(self.scores[b]))
        ranked = sorted(self.hyps.beams, key=lambda x: x[0])
        best = [ranked.pop()[1] for _ in range(num_return_sequences)]
        lengths = [self.prompt_len + len(h) for h in best]
        sent_max_len = min(max(lengths) + 1, self.max_length) if self.max_length is not None else max(lengths) + 1
        out = []
        for h, n in zip(best, lengths):
            row = list(h)
            if n < sent_max_len:
                row.append(self.eos)
            row += [self.eos] * (sent_max_len - self.prompt_len - len(row))
            out.append(row)
        return out
