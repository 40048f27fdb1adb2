"""The CPU oracle of speculative decoding (tests/_spec_oracle.py) and the prompt-lookup drafter (vstar_amd/spec.py): the
speculative loop is lossless over a pure logits function, the sampled accept / residual rule preserves the kept distribution
over all 2^24 uniforms, and hand-worked drafter cases.  test_prompt_lookup_* and test_replay_drafter need vstar_amd/spec.py; the
others touch test code only."""
import numpy as np
import torch

from tests import _sampling_oracle as S
from tests import _spec_oracle as O

V, EOS = 50, 2


def _logits_fn(seed, eos_bias=0.0):
    def f(ids):       # a pure function of the ids: a hash seeds the row
        h = 1469598103934665603
        for t in list(ids)[-6:]:
            h = ((h ^ (int(t) + 1)) * 1099511628211) & ((1 << 64) - 1)
        r = np.random.default_rng((h + seed) & 0xFFFFFFFF).standard_normal(V)
        r[EOS] += eos_bias
        return r
    return f


def _run(f, prompt, max_new, d, draft_fn, max_ctx=1 << 30):
    def step(batch):
        return [np.stack([f(prefix + rows[:j + 1]) for j in range(len(rows))]) for _, rows, _, prefix in batch]
    outs, calls = O.spec_loop(step, [O.greedy_choice(f(prompt))], [prompt], [len(prompt)], max_new, d, draft_fn, EOS, V, max_ctx)
    return outs[0], calls


def test_speculative_loop_equals_plain_greedy():
    rng = np.random.default_rng(0)
    for seed in range(6):
        f = _logits_fn(seed, eos_bias=[0.0, 2.5][seed % 2])      # the biased runs meet EOS inside accepted drafts
        prompt = rng.integers(3, V, 7).tolist()
        for max_new in (1, 2, 9, 24):
            ref = O.plain_loop(f, prompt, max_new, EOS)
            full = O.plain_loop(f, prompt, 64, 10 ** 9)            # the EOS-free continuation: perfect drafts run through EOS

            def perfect(ids, k, full=full):
                done = len(ids) - len(prompt)
                return full[done:done + k]

            def adversarial(ids, k, full=full):                     # right up to a point that moves, then wrong
                done = len(ids) - len(prompt)
                g = full[done:done + k]
                j = done % (k + 1)
                return [(t + 1) % V if q >= j else t for q, t in enumerate(g)]

            def random_draft(ids, k):
                return np.random.default_rng(len(ids)).integers(0, V, k).tolist()

            for d in range(16):
                for name, fn in (("perfect", perfect), ("adversarial", adversarial), ("random", random_draft), ("none", lambda i, k: [])):
                    got, calls = _run(f, prompt, max_new, d, fn)
                    assert got == ref, (seed, max_new, d, name, got, ref)
                    if name == "perfect" and d >= 1 and len(ref) > 2:
                        assert calls < len(ref) - 1
                    if name == "none" or d == 0:
                        assert calls == len(ref) - 1
    # the context limit: the same tokens as the stepwise loop that stops at a full context
    f = _logits_fn(99)
    prompt = list(range(3, 12))
    full = O.plain_loop(f, prompt, 64, 10 ** 9)
    for max_ctx in (len(prompt) + 1, len(prompt) + 2, len(prompt) + 5, len(prompt) + 6):
        ref = O.plain_loop(f, prompt, 40, EOS, max_ctx)
        for d in (0, 1, 3, 6, 15):
            got, _ = _run(f, prompt, 40, d, lambda ids, k: full[len(ids) - len(prompt):len(ids) - len(prompt) + k], max_ctx)
            assert got == ref, (max_ctx, d, got, ref)


def test_greedy_choice_rule():
    assert O.greedy_choice([1.0, 3.0, 3.0, 2.0]) == 1
    assert O.greedy_choice([float("nan"), -float("inf"), -5.0]) == 2
    assert O.greedy_choice([float("nan"), float("nan")]) == 0
    assert O.greedy_choice([-float("inf")] * 3) == 0
    assert O.greedy_choice([float("nan"), float("inf"), float("inf")]) == 1
    assert O.verify_greedy(np.array([[0, 1.0], [1.0, 0], [0, 1.0]]), [1, 0, -1]) == (2, [1, 0, 1])
    assert O.verify_greedy(np.array([[0, 1.0], [1.0, 0], [0, 1.0]]), [1, 1, -1]) == (1, [1, 0, -1])
    assert O.verify_greedy(np.array([[0, 1.0], [1.0, 0], [0, 1.0]]), [0, 0, -1]) == (0, [1, -1, -1])
    assert O.verify_greedy(np.array([[0, 1.0]]), [-1]) == (0, [1])


def test_count_below_closed_form():
    rng = np.random.default_rng(1)
    for _ in range(200):
        Z = int(rng.integers(1, 1 << 62))
        t = int(rng.integers(0, Z + 1))
        n = O.count_below(t, Z)
        for u in {0, (1 << 24) - 1, max(n - 1, 0), min(n, (1 << 24) - 1)}:
            assert (((u * Z) >> 24) < t) == (u < n), (Z, t, u, n)


def test_sampled_rule_preserves_the_distribution():
    """Over all 2^24 values of u_a (and of u), in closed form on exact integer masses: P(token = y) = m_y / Z up to the 2^-24 grid of
    the uniforms — for a kept draft, an unkept draft, a kept set of {x} alone, and no draft."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(40, generator=g) * 2).half()
    s = S.scaled_scores(x, 0.8)
    keep, _ = S.kept(s, 12, 0.95)
    m = [int(v) for v in np.rint(S.masses(s) * keep * 2.0 ** 40)]
    Z = sum(m)
    kept_ids, unkept_ids = np.flatnonzero(keep), np.flatnonzero(~keep)
    for draft in (int(kept_ids[0]), int(kept_ids[-1]), int(np.argmax(m)), int(unkept_ids[0]), -1):
        p = O.first_token_distribution(m, draft)
        assert abs(p.sum() - 1) < 1e-12
        assert np.abs(p - np.array(m) / Z).max() <= 3 * 2.0 ** -24, (draft, np.abs(p - np.array(m) / Z).max())
        assert (p[~keep] == 0).all()
    one = [0, 0, 1 << 40, 0]                           # the kept set is {x}: every u_a accepts
    assert O.count_below(one[2], sum(one)) == 1 << 24
    assert O.first_token_distribution(one, 2).tolist() == [0, 0, 1, 0]
    # the closed form agrees with the rule itself on sampled uniforms
    rng = np.random.default_rng(5)
    draft = int(kept_ids[1])
    p = O.first_token_distribution(m, draft)
    n_acc = O.count_below(m[draft], Z)
    for ua in (0, n_acc - 1, n_acc, (1 << 24) - 1, *rng.integers(0, 1 << 24, 50).tolist()):
        tok, acc = O.verify_int(m, draft, int(ua), int(rng.integers(0, 1 << 24)))
        assert acc == (ua < n_acc) and (tok == draft) == acc and m[tok] > 0


def test_no_draft_is_the_sampling_oracles_draw():
    g = torch.Generator().manual_seed(8)
    for dtype in (torch.float16, torch.bfloat16):
        for seed in range(20):
            x = (torch.randn(300, generator=g) * 3).to(dtype)
            ref = S.sample_row(x, 0.7, 50, 0.9, S.uniform(seed, 4, 9))
            got = O.sampled_row(x, 0.7, 50, 0.9, seed, 4, 9, -1)
            assert got["token"] == ref["token"] and not got["accept"]
            a, toks, _ = O.verify_sampled([x], [-1], [(0.7, 50, 0.9, seed, 4, 9)])
            assert (a, toks) == (0, [ref["token"]])
            m = [int(v) for v in np.rint(ref["q"] * 2.0 ** 40)]
            u24 = int(S.uniform(seed, 4, 9) * 2 ** 24)
            if ref["u_dist"] > 1e-6:
                assert O.verify_int(m, -1, 0, u24) == (ref["token"], False)


def test_prompt_lookup_hand_cases():
    from vstar_amd.spec import prompt_lookup_draft as pl
    assert pl([1, 2, 3, 4, 5], 3) == []                                  # no match
    assert pl([], 3) == [] and pl([7], 3) == [] and pl([1, 2, 1], 0) == []
    # n = 3 beats a later n = 1: the trigram (1 2 3) occurred at 0; the unigram 3 also occurs later, at 5
    assert pl([1, 2, 3, 9, 8, 3, 7, 1, 2, 3], 2) == [9, 8]
    assert pl([1, 2, 3, 9, 8, 3, 7, 1, 2, 3], 2, max_ngram=1) == [7, 1]
    # the most recent match wins
    assert pl([5, 6, 10, 5, 6, 11, 5, 6], 1, max_ngram=2) == [11]
    # the match may not overlap the suffix: (7 7) at 1 overlaps the suffix (7 7) at 2; n = 2 fails, n = 1 matches at 2 (ends at 3)
    assert pl([4, 7, 7, 7], 3, max_ngram=2) == [7]
    assert pl([7, 7, 7, 7], 3, max_ngram=2) == [7, 7]                   # (7 7) at 0 ends where the suffix starts: allowed
    # fewer than d ids follow
    assert pl([1, 2, 3, 1, 2], 8) == [3, 1, 2]
    assert pl([1, 2, 3, 1, 2], 2) == [3, 1]


def test_replay_drafter():
    from vstar_amd.spec import ReplayDrafter, no_draft
    r = ReplayDrafter([[1, 2]], [[5, 6, 7, 8]], vocab=10)
    assert r([1, 2, 5], 2) == [6, 7] and r([1, 2], 9) == [5, 6, 7, 8] and r([1, 2, 9], 2) == [] and r([3], 2) == []
    w = ReplayDrafter([[1, 2]], [[5, 6, 7, 9]], vocab=10, corrupt=1.0)
    assert w([1, 2], 4) == [6, 7, 8, 0]
    h = ReplayDrafter([[1]], [list(range(2, 9)) * 40], vocab=10, corrupt=0.5)
    wrong = sum(a != b for a, b in zip(h([1], 280), list(range(2, 9)) * 40))
    assert 100 < wrong < 180
    assert no_draft([1, 2, 1], 3) == []
