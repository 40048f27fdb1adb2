"""Block-scaled fp8 KV cache (MX e4m3, blocks of 32) on the GPU: the quantiser against the oracle bit for bit, every
writer pinned to the oracle through the decoded cache, the fp8-storage engine (format 1) bit-identical to the engine that holds the
same values in its fp16 cache (format 2) in every kind of call, the tails and drivers on the format-1 engine, and a loose net against
the chain oracle.  All engines: VQAConfig.tiny(llm_hidden=512, llm_heads=4, llm_mlp=1024, max_slots=12): with 4 heads a decode step of
one sequence of 256 or more keys takes the split-KV kernels."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from oracle import vqa_oracle as O
from tests._kv8_oracle import kv8_quantize, kv8_round_trip, llama_forward_kv8, rel_l2
from vstar_amd import _lib
from vstar_amd.config import KVFMT_MXFP8, KVFMT_MXFP8_EMULATED, VQAConfig
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
U = 2.0 ** -24


def _cfg(fmt, bits=0):
    return dataclasses.replace(VQAConfig.tiny(llm_hidden=512, llm_heads=4, llm_mlp=1024, max_slots=12).with_decode_bits(bits),
                               kv_cache_format=fmt)


def _build(fmt, sd, bits=0):
    eng = VqaEngine(_cfg(fmt, bits), 0)
    eng.load_state_dict(sd)
    return eng


def _prompts(n, length, seed):
    g = torch.Generator().manual_seed(seed)
    return [[1] + torch.randint(3, 300, (length - 1 + i,), generator=g).tolist() for i in range(n)]


def _prefill_and_steps(eng, prompts, steps, seed=5):
    """Ragged prefill of len(prompts) sequences, then `steps` teacher-forced one-token steps of all of them: [logits ...]."""
    n = len(prompts)
    out = [eng.forward([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [(i, -1) for i in range(n)])[0]]
    g = torch.Generator().manual_seed(seed)
    for t in range(steps):
        toks = torch.randint(3, 300, (n,), generator=g).tolist()
        out.append(eng.forward([Seq([toks[i]], kv_slot=i, past_len=len(prompts[i]) + t) for i in range(n)], [(i, 0) for i in range(n)])[0])
    return out


def _same(a, b):
    return all(np.array_equal(x.view(np.int16), y.view(np.int16)) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def engines(cuda):
    sd = random_state_dict(_cfg(0), seed=3, dtype=torch.float16)
    off_before = _build(0, sd)                        # built (and run) before any engine of the new formats exists in the process
    base = _prefill_and_steps(off_before, _prompts(3, 30, 1), 2)
    return {"sd": sd, "off_before": off_before, "base": base, 0: off_before, 1: _build(KVFMT_MXFP8, sd), 2: _build(KVFMT_MXFP8_EMULATED, sd)}


# ------------------------------------------------ 1. quantiser ------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 300])
def test_quantiser_matches_oracle_bit_for_bit(cuda, lib, rows):
    g = np.random.default_rng(rows)
    x = g.standard_normal((rows, 128)).astype(np.float32)
    kinds = np.arange(rows) % 8
    x[kinds == 1, 17] *= 30                                                      # one loud channel
    x[kinds == 2, 32:64] = 0                                                     # an all-zero block
    x[kinds == 3] = 0                                                            # an all-zero row
    x[kinds == 4] = g.integers(-1023, 1024, (int((kinds == 4).sum()), 128)) * U  # subnormal-only blocks
    x[kinds == 5] *= np.exp2(g.integers(-14, 13, (int((kinds == 5).sum()), 1)))  # magnitudes up to 2^15
    x = np.clip(x, -2.0 ** 15, 2.0 ** 15).astype(np.float16)
    for r in np.nonzero(kinds == 6)[0]:                                          # block maxima of exactly 448 x 2^n ...
        n = int(g.integers(-12, 7))
        x[r] = (np.clip(x[r].astype(np.float32), -1, 1) * 100 * 2.0 ** n).astype(np.float16)
        x[r, [3, 40, 70, 127]] = np.float16(448 * 2.0 ** n) * np.array([1, -1, 1, -1], np.float16)
    for r in np.nonzero(kinds == 7)[0]:                                          # ... and of the next fp16 above that
        n = int(g.integers(-12, 7))
        x[r] = (np.clip(x[r].astype(np.float32), -1, 1) * 100 * 2.0 ** n).astype(np.float16)
        up = np.nextafter(np.float16(448 * 2.0 ** n), np.float16(np.inf))
        x[r, [3, 40, 70, 127]] = up * np.array([1, -1, 1, -1], np.float16)
    assert np.abs(x.astype(np.float32)).max() <= 2.0 ** 15
    co, eo, xo = kv8_quantize(x)
    if rows >= 8:
        r6, r7 = int(np.nonzero(kinds == 6)[0][0]), int(np.nonzero(kinds == 7)[0][0])
        assert (co[r6, [3, 40, 70, 127]] & 0x7F == 0x7E).all()                   # 448 itself: the top code, no saturation
        assert (co[r7, [3, 40, 70, 127]] & 0x7F != 0x7E).all()                   # one ulp more: the next power of two
    xd = torch.from_numpy(x).cuda()
    codes = torch.full((rows, 128), 0x55, dtype=torch.uint8, device="cuda")
    sc = torch.full((rows, 4), 0x55, dtype=torch.uint8, device="cuda")
    xhat = torch.full((rows, 128), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_kv_quantize(P(xd), rows, P(codes), P(sc), P(xhat)) == 0, lib.vstar_vqa_last_error(None)
    assert np.array_equal(sc.cpu().numpy(), eo)
    assert np.array_equal(codes.cpu().numpy(), co)
    assert np.array_equal(xhat.cpu().numpy().view(np.int16), xo.view(np.int16))
    # without xhat, and in place (xhat aliases x)
    c2, s2 = torch.zeros_like(codes), torch.zeros_like(sc)
    assert lib.vstar_vqa_op_kv_quantize(P(xd), rows, P(c2), P(s2), None) == 0
    assert torch.equal(c2, codes) and torch.equal(s2, sc)
    assert lib.vstar_vqa_op_kv_quantize(P(xd), rows, P(c2), P(s2), P(xd)) == 0
    assert torch.equal(c2, codes) and np.array_equal(xd.cpu().numpy().view(np.int16), xo.view(np.int16))


# ------------------------------------------------ 2. writers ------------------------------------------------
def _writer_calls(eng):
    """Every writer of the cache, layer 0's K and V of which do not depend on the cache format (they are functions of the new rows'
    embeddings alone).  Returns {slot: written positions}."""
    pr = _prompts(3, 20, 31)                                          # ragged prefill: rope_kv_append
    eng.forward([Seq(p, kv_slot=i) for i, p in enumerate(pr)], [(0, -1)], logits=False)
    for t in range(2):                                                # one-token steps: the fused unsplit writer
        eng.forward([Seq([5 + t + i], kv_slot=i, past_len=len(pr[i]) + t) for i in range(3)], [(0, 0)], logits=False)
    long = _prompts(1, 300, 32)[0]                                    # 300 keys, one sequence: the split kernels' writer
    eng.forward([Seq(long, kv_slot=3)], [(0, -1)], logits=False)
    for t in range(2):
        eng.forward([Seq([9 + t], kv_slot=3, past_len=300 + t)], [(0, 0)], logits=False)
    eng.forward([Seq([11, 12, 13, 14], kv_slot=0, past_len=len(pr[0]) + 2)], [(0, -1)], logits=False)      # a 4-row continuation
    return {0: len(pr[0]) + 6, 1: len(pr[1]) + 2, 2: len(pr[2]) + 2, 3: 302}


def test_writers_store_the_oracle_round_trip(engines):
    written = _writer_calls(engines[0])
    for fmt in (1, 2):
        assert _writer_calls(engines[fmt]) == written
    for slot, n in written.items():
        ref = engines[0].kv_rows(0, slot)[:, :, :n]
        want = kv8_round_trip(torch.from_numpy(ref.copy())).numpy()
        assert not np.array_equal(want, ref) and np.abs(ref).max() > 0
        for fmt in (1, 2):
            got = engines[fmt].kv_rows(0, slot)[:, :, :n]
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (fmt, slot)


# ------------------------------------------------ 3. format 1 == format 2 ------------------------------------------------
def test_prefill_is_bit_identical_between_storage_and_emulation(engines):
    pr = _prompts(1, 96, 2)[0]
    la = engines[1].forward([Seq(pr, kv_slot=0)], [(0, -1), (0, 10)])[0]
    lb = engines[2].forward([Seq(pr, kv_slot=0)], [(0, -1), (0, 10)])[0]
    l0 = engines[0].forward([Seq(pr, kv_slot=0)], [(0, -1), (0, 10)])[0]
    assert np.isfinite(la.astype(np.float32)).all()
    assert np.array_equal(la.view(np.int16), lb.view(np.int16))
    assert not np.array_equal(la.view(np.int16), l0.view(np.int16))      # ... and the quantised cache is not the fp16 one
    assert engines[1].kv_cache_format() == 1 and engines[2].kv_cache_format() == 2 and engines[0].kv_cache_format() == 0


@pytest.mark.parametrize("nseq,prompt,steps", [(1, 96, 4), (1, 300, 3), (1, 255, 2), (3, 30, 4), (12, 8, 1)])
def test_decode_is_bit_identical_between_storage_and_emulation(engines, nseq, prompt, steps):
    """The unsplit fused kernel, the split kernels (300 keys: trailing partitions empty; 255 -> 256: the crossing) and 12 sequences."""
    pr = _prompts(nseq, prompt, 10 + nseq + prompt)
    la = _prefill_and_steps(engines[1], pr, steps)
    lb = _prefill_and_steps(engines[2], pr, steps)
    l0 = _prefill_and_steps(engines[0], pr, steps)
    for t in range(steps + 1):
        assert np.array_equal(la[t].view(np.int16), lb[t].view(np.int16)), (nseq, prompt, t)
    assert not _same(la, l0)


def _forks_reorder_copy(eng, ctx_len):
    """Options forked from a question prefix (multi-row continuations), a step after kv_reorder with a swap, a step after kv_copy."""
    out = []
    q = _prompts(1, ctx_len, 40 + ctx_len)[0]
    out.append(eng.forward([Seq(q, kv_slot=0)], [(0, -1)])[0])
    opts = [[21, 22, 23, 24], [31, 32, 33, 34, 35], [41, 42, 43]]
    out.append(eng.forward([Seq(o, kv_slot=1 + i, past_len=len(q), prefix_slot=0) for i, o in enumerate(opts)],
                           [(i, r) for i, o in enumerate(opts) for r in range(len(o))])[0])
    # two beams of the question: slot 4 shares slot 0's rows through the ancestry table, both step, then they swap
    eng.kv_reorder([4], [0], 0, len(q))
    out.append(eng.forward([Seq([50], kv_slot=0, past_len=len(q)), Seq([51], kv_slot=4, past_len=len(q))], [(0, 0), (1, 0)])[0])
    eng.kv_reorder([0, 4], [4, 0], 0, len(q) + 1)
    out.append(eng.forward([Seq([52], kv_slot=0, past_len=len(q) + 1), Seq([53], kv_slot=4, past_len=len(q) + 1)], [(0, 0), (1, 0)])[0])
    # detach beam 4 into slot 5 (codes AND scale bytes move), continue it there
    eng.kv_copy(5, 4, 0, len(q) + 2)
    out.append(eng.forward([Seq([54], kv_slot=5, past_len=len(q) + 2)], [(0, 0)])[0])
    out.append(eng.forward([Seq([55, 56, 57], kv_slot=5, past_len=len(q) + 3)], [(0, 0), (0, 2)])[0])
    out.append(eng.forward([Seq([58], kv_slot=4, past_len=len(q) + 2)], [(0, 0)])[0])
    return out


@pytest.mark.parametrize("ctx_len", [40, 270])
def test_forks_reorder_and_copy_are_bit_identical_between_storage_and_emulation(engines, ctx_len):
    la = _forks_reorder_copy(engines[1], ctx_len)
    lb = _forks_reorder_copy(engines[2], ctx_len)
    for t, (x, y) in enumerate(zip(la, lb)):
        assert np.isfinite(x.astype(np.float32)).all()
        assert np.array_equal(x.view(np.int16), y.view(np.int16)), (ctx_len, t)
    # ... and none of it is what the fp16 cache computes
    assert not _same(la, _forks_reorder_copy(engines[0], ctx_len))


@pytest.mark.parametrize("bits", [8, 4])
def test_weight_modes_combine_with_the_kv_format(engines, bits):
    a, b = _build(1, engines["sd"], bits), _build(2, engines["sd"], bits)
    assert a.decode_weight_bits() == bits and a.kv_cache_format() == 1 and b.kv_cache_format() == 2
    for pr, steps in ((_prompts(1, 260, 61), 2), (_prompts(3, 30, 62), 2)):
        la, lb = _prefill_and_steps(a, pr, steps), _prefill_and_steps(b, pr, steps)
        for t in range(steps + 1):
            assert np.array_equal(la[t].view(np.int16), lb[t].view(np.int16)), (bits, t)


# ------------------------------------------------ 4. tails and drivers ------------------------------------------------
def test_greedy_decode_and_tails_on_the_fp8_kv_engine(engines, lib):
    from tests.test_beam_gpu import op_select
    from tests.test_sampling_gpu import op_sample
    from tests.test_score_gpu import op_score
    from vstar_amd.vqa import VQA_LLM
    a = engines[1]
    cfg = a.cfg
    pr = _prompts(1, 70, 21)[0]
    llm = VQA_LLM(cfg=cfg, engine=a, kv_cache_bits=8)
    got = llm.greedy_decode([Seq(pr, kv_slot=0)], [len(pr)], 6)[0]          # (the captured greedy step)
    lg, _ = a.forward([Seq(pr, kv_slot=1)], [(0, -1)])
    want, past = [], len(pr)
    for _ in range(6):
        tok = int(np.argmax(lg[0].astype(np.float32)))
        want.append(tok)
        if tok == llm.eos_token_id:
            break
        lg, _ = a.forward([Seq([tok], kv_slot=1, past_len=past)], [(0, 0)])
        past += 1
    assert got[:len(want)] == want and len(got) == len(want)
    # the tails on a 3-sequence decode step: what their op-level entries give on the logits forward returns for the same arguments
    prs = _prompts(3, 30, 22)
    a.forward([Seq(p, kv_slot=i) for i, p in enumerate(prs)], [(0, -1)])
    step = [Seq([7 + i], kv_slot=i, past_len=len(prs[i])) for i in range(3)]
    wanted = [(i, 0) for i in range(3)]
    lg, _ = a.forward(step, wanted)
    x = torch.from_numpy(lg).cuda()
    prm = [_lib.VqaSampling(0.8, 20, 0.9, 3, 1234, i) for i in range(3)]
    assert a.forward_sample(step, wanted, prm).tolist() == op_sample(lib, x, prm)[0].tolist()
    sc = np.asarray([0.0, -0.5, -1.25], np.float32)
    cs, ct, cr, _ = a.forward_beam(step, wanted, sc, [0, 3], 6)
    os_, ot, orow, _ = op_select(lib, x, sc, [0, 3], 6, want_lp=False)
    assert np.array_equal(cs, os_) and np.array_equal(ct, ot) and np.array_equal(cr, orow)
    tg = [5, 100, 319]
    nll, rk = a.forward_score(step, wanted, tg, rank=True)
    onll, ork, _ = op_score(lib, x, tg)
    assert np.array_equal(nll, onll) and np.array_equal(rk, ork)
    # a verify step against the greedy rule
    _, first = a.forward([Seq(pr, kv_slot=2)], [(0, -1)], logits=False)
    _, am = a.forward([Seq([int(first[0]), 11, 12, 13], kv_slot=2, past_len=len(pr))], [(0, r) for r in range(4)], logits=False)
    for drafts in ([int(am[0]), int(am[1]), (int(am[2]) + 1) % 300], [(int(am[0]) + 1) % 300, 12, 13]):
        rows = [int(first[0])] + drafts
        w4 = [(0, r) for r in range(4)]
        _, am2 = a.forward([Seq(rows, kv_slot=2, past_len=len(pr))], w4, logits=False)
        acc, tok = a.forward_verify([Seq(rows, kv_slot=2, past_len=len(pr))], w4, [0, 4], drafts + [-1])
        n = 0
        while n < 3 and drafts[n] == int(am2[n]):
            n += 1
        assert int(acc[0]) == n and tok.tolist() == [int(t) for t in am2[:n + 1]] + [-1] * (3 - n)
    # one beam search and one speculative decode, to completion
    beams = llm.beam_decode([Seq(pr, kv_slot=0)], [len(pr)], [len(pr)], 5, 3)
    assert len(beams) == 1 and len(beams[0]) == 1 and 1 <= len(beams[0][0]) <= 5 and all(0 <= t < cfg.llm_vocab for t in beams[0][0])
    spec = llm.speculative_decode([Seq(pr, kv_slot=3)], [len(pr)], [pr], 6, 3)
    assert len(spec) == 1 and 1 <= len(spec[0]) <= 6 and all(0 <= t < cfg.llm_vocab for t in spec[0])
    assert llm.spec_stats["tokens"] == len(spec[0])


# ------------------------------------------------ 5. loose net against the chain oracle ------------------------------------------------
def test_engine_against_the_chain_oracle(engines):
    """test_vqa_gpu.py's gate form: rel_L2(engine format 1, fp32 kv8 oracle) <= max(5e-3, 3 x noise), noise = the fp16 kv8 oracle
    against the fp32 one (about 8e-3: code flips amplify fp16 noise, so the gate is loose by construction)."""
    cfg = _cfg(1)
    sd16 = engines["sd"]
    sd32 = {k: v.float() for k, v in sd16.items()}
    pr = _prompts(1, 96, 2)[0]
    ids = torch.tensor(pr)
    ref, past = llama_forward_kv8(sd32, cfg, sd32["model.embed_tokens.weight"][ids])
    n16, past16 = llama_forward_kv8(sd16, cfg, sd16["model.embed_tokens.weight"][ids])
    noise = rel_l2(n16.float()[[-1, 10]], ref[[-1, 10]])
    got = engines[1].forward([Seq(pr, kv_slot=0)], [(0, -1), (0, 10)])[0]
    err = rel_l2(got.astype(np.float32), ref[[-1, 10]])
    # three one-token steps on top (the cached path): engine rows against the oracle continued with `past`
    toks, rows, refs, n16s = [7, 8, 9], [], [], []
    for t, tok in enumerate(toks):
        rows.append(engines[1].forward([Seq([tok], kv_slot=0, past_len=len(pr) + t)], [(0, 0)])[0][0])
        r, past = llama_forward_kv8(sd32, cfg, sd32["model.embed_tokens.weight"][torch.tensor([tok])], past)
        r16, past16 = llama_forward_kv8(sd16, cfg, sd16["model.embed_tokens.weight"][torch.tensor([tok])], past16)
        refs.append(r[0])
        n16s.append(r16[0].float())
    noise_d = rel_l2(torch.stack(n16s), torch.stack(refs))
    err_d = rel_l2(np.stack(rows).astype(np.float32), torch.stack(refs))
    plain = rel_l2(O.llama_forward(sd32, cfg, sd32["model.embed_tokens.weight"][ids])[0][[-1, 10]], ref[[-1, 10]])
    print(f"kv8 engine vs fp32 kv8 oracle: prefill {err:.2e} (noise {noise:.2e}), decode {err_d:.2e} (noise {noise_d:.2e}); "
          f"plain oracle vs kv8 oracle {plain:.2e}")
    assert err <= max(5e-3, 3 * noise), (err, noise)
    assert err_d <= max(5e-3, 3 * noise_d), (err_d, noise_d)


# ------------------------------------------------ 6. - 8. ------------------------------------------------
def test_kv_cache_bytes(engines):
    c = _cfg(0)
    n = 2 * c.llm_layers * c.max_slots * c.llm_heads * c.max_ctx
    assert engines[0].kv_cache_bytes() == n * 128 * 2 == engines[2].kv_cache_bytes()
    assert engines[1].kv_cache_bytes() == n * 132


def test_errors(engines, lib):
    with pytest.raises(_lib.VstarError, match="kv_cache_format"):
        VqaEngine(_cfg(3), 0)
    with pytest.raises(_lib.VstarError, match="kv_cache_format"):
        VqaEngine(_cfg(-1), 0)
    x = torch.zeros(4, 128, dtype=torch.float16, device="cuda")
    c = torch.zeros(4, 128, dtype=torch.uint8, device="cuda")
    s = torch.zeros(4, 4, dtype=torch.uint8, device="cuda")
    for args in ((P(x), 0, P(c), P(s), None), (P(x), -3, P(c), P(s), None), (None, 4, P(c), P(s), None), (P(x), 4, None, P(s), None),
                 (P(x), 4, P(c), None, None)):
        assert lib.vstar_vqa_op_kv_quantize(*args) != 0
        assert b"vstar_vqa_op_kv_quantize" in lib.vstar_vqa_last_error(None)
    eng = engines[1]
    cfg = eng.cfg
    for name in (f"kv:{cfg.llm_layers}:0", f"kv:0:{cfg.max_slots}", "kv:-1:0", "kv:0", "kv:0:0:0", "kv:a:b", "kvx"):
        with pytest.raises(_lib.VstarError):
            eng.debug_read(name, 16)
    assert eng.debug_read("kv:0:0", 16).shape == (16,)


def test_format_0_is_untouched_by_fp8_kv_engines_in_the_process(engines):
    """An fp16-cache engine built AFTER engines of the new formats existed (and ran) gives the logits of one built before them."""
    _prefill_and_steps(engines[1], _prompts(3, 30, 1), 2)
    _prefill_and_steps(engines[2], _prompts(3, 30, 1), 2)
    after = _build(0, engines["sd"])
    assert after.kv_cache_format() == 0
    assert _same(_prefill_and_steps(after, _prompts(3, 30, 1), 2), engines["base"])
    assert _same(_prefill_and_steps(engines["off_before"], _prompts(3, 30, 1), 2), engines["base"])
