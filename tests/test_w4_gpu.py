"""int4 group-scaled weight-only decode (W4A16, groups of 128) on the GPU: the quantiser against the numpy oracle
bit for bit, the W4 form of the weight-streaming kernels against the fp16 kernels on the oracle's dequantised weights (bit-identical
for ARBITRARY scales: the group scale is one fp16 multiply per weight in registers), general weights against the float64 oracle,
and the engine mode end to end — bit-identical to an fp16 engine loaded with the dequantised weights."""
import ctypes

import numpy as np
import pytest
import torch

from tests._w4_oracle import dequant_fp16, gemv_w4, pack_words, quantize_groups, unpack_words
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731
U = 2.0 ** -24


def _words_to_dev(words):
    return torch.from_numpy(words.view(np.int32)).cuda()


def _words_from_dev(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------ 1. quantiser ------------------------------------------------
@pytest.mark.parametrize("rows,K", [(16, 128), (48, 256), (256, 1152)])
def test_quantiser_matches_oracle_bit_for_bit(cuda, lib, rows, K):
    g = np.random.default_rng(rows + K)
    G = K // 128
    W = (g.standard_normal((rows, K)) * np.exp(g.uniform(-9, 6, (rows, G)).repeat(128, axis=1))).astype(np.float16)
    W[1] = 0                                                             # zero groups
    W[2] = (g.integers(-1023, 1024, K) * U).astype(np.float16)           # subnormal groups
    W[3] = 0
    W[3, :3] = [1 * U, -1 * U, 0]                                        # a / 7 rounds to zero: s = 1
    W[4] = 0
    W[4, :4] = [3 * U, 2 * U, -3 * U, U]                                 # ... again
    W[5, K // 2] = 65504                                                 # s = 9352, What finite
    W[6, 5] = -65504
    W[7] = np.round(g.uniform(-7, 7, K) * 2) / 2                         # s = 1: quotients x.5 round half to even
    W[7, ::128] = 7
    W[8] = 0
    W[8, :4] = [10 * U, -10 * U, 3 * U, 7 * U]                           # s rounds down to 2^-24: |W| / s = 10 clamps to 7
    W[9] = 0
    W[9, :3] = [7 * U, -3 * U, 4 * U]                                    # s = 2^-24
    qo, so = quantize_groups(W)
    assert so[5, G // 2] == 9352 and so[3, 0] == 1 and float(so[8, 0]) == U and qo[8, 0] == 7 and qo.min() >= -7
    wo = pack_words(qo)
    Wo = dequant_fp16(qo, so)
    assert np.isfinite(Wo.astype(np.float32)).all()
    Wd = torch.from_numpy(W).cuda()
    q = torch.zeros((rows, K // 8), dtype=torch.int32, device="cuda")
    s = torch.full((rows, G), float("nan"), dtype=torch.float16, device="cuda")
    What = torch.full((rows, K), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_quantize_w4(P(Wd), rows, K, P(q), P(s), P(What)) == 0, lib.vstar_vqa_last_error(None)
    assert np.array_equal(s.cpu().numpy().view(np.int16), so.view(np.int16))
    assert np.array_equal(_words_from_dev(q), wo)
    assert np.array_equal(What.cpu().numpy().view(np.int16), Wo.view(np.int16))
    # without What, and in place (What aliases W: how the engine overwrites its masters)
    q2, s2 = torch.zeros_like(q), torch.zeros_like(s)
    assert lib.vstar_vqa_op_quantize_w4(P(Wd), rows, K, P(q2), P(s2), None) == 0
    assert torch.equal(q2, q) and torch.equal(s2.view(torch.int16), s.view(torch.int16))
    q3 = torch.zeros_like(q)
    assert lib.vstar_vqa_op_quantize_w4(P(Wd), rows, K, P(q3), P(s2), P(Wd)) == 0
    assert torch.equal(q3, q) and np.array_equal(Wd.cpu().numpy().view(np.int16), Wo.view(np.int16))


# ------------------------------------------------ 2. bit-identity with the fp16 kernels ------------------------------------------------
def _general_case(M, N, K, epi, norm, use_res, seed):
    """q uniform over ALL of -8..7 (u = 0 included), general fp16 scales (random mantissas, 2^-4 .. 2^-10), a few subnormal scales, one
    group with s = 9352 (q in -7..7 there: -8 * 9352 is not finite) and one group of q = 0; padding rows q = 0, s = 1.  The fp16
    kernels get the oracle's dequantised weights.  The activations of group 1 — where the 9352 group sits — are scaled by 2^-10 so
    that the outputs stay finite in fp16."""
    g = np.random.default_rng(seed)
    t = torch.Generator().manual_seed(seed)
    Npad = (N + 255) // 256 * 256
    G = K // 128
    n_out = N // 2 if epi == 4 else N
    A = torch.randn(M, K, generator=t) * 1.5
    A[:, 128:256] *= 2.0 ** -10
    A = A.half()
    q = np.zeros((Npad, K), np.int8)
    q[:N] = g.integers(-8, 8, (N, K))
    s = np.ones((Npad, G), np.float16)
    s[:N] = (g.uniform(1, 2, (N, G)) * 2.0 ** -g.integers(4, 11, (N, G))).astype(np.float16)
    s[5:N:37, 0] = (g.integers(1, 1024, len(range(5, N, 37))) * U).astype(np.float16)       # subnormal scales
    s[3, 1] = 9352
    q[3, 128:256] = np.clip(q[3, 128:256], -7, 7)
    q[7, :128] = 0
    W = dequant_fp16(q, s)
    assert np.isfinite(W.astype(np.float32)).all() and set(np.unique(q[:N])) == set(range(-8, 8))
    gain = (1 + 0.1 * torch.randn(K, generator=t)).half().cuda() if norm else None
    bias = (torch.randn(Npad, generator=t) * 0.1).half().cuda() if epi != 4 and not norm else None
    res = (torch.randn(M, n_out, generator=t) * 0.5).half().cuda() if use_res else None
    return A.cuda(), _words_to_dev(pack_words(q)), torch.from_numpy(s).cuda(), torch.from_numpy(W).cuda(), gain, bias, res, n_out


def _run_pair(lib, M, N, K, epi, kernel, layouts, case):
    A, q, s, W, gain, bias, res, n_out = case
    C = torch.full((M, n_out), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_gemm(P(A), P(W), P(bias), P(res), P(C), M, N, K, epi, kernel, P(gain), 1e-5) == 0, lib.vstar_vqa_last_error(None)
    assert torch.isfinite(C.float()).all()
    for layout in layouts:
        C4 = torch.full((M, n_out), float("nan"), dtype=torch.float16, device="cuda")
        rc = lib.vstar_vqa_op_gemm_w4(P(A), P(q), P(s), P(bias), P(res), P(C4), M, N, K, epi, kernel, P(gain), 1e-5, layout)
        assert rc == 0, lib.vstar_vqa_last_error(None)
        assert not torch.isnan(C4.float()).any(), (kernel, layout)
        assert torch.equal(C4.view(torch.int16), C.view(torch.int16)), (kernel, layout, float((C4.float() - C.float()).abs().max()))


@pytest.mark.parametrize("M,N,K,epi,norm,use_res", [
    (1, 256, 512, 0, False, True),         # one double step per wave
    (2, 256, 640, 0, False, False),        # waves 0 - 1 have two steps, the rest one
    (4, 1000, 1152, 0, True, True),        # ragged waves, N tail
    (7, 512, 1536, 4, False, False),       # NT = 2
    (3, 256, 6144, 0, True, False),        # steady state
    (1, 512, 11008, 0, False, True),       # 21.5 steps per wave
    (8, 512, 1024, 0, False, False),
    (1, 256, 384, 0, False, False),        # below the ring's K
])
def test_w4_kernels_are_bit_identical_to_fp16_on_dequantised_weights(cuda, lib, M, N, K, epi, norm, use_res):
    case = _general_case(M, N, K, epi, norm, use_res, M * 7 + N + K)
    lay = (0, 1) if N % 16 == 0 else (0,)                                       # 1: the tile-major image
    _run_pair(lib, M, N, K, epi, 1, lay, case)                                  # dispatch against dispatch (the fp16 side: the ring)
    _run_pair(lib, M, N, K, epi, 3, lay, case)                                  # register kernel against register kernel


@pytest.mark.parametrize("epi", [0, 2, 4])
@pytest.mark.parametrize("N,K", [(320, 256), (768, 1024)])
@pytest.mark.parametrize("M", [9, 16, 33, 64])
def test_w4_register_kernel_row_tiles_are_bit_identical_to_fp16(cuda, lib, M, N, K, epi):
    case = _general_case(M, N, K, epi, False, M % 2 == 1, M * 11 + N + K + epi)
    _run_pair(lib, M, N, K, epi, 1, (0, 1), case)
    _run_pair(lib, M, N, K, epi, 3, (0, 1), case)


# ------------------------------------------------ 3. general weights against the oracle ------------------------------------------------
@pytest.mark.parametrize("M,N,K,epi", [(1, 4096, 4096, 0), (5, 1024, 1024, 4), (48, 320, 256, 0)])
def test_w4_gemv_general_weights_against_oracle(cuda, lib, M, N, K, epi):
    """test_w8_gemv_general_scales_against_oracle's bound, the fp16 kernels' own (fp32 accumulate, fp16 store): 2e-3 * max|ref| + 1e-3."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    Npad = (N + 255) // 256 * 256
    n_out = N // 2 if epi == 4 else N
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = torch.zeros(Npad, K, dtype=torch.float16)
    W[:N] = (torch.randn(N, K, generator=g) / K ** 0.5 * torch.exp(torch.randn(N, 1, generator=g))).half()
    bias = (torch.randn(Npad, generator=g) * 0.1).half() if epi != 4 else None
    res = (torch.randn(M, n_out, generator=g) * 0.5).half() if M % 2 else None
    Wd, Ad = W.cuda(), A.cuda()
    q = torch.zeros(Npad, K // 8, dtype=torch.int32, device="cuda")
    s = torch.zeros(Npad, K // 128, dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_quantize_w4(P(Wd), Npad, K, P(q), P(s), None) == 0, lib.vstar_vqa_last_error(None)
    qh, sh = unpack_words(_words_from_dev(q)), s.cpu().numpy()
    assert (qh[N:] == 0).all() and (sh[N:] == 1).all()                   # padding rows: u = 8, s = 1
    ref = gemv_w4(A.numpy(), qh[:N], sh[:N], None if bias is None else bias.numpy()[:N], None if res is None else res.numpy(), epi)
    scale = float(np.abs(ref).max())
    bd, rd = (None if bias is None else bias.cuda()), (None if res is None else res.cuda())
    for kernel, layout in ((1, 0), (1, 1), (3, 0)):
        C = torch.full((M, n_out), float("nan"), dtype=torch.float16, device="cuda")
        rc = lib.vstar_vqa_op_gemm_w4(P(Ad), P(q), P(s), P(bd), P(rd), P(C), M, N, K, epi, kernel, None, 0.0, layout)
        assert rc == 0, lib.vstar_vqa_last_error(None)
        err = float(np.abs(C.float().cpu().numpy().astype(np.float64) - ref).max())
        print(f"w4 gemv M={M} N={N} K={K} epi={epi} kernel={kernel} layout={layout}: max err {err:.3e}, bound {2e-3 * scale + 1e-3:.3e}")
        assert err <= 2e-3 * scale + 1e-3, err


# ------------------------------------------------ 4. the engine mode ------------------------------------------------
LIN_KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _cfg(bits):
    # hidden 512: the fp16 side runs its ring kernel and tile-major images; 12 slots for the 12-sequence step
    return VQAConfig.tiny(llm_hidden=512, llm_heads=4, llm_mlp=1024, max_slots=12).with_decode_bits(bits)


def _build(bits, sd):
    eng = VqaEngine(_cfg(bits), 0)
    eng.load_state_dict(sd)
    return eng


def _prompts(n, length, seed):
    g = torch.Generator().manual_seed(seed)
    return [[1] + torch.randint(3, 300, (length - 1 + i,), generator=g).tolist() for i in range(n)]


def _prefill_and_steps(eng, prompts, steps, seed=5):
    """Ragged text-only prefill of len(prompts) sequences (> 64 rows: the tile-kernel path), then `steps` teacher-forced one-token
    steps of all of them.  Returns [prefill logits, step logits ...] (fp16 arrays)."""
    n = len(prompts)
    assert sum(len(p) for p in prompts) > 64
    out = [eng.forward([Seq(p, kv_slot=i) for i, p in enumerate(prompts)], [(i, -1) for i in range(n)])[0]]
    g = torch.Generator().manual_seed(seed)
    for t in range(steps):
        toks = torch.randint(3, 300, (n,), generator=g).tolist()
        out.append(eng.forward([Seq([toks[i]], kv_slot=i, past_len=len(prompts[i]) + t) for i in range(n)], [(i, 0) for i in range(n)])[0])
    return out


@pytest.fixture(scope="module")
def engines(cuda):
    sd = random_state_dict(_cfg(0), seed=3, dtype=torch.float16)
    off_before = _build(0, sd)                       # mode off and the 8-bit mode, built before any 4-bit engine of this module
    w8_before = _build(8, sd)
    base = {0: _prefill_and_steps(off_before, _prompts(3, 30, 1), 2), 8: _prefill_and_steps(w8_before, _prompts(3, 30, 1), 2)}
    sd_hat = dict(sd)                                # the oracle's dequantised weights for engine B
    for k, v in sd.items():
        if k.startswith("model.layers.") and k.endswith(".weight") and any(x in k for x in LIN_KEYS):
            q, s = quantize_groups(v.numpy())
            sd_hat[k] = torch.from_numpy(dequant_fp16(q, s))
    a = _build(4, sd)
    b = _build(0, sd_hat)
    return {"sd": sd, "off_before": off_before, "w8_before": w8_before, "base": base, "a": a, "b": b}


def test_engine_prefill_is_bit_identical_to_dequantised_fp16_engine(engines):
    a, b = engines["a"], engines["b"]
    assert a.decode_weight_bits() == 4 and b.decode_weight_bits() == 0 and engines["w8_before"].decode_weight_bits() == 8
    pr = _prompts(1, 96, 2)
    la = a.forward([Seq(pr[0], kv_slot=0)], [(0, -1), (0, 10)])[0]
    lb = b.forward([Seq(pr[0], kv_slot=0)], [(0, -1), (0, 10)])[0]
    assert np.isfinite(la.astype(np.float32)).all()
    assert np.array_equal(la.view(np.int16), lb.view(np.int16))
    # ... and the quantised model is not the unquantised one
    l0 = engines["off_before"].forward([Seq(pr[0], kv_slot=0)], [(0, -1), (0, 10)])[0]
    assert not np.array_equal(la.view(np.int16), l0.view(np.int16))


@pytest.mark.parametrize("nseq,steps", [(1, 4), (3, 4), (12, 1)])
def test_engine_decode_is_bit_identical_to_dequantised_fp16_engine(engines, nseq, steps):
    """Same model, same MFMA operands in the same order: the decode steps agree bit for bit, not within a band.  On the fp16 side 1
    and 3 sequences run the ring kernel (tile-major images), 12 the register kernel."""
    pr = _prompts(nseq, 96 if nseq == 1 else (30 if nseq == 3 else 8), 10 + nseq)
    la = _prefill_and_steps(engines["a"], pr, steps)
    lb = _prefill_and_steps(engines["b"], pr, steps)
    for t in range(steps + 1):
        assert np.array_equal(la[t].view(np.int16), lb[t].view(np.int16)), (nseq, t)


def test_greedy_decode_and_tails_on_the_w4_engine(engines, lib):
    from tests.test_beam_gpu import op_select
    from tests.test_sampling_gpu import op_sample
    from tests.test_score_gpu import op_score
    from vstar_amd.vqa import VQA_LLM
    a = engines["a"]
    cfg = a.cfg
    pr = _prompts(1, 70, 21)[0]
    # greedy_decode against a hand-rolled forward + arg-max loop
    llm = VQA_LLM(cfg=cfg, engine=a, decode_weight_bits=4)
    got = llm.greedy_decode([Seq(pr, kv_slot=0)], [len(pr)], 6)[0]
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
    # a verify step of one sequence against the greedy rule: the leading drafts that equal the arg-max of the row before them are
    # accepted, one more token follows, -1 behind it
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


def test_errors(cuda, lib):
    with pytest.raises(_lib.VstarError, match="decode_weight_format"):
        VqaEngine(VQAConfig.tiny(decode_weight_format=1, decode_weight_bits=8), 0)
    M, N, K = 65, 256, 256
    A = torch.zeros(M, K, dtype=torch.float16, device="cuda")
    q = torch.zeros(N, K // 8, dtype=torch.int32, device="cuda")
    s = torch.ones(N, K // 128, dtype=torch.float16, device="cuda")
    C = torch.zeros(M, N, dtype=torch.float16, device="cuda")
    for args in ((P(A), P(q), P(s), None, None, P(C), 65, N, K, 0, 1, None, 0.0, 0),          # M = 65
                 (P(A), P(q), P(s), None, None, P(C), 4, N, K, 0, 2, None, 0.0, 0),           # the tile kernels have no W4 form
                 (P(A), P(q), P(s), None, None, P(C), 4, N, 192, 0, 1, None, 0.0, 0),         # K % 128 != 0
                 (P(A), P(q), None, None, None, P(C), 4, N, K, 0, 1, None, 0.0, 0)):          # null scales
        assert lib.vstar_vqa_op_gemm_w4(*args) != 0
        assert b"vstar_vqa_op_gemm_w4" in lib.vstar_vqa_last_error(None)
    assert lib.vstar_vqa_op_quantize_w4(P(A), 4, 192, P(q), P(s), None) != 0
    assert b"vstar_vqa_op_quantize_w4" in lib.vstar_vqa_last_error(None)


def test_other_modes_are_untouched_by_a_4bit_engine_in_the_process(engines):
    """An fp16 engine and an 8-bit engine built AFTER a 4-bit engine existed (and ran) give the logits of ones built before it: no
    launch attribute, environment cache or buffer is shared between the variants."""
    _prefill_and_steps(engines["a"], _prompts(3, 30, 1), 2)
    for bits, before in ((0, engines["off_before"]), (8, engines["w8_before"])):
        after = _build(bits, engines["sd"])
        assert after.decode_weight_bits() == bits
        got = _prefill_and_steps(after, _prompts(3, 30, 1), 2)
        for x, y in zip(got, engines["base"][bits]):
            assert np.array_equal(x.view(np.int16), y.view(np.int16))
        again = _prefill_and_steps(before, _prompts(3, 30, 1), 2)
        for x, y in zip(again, engines["base"][bits]):
            assert np.array_equal(x.view(np.int16), y.view(np.int16))
