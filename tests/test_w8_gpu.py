"""int8 weight-only decode (W8A16) on the GPU: the quantiser against the numpy oracle bit for bit, the W8 forms of
the weight-streaming kernels against the fp16 kernels they are derived from (bit-identical when the scales are powers of two),
general scales against the float64 oracle, and the engine mode end to end."""
import ctypes

import numpy as np
import pytest
import torch

from tests._w8_oracle import dequant_fp16, gemv_w8, quantize_rows
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu

P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None       # noqa: E731


def rel_l2(got, ref):
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


# ------------------------------------------------ 1. quantiser ------------------------------------------------
@pytest.mark.parametrize("rows,K", [(16, 64), (48, 256), (256, 1088)])
def test_quantiser_matches_oracle_bit_for_bit(cuda, lib, rows, K):
    g = np.random.default_rng(rows + K)
    W = (g.standard_normal((rows, K)) * np.exp(g.uniform(-5, 3, (rows, 1)))).astype(np.float16)
    W[1] = 0                                                             # a zero row
    W[2] = (g.integers(-1023, 1024, K) * 2.0 ** -24).astype(np.float16)     # a row of subnormals
    W[3, K // 2] = 65504
    W[4, 5] = -65504
    W[5] = np.round(g.uniform(-127, 127, K) * 2) / 2                     # s = 1: ties
    W[5, 0] = 127
    W[6] = 0
    W[6, :8] = [65504, -65504, 257.9, 0, 1, -1, 32752, 515.5]            # test_w8_oracle's row: 32752 / s rounds to 63.5 in fp32 -> 64
    qo, so = quantize_rows(W)
    assert qo[6, 6] == 64
    Wo = dequant_fp16(qo, so)
    Wd = torch.from_numpy(W).cuda()
    q = torch.full((rows, K), -128, dtype=torch.int8, device="cuda")
    s = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
    What = torch.full((rows, K), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_quantize_w8(P(Wd), rows, K, P(q), P(s), P(What)) == 0, lib.vstar_vqa_last_error(None)
    assert np.array_equal(s.cpu().numpy().view(np.int32), so.view(np.int32))
    assert np.array_equal(q.cpu().numpy(), qo)
    assert np.array_equal(What.cpu().numpy().view(np.int16), Wo.view(np.int16))
    # in place (What aliases W: how the engine overwrites its masters), and without What
    q2 = torch.empty_like(q)
    assert lib.vstar_vqa_op_quantize_w8(P(Wd), rows, K, P(q2), P(s), P(Wd)) == 0
    assert torch.equal(q2, q) and np.array_equal(Wd.cpu().numpy().view(np.int16), Wo.view(np.int16))


# ------------------------------------------------ 2. bit-identity with the fp16 kernels ------------------------------------------------
def _pow2_case(M, N, K, epi, norm, use_res, seed):
    """q uniform in [-127, 127], per-row scales 2^-e, e in 4..10: every q * 2^-e is a normal fp16 and the fp32 scaling is exact."""
    g = torch.Generator().manual_seed(seed)
    Npad = (N + 255) // 256 * 256
    n_out = N // 2 if epi == 4 else N
    A = (torch.randn(M, K, generator=g) * 1.5).half().cuda()
    q = torch.zeros(Npad, K, dtype=torch.int8)
    q[:N] = torch.randint(-127, 128, (N, K), generator=g, dtype=torch.int8)
    s = torch.ones(Npad)
    s[:N] = 2.0 ** -torch.randint(4, 11, (N,), generator=g).float()
    W = (q.float() * s[:, None]).half()
    assert torch.equal(W.float(), q.float() * s[:, None])
    gain = (1 + 0.1 * torch.randn(K, generator=g)).half().cuda() if norm else None
    bias = (torch.randn(Npad, generator=g) * 0.1).half().cuda() if epi != 4 and not norm else None
    res = (torch.randn(M, n_out, generator=g) * 0.5).half().cuda() if use_res else None
    return A, q.cuda(), s.cuda(), W.cuda(), gain, bias, res, n_out


def _run_pair(lib, M, N, K, epi, kernel, layouts, case):
    A, q, s, W, gain, bias, res, n_out = case
    C = torch.full((M, n_out), float("nan"), dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_gemm(P(A), P(W), P(bias), P(res), P(C), M, N, K, epi, kernel, P(gain), 1e-5) == 0, lib.vstar_vqa_last_error(None)
    assert not torch.isnan(C.float()).any()
    for layout in layouts:
        C8 = torch.full((M, n_out), float("nan"), dtype=torch.float16, device="cuda")
        rc = lib.vstar_vqa_op_gemm_w8(P(A), P(q), P(s), P(bias), P(res), P(C8), M, N, K, epi, kernel, P(gain), 1e-5, layout)
        assert rc == 0, lib.vstar_vqa_last_error(None)
        assert not torch.isnan(C8.float()).any(), (kernel, layout)
        assert torch.equal(C8.view(torch.int16), C.view(torch.int16)), (kernel, layout, float((C8.float() - C.float()).abs().max()))


@pytest.mark.parametrize("M,N,K,epi,norm,use_res", [
    (1, 256, 512, 0, False, True),         # one double step per wave
    (4, 1000, 1088, 0, True, True),        # 17 steps: ragged across waves, N tail (row-major only: tiling needs N % 16 == 0)
    (7, 512, 1536, 4, False, False),       # NT = 2
    (3, 256, 6144, 0, True, False),        # several steady rounds
    (1, 512, 11008, 0, False, True),       # 21.5 steps per wave
    (8, 512, 1024, 0, False, False),       # M = 8 without norm
])
def test_w8_ring_and_register_kernels_are_bit_identical_to_fp16(cuda, lib, M, N, K, epi, norm, use_res):
    case = _pow2_case(M, N, K, epi, norm, use_res, M * 7 + N + K)
    _run_pair(lib, M, N, K, epi, 1, (0, 1) if N % 16 == 0 else (0,), case)      # ring against ring
    _run_pair(lib, M, N, K, epi, 3, (0,), case)                                  # register kernel against register kernel


@pytest.mark.parametrize("epi", [0, 2, 4])
@pytest.mark.parametrize("N,K", [(320, 256), (768, 1024)])
@pytest.mark.parametrize("M", [9, 16, 33, 64])
def test_w8_register_kernel_row_tiles_are_bit_identical_to_fp16(cuda, lib, M, N, K, epi):
    case = _pow2_case(M, N, K, epi, False, M % 2 == 1, M * 11 + N + K + epi)
    _run_pair(lib, M, N, K, epi, 1, (0,), case)
    _run_pair(lib, M, N, K, epi, 3, (0,), case)


@pytest.mark.parametrize("M,kernel", [(2, 1), (2, 3), (12, 1)])
def test_w8_scale_is_a_multiply_of_its_own_before_the_bias_add(cuda, lib, M, kernel):
    """Contract item 2: fp32(acc * s), then the epilogue's fp32 bias add — two roundings, not one fma.  Integer activations in
    [-4, 4] make the fp32 accumulator exact in any order (|acc| <= 4 * 127 * 512 < 2^24), the scales are not powers of two, and
    bias = -fp16(acc[0] * s) cancels the product of row 0 down to its own rounding error, where a fused multiply-add (which adds the
    bias to the UNROUNDED product) gives other fp16 bits.  Bit-exact against the float32 restatement; the case is checked to tell
    the two forms apart."""
    N, K = 256, 512
    g = np.random.default_rng(100 * M + kernel)
    A = g.integers(-4, 5, (M, K)).astype(np.float16)
    q = g.integers(-127, 128, (N, K)).astype(np.int8)
    s = g.uniform(1e-3, 1e-2, N).astype(np.float32)
    acc = A.astype(np.int64) @ q.astype(np.int64).T                                # exact
    prod = acc.astype(np.float32) * s[None, :]                                     # fp32, one rounding
    bias = (-prod[0]).astype(np.float16)
    b32 = bias.astype(np.float32)[None, :]
    want = (prod + b32).astype(np.float16)                                         # fp32 add, then the fp16 store
    fused = (acc.astype(np.float64) * s.astype(np.float64)[None, :] + b32.astype(np.float64)).astype(np.float32).astype(np.float16)
    assert (want[0].view(np.int16) != fused[0].view(np.int16)).sum() >= 8          # the case can see a fused multiply-add
    C = torch.full((M, N), float("nan"), dtype=torch.float16, device="cuda")
    Ad, qd, sd, bd = (torch.from_numpy(x).cuda() for x in (A, q, s, bias))
    rc = lib.vstar_vqa_op_gemm_w8(P(Ad), P(qd), P(sd), P(bd), None, P(C), M, N, K, 0, kernel, None, 0.0, 0)
    assert rc == 0, lib.vstar_vqa_last_error(None)
    assert np.array_equal(C.cpu().numpy().view(np.int16), want.view(np.int16))


# ------------------------------------------------ 3. general scales against the oracle ------------------------------------------------
@pytest.mark.parametrize("M,N,K,epi", [(1, 4096, 4096, 0), (5, 1024, 1024, 4), (48, 320, 256, 0)])
def test_w8_gemv_general_scales_against_oracle(cuda, lib, M, N, K, epi):
    """test_weight_streaming_gemm's bound (fp32 accumulate, fp16 store): 2e-3 * max|ref| + 1e-3."""
    g = torch.Generator().manual_seed(M * 1000 + N)
    Npad = (N + 255) // 256 * 256
    n_out = N // 2 if epi == 4 else N
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = torch.zeros(Npad, K, dtype=torch.float16)
    W[:N] = (torch.randn(N, K, generator=g) / K ** 0.5 * torch.exp(torch.randn(N, 1, generator=g))).half()
    bias = (torch.randn(Npad, generator=g) * 0.1).half() if epi != 4 else None
    res = (torch.randn(M, n_out, generator=g) * 0.5).half() if M % 2 else None
    Wd, Ad = W.cuda(), A.cuda()
    q = torch.empty(Npad, K, dtype=torch.int8, device="cuda")
    s = torch.empty(Npad, dtype=torch.float32, device="cuda")
    assert lib.vstar_vqa_op_quantize_w8(P(Wd), Npad, K, P(q), P(s), None) == 0, lib.vstar_vqa_last_error(None)
    ref = gemv_w8(A.numpy(), q.cpu().numpy()[:N], s.cpu().numpy()[:N], None if bias is None else bias.numpy()[:N],
                  None if res is None else res.numpy(), epi)
    scale = float(np.abs(ref).max())
    bd, rd = (None if bias is None else bias.cuda()), (None if res is None else res.cuda())
    for kernel, layout in ((1, 0), (1, 1), (3, 0)):
        C = torch.full((M, n_out), float("nan"), dtype=torch.float16, device="cuda")
        rc = lib.vstar_vqa_op_gemm_w8(P(Ad), P(q), P(s), P(bd), P(rd), P(C), M, N, K, epi, kernel, None, 0.0, layout)
        assert rc == 0, lib.vstar_vqa_last_error(None)
        err = float(np.abs(C.float().cpu().numpy().astype(np.float64) - ref).max())
        print(f"w8 gemv M={M} N={N} K={K} epi={epi} kernel={kernel} layout={layout}: max err {err:.3e}, bound {2e-3 * scale + 1e-3:.3e}")
        assert err <= 2e-3 * scale + 1e-3, err


# ------------------------------------------------ 4-8. the engine mode ------------------------------------------------
LIN_KEYS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _cfg(bits):
    # hidden 512: the ring kernel and the tile-major images are live; 12 slots for the 12-sequence step
    return VQAConfig.tiny(llm_hidden=512, llm_heads=4, llm_mlp=1024, max_slots=12, decode_weight_bits=bits)


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
    off_before = _build(0, sd)                       # mode off, built before any 8-bit engine of this module
    base = _prefill_and_steps(off_before, _prompts(3, 30, 1), 2)
    sd_hat = dict(sd)                                # the oracle's dequantised weights for engine B
    for k, v in sd.items():
        if k.startswith("model.layers.") and k.endswith(".weight") and any(x in k for x in LIN_KEYS):
            q, s = quantize_rows(v.numpy())
            sd_hat[k] = torch.from_numpy(dequant_fp16(q, s))
    a = _build(8, sd)
    b = _build(0, sd_hat)
    return {"sd": sd, "off_before": off_before, "base": base, "a": a, "b": b}


def test_engine_prefill_is_bit_identical_to_dequantised_fp16_engine(engines):
    a, b = engines["a"], engines["b"]
    assert a.decode_weight_bits() == 8 and b.decode_weight_bits() == 0
    pr = _prompts(1, 96, 2)
    la = a.forward([Seq(pr[0], kv_slot=0)], [(0, -1), (0, 10)])[0]
    lb = b.forward([Seq(pr[0], kv_slot=0)], [(0, -1), (0, 10)])[0]
    assert np.isfinite(la.astype(np.float32)).all()
    assert np.array_equal(la.view(np.int16), lb.view(np.int16))
    # ... and the quantised model is not the unquantised one
    l0 = engines["off_before"].forward([Seq(pr[0], kv_slot=0)], [(0, -1), (0, 10)])[0]
    assert not np.array_equal(la.view(np.int16), l0.view(np.int16))


@pytest.mark.parametrize("nseq,steps", [(1, 4), (3, 4), (12, 1)])
def test_engine_decode_matches_dequantised_fp16_engine(engines, nseq, steps):
    """Same model, different GEMM path (int8 stream + fp32 scale against fp16(q * s) weights): test_batched_ragged_decode_equals_single's
    bound.  1 and 3 sequences run the ring kernel, 12 the register kernel."""
    pr = _prompts(nseq, 96 if nseq == 1 else (30 if nseq == 3 else 8), 10 + nseq)
    la = _prefill_and_steps(engines["a"], pr, steps)
    lb = _prefill_and_steps(engines["b"], pr, steps)
    assert np.array_equal(la[0].view(np.int16), lb[0].view(np.int16))       # the prefill (tile kernels) again
    for t in range(1, steps + 1):
        r = rel_l2(la[t], lb[t])
        print(f"w8 decode nseq={nseq} step={t}: rel_l2 vs the dequantised fp16 engine = {r:.3e}")
        assert r < 2e-3, r


def test_greedy_decode_and_tails_on_the_w8_engine(engines, lib):
    from tests.test_beam_gpu import op_select
    from tests.test_sampling_gpu import op_sample
    from tests.test_score_gpu import op_score
    from vstar_amd.vqa import VQA_LLM
    a = engines["a"]
    cfg = a.cfg
    pr = _prompts(1, 70, 21)[0]
    # greedy_decode against a hand-rolled forward + arg-max loop
    llm = VQA_LLM(cfg=cfg, engine=a)
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


def test_errors(cuda, lib):
    with pytest.raises(_lib.VstarError, match="decode_weight_bits"):
        VqaEngine(VQAConfig.tiny(decode_weight_bits=4), 0)
    M, N, K = 65, 256, 256
    A = torch.zeros(M, K, dtype=torch.float16, device="cuda")
    q = torch.zeros(N, K, dtype=torch.int8, device="cuda")
    s = torch.ones(N, dtype=torch.float32, device="cuda")
    C = torch.zeros(M, N, dtype=torch.float16, device="cuda")
    assert lib.vstar_vqa_op_gemm_w8(P(A), P(q), P(s), None, None, P(C), M, N, K, 0, 1, None, 0.0, 0) != 0
    assert b"gemm_w8" in lib.vstar_vqa_last_error(None)
    assert lib.vstar_vqa_op_gemm_w8(P(A), P(q), P(s), None, None, P(C), 4, N, K, 0, 2, None, 0.0, 0) != 0      # the tile kernels have no W8 form


def test_mode_off_is_untouched_by_an_8bit_engine_in_the_process(engines):
    """An fp16 engine built AFTER an 8-bit engine existed (and ran) gives the logits of one built before it: no launch attribute,
    environment cache or buffer is shared between the variants."""
    _prefill_and_steps(engines["a"], _prompts(3, 30, 1), 2)
    after = _build(0, engines["sd"])
    assert after.decode_weight_bits() == 0
    got = _prefill_and_steps(after, _prompts(3, 30, 1), 2)
    for x, y in zip(got, engines["base"]):
        assert np.array_equal(x.view(np.int16), y.view(np.int16))
    again = _prefill_and_steps(engines["off_before"], _prompts(3, 30, 1), 2)
    for x, y in zip(again, engines["base"]):
        assert np.array_equal(x.view(np.int16), y.view(np.int16))
