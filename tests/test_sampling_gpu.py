"""Sampled decoding on the MI355X (csrc/sample.hip): the op against the CPU oracle (tests/_sampling_oracle.py) at
real vocabulary sizes, the draw distribution, determinism and row independence, and the VQA-LLM decode built on it."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sampling_oracle as S
from vstar_amd import _lib
from vstar_amd.vqa import sampling_params

pytestmark = pytest.mark.gpu
U_EPS = 1e-5            # a draw whose u*Z lies this close (relative to Z) to a prefix-mass boundary may differ from the oracle


def op_sample(lib, x_dev: torch.Tensor, params, vocab=None):
    """vstar_vqa_op_sample on device rows x_dev [rows, ld] (fp16 / bf16), the first `vocab` (default ld) of each: (tokens, u,
    n_kept)."""
    rows, ld = x_dev.shape
    assert x_dev.is_cuda and x_dev.dtype in (torch.float16, torch.bfloat16) and len(params) == rows <= 256
    prm = (_lib.VqaSampling * rows)(*params)
    tok, u, nk = (np.empty(rows, np.int32), np.empty(rows, np.float32), np.empty(rows, np.int32))
    dt = _lib.F16 if x_dev.dtype == torch.float16 else _lib.BF16
    vocab = ld if vocab is None else vocab
    _lib.check_vqa(lib.vstar_vqa_op_sample(ctypes.c_void_p(x_dev.data_ptr()), dt, rows, vocab, ld, ctypes.cast(prm, ctypes.c_void_p),
                                           ctypes.c_void_p(tok.ctypes.data), ctypes.c_void_p(u.ctypes.data),
                                           ctypes.c_void_p(nk.ctypes.data)))
    return tok, u, nk


def make_row(kind, V, g, dtype):
    x = torch.randn(V, generator=g) * 3
    if kind == "peaked":
        x = torch.randn(V, generator=g)
        x[int(torch.randint(0, V, (1,), generator=g))] += 15
    elif kind == "flat":
        x = torch.full((V,), 1.5)
    elif kind == "masked":
        m = torch.rand(V, generator=g) < 0.5
        x = torch.where(m, torch.where(torch.rand(V, generator=g) < 0.5, -float("inf"), -65504.0), x)
        if V > 1:
            x[0] = 2.0                      # at least one finite score
    return x.to(dtype)


TEMPS, TOPKS, TOPPS = (0.01, 0.7, 1.0, 5.0), ("0", "1", "50", "V", "V+7"), (1.0, 0.9, 0.5, 0.0)
KINDS = ("random", "peaked", "flat", "masked")


def test_op_against_oracle(cuda, lib):
    draws = excused = checked_kept = skipped_kept = 0
    for dtype in (torch.float16, torch.bfloat16):
        for V in (1, 2, 320, 1000, 32000, 32001, 131075):
            g = torch.Generator().manual_seed(V)
            combos = [(t, k, p) for t in TEMPS for k in TOPKS for p in TOPPS]
            rows, cases = [], []
            for ci, (t, k, p) in enumerate(combos):
                kinds = KINDS if V <= 1000 else (KINDS[ci % 4],)
                for kind in kinds:
                    kk = {"0": 0, "1": 1, "50": 50, "V": V, "V+7": V + 7}[k]
                    rows.append(make_row(kind, V, g, dtype))
                    cases.append((t, kk, p, kind, 1000 + len(cases)))
            ld = V + 13                      # a row stride that is not the vocabulary
            for c0 in range(0, len(rows), 256):
                chunk = rows[c0:c0 + 256]
                x = torch.zeros(len(chunk), ld, dtype=dtype)
                x[:, :V] = torch.stack(chunk)
                cs = cases[c0:c0 + 256]
                params = [sampling_params(t, k, p, seed=seed, step=7, stream=seed * 3) for t, k, p, _, seed in cs]
                tok, u, nk = op_sample(lib, x.to(cuda), params, vocab=V)
                for j, (t, k, p, kind, seed) in enumerate(cs):
                    uu = S.uniform(seed, 7, seed * 3)
                    assert float(u[j]) == uu, (V, j)
                    ref = S.sample_row(chunk[j], params[j].temperature, k, p, uu)
                    if ref["p_dist"] < 1e-6:
                        skipped_kept += 1
                        continue
                    assert nk[j] == ref["n_kept"], (dtype, V, t, k, p, kind, int(nk[j]), ref["n_kept"])
                    checked_kept += 1
                    draws += 1
                    if tok[j] != ref["token"]:
                        assert ref["u_dist"] < U_EPS, (dtype, V, t, k, p, kind, int(tok[j]), ref["token"], ref["u_dist"])
                        excused += 1
    print(f"op vs oracle: {draws} draws, {excused} excused at a prefix-mass boundary; n_kept compared on {checked_kept} rows, "
          f"{skipped_kept} top-p boundary rows skipped")
    assert excused <= 0.001 * draws
    assert skipped_kept <= 0.01 * (checked_kept + skipped_kept)


def test_op_tie_rule(cuda, lib):
    for dtype in (torch.float16, torch.bfloat16):
        x = torch.tensor([[1.0, 3.0, 3.0, 3.0, 2.0, 0.0]] * 2, dtype=dtype)
        y = torch.log(torch.tensor([0.1, 0.5, 0.05, 0.05, 0.15, 0.15], dtype=torch.float64)).to(dtype)
        rows = torch.cat([x, y[None]], 0).to(cuda)
        params = [sampling_params(1.0, 2, None, seed=1), sampling_params(1.0, 0, 0.0, seed=2), sampling_params(1.0, 0, 0.6, seed=3)]
        tok, u, nk = op_sample(lib, rows, params)
        assert nk.tolist() == [3, 3, 3]
        assert tok[0] in (1, 2, 3) and tok[1] in (1, 2, 3) and tok[2] in (1, 4, 5)


def test_draw_distribution_chi_square(cuda, lib):
    scipy_stats = pytest.importorskip("scipy.stats")
    g = torch.Generator().manual_seed(21)
    V = 1000
    x = (torch.randn(V, generator=g) * 2).half()
    xd = x[None].expand(256, V).contiguous().to(cuda)
    ref = S.sample_row(x, 0.8, 50, 0.9, 0.5)
    counts = np.zeros(V, np.int64)
    n = 0
    for launch in range(79):                    # 20224 draws, rows differing only in `step`
        params = [sampling_params(0.8, 50, 0.9, seed=1234, step=launch * 256 + r) for r in range(256)]
        tok, _, nk = op_sample(lib, xd, params)
        assert (nk == ref["n_kept"]).all()
        np.add.at(counts, tok, 1)
        n += 256
    q = ref["q"]
    assert counts[q == 0].sum() == 0
    exp = q * n
    big = exp >= 5
    obs = np.append(counts[big], counts[~big].sum())
    ex = np.append(exp[big], exp[~big].sum())
    if ex[-1] == 0:
        obs, ex = obs[:-1], ex[:-1]
    stat, pval = scipy_stats.chisquare(obs, ex)
    print(f"chi-square over {len(obs)} bins, {n} draws: stat {stat:.1f}, p {pval:.4f}")
    assert pval > 1e-4


def test_determinism_independence_and_top1_argmax(cuda, lib):
    g = torch.Generator().manual_seed(5)
    V = 32001
    x = torch.randn(64, V, generator=g) * 2
    x[torch.arange(64), torch.randint(0, V, (64,), generator=g)] = 12.0      # a unique maximum per row
    x = x.half()
    xd = x.to(cuda)
    params = [sampling_params(0.9, [0, 50][r % 2], [1.0, 0.9][(r // 2) % 2], seed=77 + r, step=r) for r in range(64)]
    a, _, _ = op_sample(lib, xd, params)
    b, _, _ = op_sample(lib, xd, params)
    assert (a == b).all()
    sub = [5, 17, 40]
    c, _, _ = op_sample(lib, xd[sub].contiguous(), [params[i] for i in sub])
    assert c.tolist() == a[sub].tolist()
    top1 = [sampling_params(1.0, 1, None, seed=s, step=s * 7) for s in range(64)]
    t1, _, nk = op_sample(lib, xd, top1)
    assert (nk == 1).all()
    assert t1.tolist() == x.float().argmax(1).tolist()


def test_op_rejects_bad_parameters(cuda, lib):
    xd = torch.zeros(1, 8, dtype=torch.float16, device=cuda)
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=float("nan"))):
        p = sampling_params(1.0, 50, None)
        for k, v in bad.items():
            setattr(p, k, v)
        with pytest.raises(_lib.VstarError):
            op_sample(lib, xd, [p])


# ------------------------------------------------ the VQA-LLM decode ------------------------------------------------
def _engine():
    from tests.test_vqa_gpu import engine_for
    from vstar_amd.config import VQAConfig
    cfg = VQAConfig.tiny()
    return engine_for(cfg, 0), cfg


def test_forward_sample_equals_host_oracle_loop(cuda):
    from vstar_amd.vqa_engine import Seq
    eng, cfg = _engine()
    g = torch.Generator().manual_seed(31)
    eng.encode_images(torch.randn(1, 3, 224, 224, generator=g), 0)
    ids = [1] + torch.randint(3, 300, (9,), generator=g).tolist()
    ids[2] = -200
    rows = eng.expand_ids(ids, [0], [], None, None)
    seeds, steps = (11, 12), 8
    p = [sampling_params(0.8, 50, 0.9, seed=s) for s in seeds]
    # device: both sequences in one call per step, slots 0 / 1
    got = [[], []]
    tok = eng.forward_sample([Seq(rows, kv_slot=0), Seq(rows, kv_slot=1)], [(0, -1), (1, -1)], p)
    for t in range(steps):
        for i in range(2):
            got[i].append(int(tok[i]))
        if t + 1 < steps:
            pp = [sampling_params(0.8, 50, 0.9, seed=s, step=t + 1) for s in seeds]
            tok = eng.forward_sample([Seq([got[i][-1]], kv_slot=i, past_len=len(rows) + t) for i in range(2)], [(0, 0), (1, 0)], pp)
    # host: the same calls (slots 2 / 3) with the logits brought back, fed the device's tokens; the oracle draws with the same
    # uniforms and must pick the device's token except at a prefix-mass boundary
    compared = excused = 0
    lg, _ = eng.forward([Seq(rows, kv_slot=2), Seq(rows, kv_slot=3)], [(0, -1), (1, -1)])
    for t in range(steps):
        for i, s in enumerate(seeds):
            ref = S.sample_row(torch.from_numpy(lg[i]), float(np.float32(0.8)), 50, 0.9, S.uniform(s, t))
            if ref["token"] != got[i][t]:
                assert ref["u_dist"] < U_EPS or ref["p_dist"] < 1e-6, (i, t, got[i][t], ref["token"])
                excused += 1
            compared += 1
        if t + 1 < steps:
            lg, _ = eng.forward([Seq([got[i][t]], kv_slot=2 + i, past_len=len(rows) + t) for i in range(2)], [(0, 0), (1, 0)])
    print(f"forward_sample vs host oracle: {compared} draws, {excused} excused")
    assert excused <= 1


def test_vqa_llm_sampled_free_form(cuda):
    from PIL import Image
    from tests.test_vqa_gpu import _vqa_llm
    from vstar_amd.vqa_engine import Seq
    llm, cfg = _vqa_llm(0)
    rng = np.random.default_rng(9)
    image = Image.fromarray(rng.integers(0, 256, (300, 420, 3), dtype=np.uint8))
    q = "What is in the picture?"
    samples = [dict(image=image, question=q), dict(image=image, question="Describe it."), dict(image=image, question=q)]
    texts = llm.free_form_batch(samples, max_new_tokens=6, temperature=0.8, seed=40)
    batch_ids = [list(x) for x in llm.generated_ids]
    for i, s in enumerate(samples):
        one = llm.free_form_inference(image, s["question"], temperature=0.8, max_new_tokens=6, seed=40 + i)
        assert one == texts[i] and list(llm.generated_ids[0]) == batch_ids[i], i
    # per-sample seeds override the base seed
    llm.free_form_batch([dict(image=image, question=q, seed=42)], max_new_tokens=6, temperature=0.8, seed=0)
    assert list(llm.generated_ids[0]) == batch_ids[2]
    # reproducible: explicit seed, and torch.manual_seed for seed=None
    a = llm.free_form_inference(image, q, temperature=0.8, max_new_tokens=6, seed=3)
    assert a == llm.free_form_inference(image, q, temperature=0.8, max_new_tokens=6, seed=3)
    torch.manual_seed(123)
    a = llm.free_form_inference(image, q, temperature=1.0, max_new_tokens=6)
    ids_a = list(llm.generated_ids[0])
    torch.manual_seed(123)
    llm.free_form_inference(image, q, temperature=1.0, max_new_tokens=6)
    assert list(llm.generated_ids[0]) == ids_a
    # a hot temperature spreads the draws
    seqs = set()
    for s in range(6):
        llm.free_form_inference(image, q, temperature=5.0, top_k=0, max_new_tokens=6, seed=s)
        seqs.add(tuple(llm.generated_ids[0]))
    assert len(seqs) >= 2
    # temperature 0 is the greedy decode: the engine's arg-max, step by step
    llm.free_form_inference(image, q, max_new_tokens=6)
    greedy = list(llm.generated_ids[0])
    img_slots, _ = llm._encode(image, None, 0)
    _, rows = llm._question_rows(q, img_slots, [], None, None)
    _, nxt = llm.engine.forward([Seq(rows, kv_slot=0)], [(0, -1)], logits=False)
    host = [int(nxt[0])]
    while len(host) < len(greedy):
        _, nxt = llm.engine.forward([Seq([host[-1]], kv_slot=0, past_len=len(rows) + len(host) - 1)], [(0, 0)], logits=False)
        host.append(int(nxt[0]))
    assert greedy == host
    with pytest.raises(NotImplementedError):
        llm.free_form_inference(image, q, temperature=0.8, num_beams=2)
    with pytest.raises(ValueError):
        llm.free_form_inference(image, q, temperature=-1.0)


def test_llava_search_model_generate_samples(cuda):
    from PIL import Image
    from vstar_amd import vqa
    from vstar_amd.api import load_pretrained_model
    from vstar_amd.config import VQAConfig
    from vstar_amd.weights import random_state_dict
    cfg = VQAConfig.tiny()
    sd = random_state_dict(cfg, seed=0, dtype=torch.float16)
    tokenizer, model, image_processor, _ = load_pretrained_model("seal_vqa_7b", None, "seal_vqa_7bllava", cfg=cfg, state_dict=sd)
    llm = vqa.VQA_LLM(cfg=cfg, engine=model.engine)
    rng = np.random.default_rng(5)
    image = Image.fromarray(rng.integers(0, 256, (300, 420, 3), dtype=np.uint8))
    q = "What is in the picture?"
    input_ids = torch.tensor(vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + q), tokenizer)).unsqueeze(0)
    image_tensor = image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0]
    kw = dict(images=image_tensor.unsqueeze(0).half(), object_features=None, images_long=None, objects_long=None, num_beams=1,
              max_new_tokens=6, use_cache=True)
    out = model.generate(input_ids, do_sample=True, temperature=0.8, top_p=0.9, seed=17, **kw)
    assert out.dim() == 2 and out.shape[0] == 1 and (out[:, :input_ids.shape[1]] == input_ids).all()
    llm.free_form_inference(image, q, temperature=0.8, top_p=0.9, max_new_tokens=6, seed=17)
    assert out[0, input_ids.shape[1]:].tolist() == list(llm.generated_ids[0])
    with pytest.raises(ValueError):
        model.generate(input_ids, do_sample=True, temperature=0, **kw)
    with pytest.raises(NotImplementedError):
        model.generate(input_ids, do_sample=True, temperature=0.8, **{**kw, "num_beams": 2})
