"""Batched multiple-choice scoring on the MI355X (csrc/score.hip, VQA_LLM.option_losses_batch): the op against
the CPU oracle (tests/_score_oracle.py), the forward tail against the oracle applied to the logits the plain forward returns
for the same arguments, the 256-row chunking, the batched Python API against today's host-logits path and against the
reference algorithm (oracle/vqa_oracle.py), and the evaluation loop with --vqa-batch."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import vqa_oracle as O
from tests import _score_oracle as S
from vstar_amd import _lib
from vstar_amd.config import VQAConfig
from vstar_amd.vqa_engine import Seq, VqaEngine
from vstar_amd.weights import random_state_dict

pytestmark = pytest.mark.gpu


def op_score(lib, x_dev, targets, vocab=None, want_rank=True):
    rows, ld = x_dev.shape
    vocab = ld if vocab is None else vocab
    tg = np.ascontiguousarray(targets, np.int32)
    nll, lse = np.empty(rows, np.float32), np.empty(rows, np.float64)
    rank = np.empty(rows, np.int32) if want_rank else None
    dt = _lib.F16 if x_dev.dtype == torch.float16 else _lib.BF16
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None       # noqa: E731
    _lib.check_vqa(lib.vstar_vqa_op_score(ctypes.c_void_p(x_dev.data_ptr()), dt, rows, vocab, ld, p(tg), p(nll), p(rank), p(lse)))
    return nll, rank, lse


def make_row(kind, V, g):
    x = torch.randn(V, generator=g) * 3
    if kind == "peaked":
        x = torch.randn(V, generator=g)
        x[int(torch.randint(0, V, (1,), generator=g))] += 15
    elif kind == "flat":
        x = torch.full((V,), 1.5)
    elif kind == "masked":
        m = torch.rand(V, generator=g) < 0.5
        x = torch.where(m, torch.where(torch.rand(V, generator=g) < 0.5, -float("inf"), -65504.0), x)
        x[0] = 2.0
    return x


def check_rows(nll_dev, rank_dev, logits, targets, what):
    """The <= 1-ulp rule: nll equals the oracle's fp32 value or its fp32 neighbour (device exp / log in double may differ from
    libm in the last place before the single rounding); the rank is equal exactly.  Returns the rows that needed the neighbour."""
    nll, rank, _, _ = S.score(logits, targets)
    d = S.ulp_distance(nll_dev, nll.numpy())
    assert d.max() <= 1, (what, int(d.argmax()), nll_dev[d.argmax()], nll[int(d.argmax())])
    if rank_dev is not None:
        assert np.array_equal(rank_dev, rank.numpy()), what
    return int((d == 1).sum())


def test_op_against_oracle(cuda, lib):
    kinds = ("random", "peaked", "flat", "masked")
    n_rows = n_nb = 0
    for dtype in (torch.float16, torch.bfloat16):
        for V in (1, 2, 320, 32001, 32768, 32769, 131075):
            g = torch.Generator().manual_seed(V)
            rows = [make_row(kinds[r % 4], V, g) for r in range(12)]
            x = torch.stack(rows).to(dtype)
            tg = torch.randint(0, V, (12,), generator=g)
            tg[0] = int(x[0].float().argmax())                         # a greedy target: rank 0
            if V > 4:
                tg[3] = int(torch.isinf(x[3].float()).nonzero()[0])    # a -inf target: +inf
            ld = V + 5
            xd = torch.zeros(12, ld, dtype=dtype)
            xd[:, :V] = x
            nll, rank, lse = op_score(lib, xd.to(cuda), tg.numpy(), vocab=V)
            n_nb += check_rows(nll, rank, x, tg, (dtype, V))
            n_rows += 12
            assert rank[0] == 0
            if V > 4:
                assert nll[3] == np.inf
            ref_lse = S.score(x, tg)[2].numpy()
            np.testing.assert_allclose(lse, ref_lse, rtol=1e-10, atol=1e-10)
            nll2, none, _ = op_score(lib, xd.to(cuda), tg.numpy(), vocab=V, want_rank=False)     # rank is optional
            assert none is None and np.array_equal(nll2.view(np.int32), nll.view(np.int32))
    print(f"score op vs oracle: {n_rows} rows, {n_nb} needed the fp32 neighbour")


def test_op_special_rows_and_errors(cuda, lib):
    inf, nan = float("inf"), float("nan")
    x = torch.tensor([[1.0, 2.0, 2.0, 3.0],          # ties: strictly greater only
                      [1.0, 2.0, 2.0, 3.0],          # the same row, another target
                      [-inf, 0.0, -inf, -inf],       # one-hot
                      [1.0, nan, 0.0, 0.0],          # NaN -> NaN
                      [0.0, 0.0, 0.0, 0.0]]).half()  # flat
    nll, rank, _ = op_score(lib, x.to(cuda), [1, 3, 1, 0, 2])
    check_rows(nll, rank, x, [1, 3, 1, 0, 2], "special")
    assert rank.tolist()[:3] == [1, 0, 0] and nll[2] == 0.0 and np.isnan(nll[3]) and rank[4] == 0
    assert nll[4] == np.float32(np.log(4.0))
    xd = torch.zeros(2, 8, dtype=torch.float16, device=cuda)
    for tg in ([0, 8], [-1, 0]):
        with pytest.raises(_lib.VstarError, match="target"):
            op_score(lib, xd, tg)


# ------------------------------------------------ the engine ------------------------------------------------
_LLM = {}


def _llm(max_slots=8):
    from vstar_amd.vqa import VQA_LLM
    if max_slots not in _LLM:
        cfg = VQAConfig.tiny(max_slots=max_slots)
        eng = VqaEngine(cfg, 0)
        eng.load_state_dict(random_state_dict(cfg, seed=0, dtype=torch.float16))
        _LLM[max_slots] = (VQA_LLM(cfg=cfg, engine=eng), cfg)
    return _LLM[max_slots]


def _prompts(eng, n_texts=(40, 17, 64), seed=31):
    g = torch.Generator().manual_seed(seed)
    eng.encode_images(torch.randn(len(n_texts), 3, 224, 224, generator=g), 0)
    out = []
    for i, n in enumerate(n_texts):
        ids = [1] + torch.randint(3, 300, (n,), generator=g).tolist()
        ids[2] = -200
        out.append(eng.expand_ids(ids, [i], [], [i != 1], None))       # sequence 1 takes the short features
    return out


def test_tail_equals_oracle_on_the_logits_of_the_same_call(cuda):
    llm, cfg = _llm()
    eng = llm.engine
    g = torch.Generator().manual_seed(7)
    rows = _prompts(eng)
    n_nb = 0
    # a ragged prefill: the last row of every sequence (one of them three times with different targets), some inner rows
    seqs = [Seq(r, kv_slot=i) for i, r in enumerate(rows)]
    want = [(0, -1), (1, -1), (1, -1), (1, -1), (2, -1), (0, 5), (2, 100), (1, 0)]
    tg = torch.randint(0, cfg.llm_vocab, (len(want),), generator=g)
    logits, arg = eng.forward(seqs, want)
    tg[0] = int(arg[0])                                                 # a greedy target: rank 0
    nll, rank = eng.forward_score(seqs, want, tg.numpy(), rank=True)
    n_nb += check_rows(nll, rank, torch.from_numpy(logits), tg, "prefill")
    assert rank[0] == 0 and nll.dtype == np.float32 and rank.dtype == np.int32
    assert np.array_equal(eng.forward_score(seqs, want, tg.numpy()).view(np.int32), nll.view(np.int32))
    # forked multi-row continuations; slot 5 was left ancestral by a beam reorder (the fork makes it an ordinary slot again)
    conts = [torch.randint(3, 300, (n,), generator=g).tolist() for n in (7, 1, 12, 4)]
    fork = [Seq(c, kv_slot=4 + j, past_len=len(rows[j % 3]), prefix_slot=j % 3) for j, c in enumerate(conts)]
    want = [(j, t) for j, c in enumerate(conts) for t in range(len(c) - 1)] + [(0, 2), (2, 0)]      # two duplicates
    tg = torch.tensor([c[t + 1] for c in conts for t in range(len(c) - 1)] + [11, 12])
    eng.kv_reorder([5], [6], 0, 40)
    logits, _ = eng.forward(fork, want)
    eng.kv_reorder([5], [6], 0, 40)
    nll, rank = eng.forward_score(fork, want, tg.numpy(), rank=True)
    n_nb += check_rows(nll, rank, torch.from_numpy(logits), tg, "fork")
    print(f"forward_score vs oracle on the same call's logits: {n_nb} rows needed the fp32 neighbour")


def test_chunked_tail_and_limits(cuda):
    llm, cfg = _llm()
    eng = llm.engine
    rows = _prompts(eng, (60, 60, 60), seed=5)
    seqs = [Seq(r, kv_slot=i) for i, r in enumerate(rows)]
    flat = [(i, t) for i, r in enumerate(rows) for t in range(len(r))]
    assert len(flat) >= 600
    want = flat[:600]
    tg = torch.randint(0, cfg.llm_vocab, (600,), generator=torch.Generator().manual_seed(3))
    nll, rank = eng.forward_score(seqs, want, tg.numpy(), rank=True)
    n_nb = 0
    for lo, hi in ((0, 256), (256, 512), (512, 600)):
        logits, _ = eng.forward(seqs, want[lo:hi])
        n_nb += check_rows(nll[lo:hi], rank[lo:hi], torch.from_numpy(logits), tg[lo:hi], (lo, hi))
        part = eng.forward_score(seqs, want[lo:hi], tg[lo:hi].numpy())          # the chunk as a call of its own: same bits
        assert np.array_equal(part.view(np.int32), nll[lo:hi].view(np.int32)), (lo, hi)
    print(f"chunked forward_score (600 rows): {n_nb} rows needed the fp32 neighbour")
    one = [Seq([5, 6, 7], kv_slot=0)]
    with pytest.raises(_lib.VstarError, match="max_rows"):
        eng.forward_score(one, [(0, 0)] * (cfg.max_rows + 1), [1] * (cfg.max_rows + 1))
    with pytest.raises(_lib.VstarError, match="target"):
        eng.forward_score(one, [(0, 0), (0, 1)], [1, cfg.llm_vocab])
    with pytest.raises(ValueError, match="targets"):
        eng.forward_score(one, [(0, 0), (0, 1)], [1])
    with pytest.raises(_lib.VstarError, match="bad argument"):                  # the other tails keep the 256-row limit
        eng.forward(one, [(0, 0)] * 257)


# ------------------------------------------------ the Python API ------------------------------------------------
def _image(seed, size=(300, 420)):
    from PIL import Image
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, (*size, 3), dtype=np.uint8))


def _class_sample(llm):
    """The sample of tests/test_vqa_gpu.py::test_vqa_llm_class_against_oracle: two object crops, short image features and long
    object features, four options, one of them a single word."""
    image = _image(5)
    crops = torch.stack([llm.get_object_crop(image, [40, 30, 50, 60], patch_scale=1.2),
                         llm.get_object_crop(image, [200, 100, 90, 40], patch_scale=1.2)], 0)
    question = "Additional visual information to focus on: mug <object> at location [0.1,0.1,0.2,0.3]; cup <object> at " \
               "location [0.5,0.3,0.7,0.5].\nWhat is the colour of the mug?"
    options = ["The colour of the mug is red.", "The colour of the mug is blue.", "green", "The mug is yellow and white."]
    return dict(image=image, question=question, options=options, object_crops=crops, images_long=[False], objects_long=[True, True])


def _losses_today(llm, s):
    return llm.option_losses(s["image"], s["question"], s["options"], s.get("object_crops"), s.get("images_long"),
                             s.get("objects_long"))


def _host_logits(llm, s):
    """Per option (logits [n, V] fp16, ids): the rows today's option_losses feeds to cross_entropy, from the same two calls."""
    eng = llm.engine
    img, obj = llm._encode(s["image"], s.get("object_crops"), 0)
    q_ids, q_rows = llm._question_rows(s["question"], img, obj, s.get("images_long"), s.get("objects_long"))
    q_logits, _ = eng.forward([Seq(q_rows, kv_slot=0)], [(0, -1)])
    out = []
    for j, o in enumerate(s["options"]):
        ids = llm._question_rows(s["question"], img, obj, s.get("images_long"), s.get("objects_long"), answer=o)[0][len(q_ids):]
        lg = q_logits[0:1]
        if len(ids) > 1:
            more, _ = eng.forward([Seq(ids, kv_slot=1, past_len=len(q_rows), prefix_slot=0)], [(0, t) for t in range(len(ids) - 1)])
            lg = np.concatenate([lg, more])
        out.append((torch.from_numpy(lg), ids))
    return out


def test_batch_of_one_equals_todays_path(cuda):
    llm, cfg = _llm()
    s = _class_sample(llm)
    today = _losses_today(llm, s)
    batch = llm.option_losses_batch([s])[0]
    per_tok = llm.score_continuations(s["image"], s["question"], s["options"], s["object_crops"], s["images_long"], s["objects_long"])
    assert [len(v) for v in per_tok] == [len(ids) for _, ids in _host_logits(llm, s)] and min(len(v) for v in per_tok) >= 1
    n_mid = 0
    for a, b, (lg, ids) in zip(batch, today, _host_logits(llm, s)):
        assert a.dtype == torch.float16 and a.dim() == 0
        _, _, lse, nll64 = S.score(lg, ids)
        verdict = S.losses_agree(a, b, nll64, lse)
        print("loss device", float(a), "host", float(b), verdict)
        assert verdict != "differ", (float(a), float(b))
        n_mid += verdict == "midpoint"
    assert n_mid <= 0.02 * len(batch)
    for a, v in zip(batch, per_tok):
        assert float(a) == float(S.loss(v))
    assert llm.multiple_choices_batch([s])[0] == llm.multiple_choices_inference(
        s["image"], s["question"], s["options"], s["object_crops"], images_long=s["images_long"], objects_long=s["objects_long"])


def _many_samples(llm):
    """Five samples of different prompt lengths, option counts and object-crop counts: (KV slots, feature slots) =
    (5, 3), (3, 1), (4, 6), (3, 3), (4, 1)."""
    def crops(image, n):
        return torch.stack([llm.get_object_crop(image, [20 + 30 * k, 30 + 10 * k, 50, 60], patch_scale=1.2) for k in range(n)], 0)

    def focus(n, q):
        return "Additional visual information to focus on: " + "; ".join(
            f"thing{k} <object> at location [0.1,0.1,0.{k + 2},0.3]" for k in range(n)) + ".\n" + q
    im = [_image(40 + i, (240 + 20 * i, 320)) for i in range(5)]
    return [
        dict(_class_sample(llm)),
        dict(image=im[1], question="Is the dog left of the cat?", options=["The dog is left of the cat.", "right"]),
        dict(image=im[2], question=focus(5, "What is on the table?"), options=["a cup", "a red plate with food", "nothing at all"],
             object_crops=crops(im[2], 5), images_long=[False], objects_long=[False] * 5),
        dict(image=im[3], question=focus(2, "What colour is the car?"), options=["blue", "The car is green."],
             object_crops=crops(im[3], 2), images_long=[False], objects_long=[True, True]),
        dict(image=im[4], question="How many people are there in the picture?", options=["one", "two people", "There are three."]),
    ]


def _oracle_losses(llm, cfg, sd, s):
    """oracle/vqa_oracle.multiple_choice (the reference algorithm in fp32) on the sample, from the same host preprocessing."""
    from vstar_amd import vqa
    crops = s.get("object_crops")
    pix = [llm.image_processor.preprocess(s["image"])["pixel_values"][0]] + ([c for c in crops] if crops is not None else [])
    lo, sh = O.encode_images(sd, cfg, torch.stack(pix, 0).half().float())

    def ids_of(answer):
        return vqa.tokenizer_image_object_token(vqa.v1_prompt("<image>\n" + s["question"], answer), llm.tokenizer)
    q_ids = ids_of(None)
    emb = O.splice(sd, q_ids, lo[:1], sh[:1], lo[1:], sh[1:], s.get("images_long"), s.get("objects_long"))
    return O.multiple_choice(sd, cfg, emb, [ids_of(o)[len(q_ids):] for o in s["options"]])


def test_batch_of_many_against_the_reference_algorithm(cuda):
    llm, cfg = _llm(16)                                  # 12 KV slots, 5 feature slots: one chunk
    sd = random_state_dict(cfg, 0, torch.float32)
    samples = [_many_samples(llm)[i] for i in (0, 1, 4)]
    losses = llm.option_losses_batch(samples)
    picks = llm.multiple_choices_batch(samples)
    assert [len(x) for x in losses] == [4, 2, 3]
    for s, got, pick in zip(samples, losses, picks):
        ref, ref_pick = _oracle_losses(llm, cfg, sd, s)
        print("losses", [round(float(x), 4) for x in got], "oracle", [round(float(x), 4) for x in ref], pick, ref_pick)
        np.testing.assert_allclose([float(x) for x in got], ref.numpy(), atol=0.03)
        srt = np.sort(ref.numpy())
        if srt[1] - srt[0] > 0.06:
            assert pick == ref_pick
        assert pick == int(torch.stack(got).argmin())


def test_large_batch_is_split_into_chunks(cuda):
    llm, cfg = _llm()                                    # max_slots 8, max_images 8
    samples = _many_samples(llm)
    got = llm.option_losses_batch(samples)
    by_hand = []
    for chunk in (samples[0:2], samples[2:3], samples[3:5]):     # 8 slots | 12 slots would not fit | 9 feature slots would not
        by_hand += llm.option_losses_batch(chunk)
    assert [[float(x) for x in per] for per in got] == [[float(x) for x in per] for per in by_hand]
    assert llm.multiple_choices_batch(samples) == [int(torch.stack(per).argmin()) for per in by_hand]
    with pytest.raises(ValueError, match="KV slots"):
        llm.option_losses_batch([dict(image=samples[1]["image"], question="q", options=["a"] * cfg.max_slots)])
    with pytest.raises(ValueError, match="max_images"):
        im = samples[2]["image"]
        llm.option_losses_batch([dict(image=im, question="q", options=["a"],
                                      object_crops=torch.zeros(cfg.max_images, 3, 224, 224))])


def test_nothing_else_moved(cuda):
    """A multiple_choices_batch in between leaves greedy, sampled and beam decodes and today's option_losses unchanged."""
    llm, cfg = _llm()
    s = _class_sample(llm)

    def snapshot():
        out = []
        for kw in (dict(), dict(temperature=0.8, top_p=0.9, seed=11), dict(num_beams=2)):
            llm.free_form_inference(s["image"], "What is in the picture?", max_new_tokens=6, **kw)
            out.append([list(x) for x in llm.generated_ids])
        out.append([float(x) for x in _losses_today(llm, s)])
        return out
    before = snapshot()
    llm.multiple_choices_batch(_many_samples(llm))
    assert snapshot() == before


def test_eval_loop_with_vqa_batch(cuda, tmp_path):
    """eval_model(vqa_batch=4) on the synthetic benchmark of tests/test_vqa_gpu.py::test_eval_loop_end_to_end_on_synthetic_benchmark:
    same schema, order, missing objects and search results; the same choice wherever the single run's two best losses differ by
    more than 0.06."""
    import json
    from types import SimpleNamespace
    from PIL import Image
    from vstar_amd import bench_eval
    from vstar_amd.config import VSMConfig
    from vstar_amd.vsm import VSM
    llm, _ = _llm()
    vsm = VSM(SimpleNamespace(version="synthetic", vision_tower="synthetic", conv_type="llava_v1", use_mm_start_end=True,
                              model_max_length=512), cfg=VSMConfig.tiny(max_text_len=128), synthetic_seed=0)
    rng = np.random.default_rng(9)
    for split, n in (("direct_attributes", 2), ("relative_position", 1)):
        d = tmp_path / split
        d.mkdir()
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)).save(d / f"img{i}.jpg")
            json.dump({"question": "What is the colour of the mug?", "options": ["red", "blue", "green", "black"]},
                      open(d / f"img{i}.json", "w"))
    calls = {"n": 0, "batch": 0}
    real_one, real_batch = llm.free_form_inference, llm.free_form_batch

    def forced():
        calls["n"] += 1
        return bench_eval.MISSING_MSG + " mug, table." if calls["n"] % 2 else "It is red."

    def free_form(image, question, **kw):
        real_batch([dict(image=image, question=question)], max_new_tokens=3)      # (free_form_inference's own body, unpatched)
        return forced()

    def free_form_batch(samples, *a, **kw):
        real_batch(samples, max_new_tokens=3)
        calls["batch"] += 1
        return [forced() for _ in samples]
    llm.free_form_inference, llm.free_form_batch = free_form, free_form_batch
    try:
        args1 = SimpleNamespace(benchmark_folder=str(tmp_path), output_path=str(tmp_path / "r1.json"), minimum_size_scale=4.0,
                                minimum_size=224, vsm_model_path="synthetic", max_found_objects=5)
        one = bench_eval.eval_model(args1, llm, vsm)
        assert calls["batch"] == 0
        calls["n"] = 0
        args4 = SimpleNamespace(**{**vars(args1), "vqa_batch": 4, "output_path": str(tmp_path / "r4.json")})
        four = bench_eval.eval_model(args4, llm, vsm)
        assert calls["batch"] == 1
    finally:
        llm.free_form_inference, llm.free_form_batch = real_one, real_batch
    assert json.load(open(args4.output_path)) == four and list(four) == list(one)
    mean_color = tuple(int(x * 255) for x in llm.image_processor.image_mean)
    n_cmp = 0
    for split in one:
        assert len(one[split]) == len(four[split])
        for a, b in zip(one[split], four[split]):
            assert set(a) == set(b) == {"question", "options", "image", "prediction_freeform", "missing_objects", "search_result",
                                        "option_chosen", "correct"}
            for k in ("question", "options", "image", "prediction_freeform", "missing_objects", "search_result"):
                assert a[k] == b[k], k
            assert b["correct"] == (1 if b["option_chosen"] == 0 else 0)
            e = dict(path=str(tmp_path / split / a["image"]), question=a["question"], options=a["options"],
                     missing=a["missing_objects"], found=a["search_result"])
            srt = np.sort([float(x) for x in _losses_today(llm, bench_eval._choice_sample(llm, e, mean_color))])
            if srt[1] - srt[0] > 0.06:
                assert a["option_chosen"] == b["option_chosen"]
                n_cmp += 1
    assert any(r["missing_objects"] for sp in four.values() for r in sp)
    print(f"eval loop: {n_cmp} choices compared")
    assert n_cmp >= 1, "no question of the synthetic benchmark has a > 0.06 gap: the choices were never compared"
