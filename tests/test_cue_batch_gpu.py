"""vstar_vsm_generate_batch on the MI355X: sequence i of a batched greedy decode has exactly the tokens vstar_vsm_generate gives for
the same pixels and prompt — whatever the batch size, the eos id, the per-sequence caps, the pixel source and the launch mode —
and the stream search built on it equals the per-sample loop.  Tiny engine of tests/test_vsm_gpu.py (224 px: P = 256 image tokens,
so every decode step is past the split-KV path's 256-key threshold); trained-like weights (seed 5) and the i.i.d. random set, whose
nearly flat logits turn any arithmetic difference into a token flip."""
import ctypes
import warnings
from collections import Counter

import numpy as np
import pytest
import torch

from vstar_amd import _lib
from vstar_amd import preprocess as pp
from vstar_amd.config import VSMConfig
from vstar_amd.engine import VstarEngine
from vstar_amd.search import visual_search, visual_search_stream
from vstar_amd.synthetic import synthetic_image
from vstar_amd.vsm import VSM
from vstar_amd.weights import random_state_dict, template_chain, trained_like_state_dict

pytestmark = pytest.mark.gpu

N_MAX = 16
NAMES = ["kite", "red umbrella", "small brown dog", "traffic light on pole", "cup of hot black coffee",
         "old wooden boat near the pier"]                                   # one to six words: ragged prompts
SIZES = [(300, 260), (224, 224), (640, 200), (180, 500), (1000, 700), (97, 131), (400, 400), (520, 380)]
CAPS = [1, 2, 7, 12]
CAP = 12


def _cfg(kind):
    wide = dict(llm_hidden=2048, llm_heads=16, llm_mlp=4096, llm_layers=2) if kind == "wide" else {}
    return VSMConfig.tiny(max_batch=8, max_text_len=96, **wide)


def _weights(kind, cfg):
    if kind == "trained":
        return trained_like_state_dict(cfg, seed=5, dtype=torch.bfloat16, share_layers=False,
                                       chain=template_chain(pp.SyntheticTokenizer(cfg.llm_vocab)))
    return random_state_dict(cfg, seed=11, dtype=torch.bfloat16)


class _Rig:
    """One engine with its 16 requests and a cache of solo decodes (vstar_vsm_generate), each computed once."""

    def __init__(self, kind):
        self.cfg = _cfg(kind)
        self.eng = VstarEngine(self.cfg, 0)
        self.eng.load_state_dict(_weights(kind, self.cfg))
        tok = pp.SyntheticTokenizer(self.cfg.llm_vocab)
        self.images = [synthetic_image(*SIZES[i % len(SIZES)], 70 + i) for i in range(N_MAX)]
        self.clip = torch.from_numpy(np.stack([pp.clip_preprocess(im, self.cfg.clip_image_size) for im in self.images])).bfloat16()
        self.prompts = [pp.tokenizer_image_token(pp.build_prompt(pp.CUE_QUESTION.format(NAMES[i % len(NAMES)])), tok)
                        for i in range(N_MAX)]
        assert len({len(p) for p in self.prompts}) >= 4
        self._solo = {}

    def solo(self, i, cap=CAP, eos=-1, clip=None, key="host"):
        k = (key, i, cap, eos)
        if k not in self._solo:
            px = self.clip[i:i + 1] if clip is None else clip
            self._solo[k] = self.eng.generate(px, self.prompts[i], cap, eos)
        return self._solo[k]

    def an_eos(self):
        """A token of the solo outputs (not the first one) that ends the rows holding it at different steps, if there is one."""
        first = Counter()
        where = {}
        for i in range(N_MAX):
            seen = set()
            for j, t in enumerate(self.solo(i)[1:], 1):
                if t not in seen:
                    seen.add(t)
                    first[t] += 1
                    where.setdefault(t, set()).add(j)
        return max(first, key=lambda t: (len(where[t]) > 1, 0 < first[t] < N_MAX, first[t]))


_RIGS = {}


def _rig(kind):
    if kind not in _RIGS:
        _RIGS[kind] = _Rig(kind)
    return _RIGS[kind]


@pytest.fixture(scope="module", autouse=True)
def _close_rigs(cuda):
    yield
    for r in _RIGS.values():
        r.eng.close()
    _RIGS.clear()


@pytest.mark.parametrize("kind", ["trained", "random"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 16])
def test_batch_equals_solo(n, kind):
    """eos_id = -1, an eos id taken from the solo outputs (rows finish at different steps while others run on), per-sequence caps."""
    r = _rig(kind)
    # ---- no eos: every row runs to the cap ----
    want = [r.solo(i) for i in range(n)]
    assert all(len(w) == CAP for w in want)
    got = r.eng.generate_batch(r.clip[:n], r.prompts[:n], CAP, -1)
    assert got == want
    assert r.eng.gen_attn_path() == 2                     # past 256 keys: the split-KV pair, at every n
    # ---- an eos id that some rows emit, at different steps ----
    eos = r.an_eos()
    want = [r.solo(i, eos=eos) for i in range(n)]
    got = r.eng.generate_batch(r.clip[:n], r.prompts[:n], CAP, eos)
    assert got == want
    for w in want:
        assert (w[-1] == eos and eos not in w[:-1]) or (len(w) == CAP and eos not in w)
    if n == N_MAX and kind == "random":
        ends = {len(w) for w in want}
        assert len(ends) > 1 and min(ends) < CAP        # some rows finished early, at different steps, while others ran on
    # ---- per-sequence caps ----
    caps = [CAPS[i % 4] for i in range(n)]
    want = [r.solo(i, cap=caps[i], eos=eos) for i in range(n)]
    got = r.eng.generate_batch(r.clip[:n], r.prompts[:n], caps, eos)
    assert got == want
    assert all(len(g) <= c for g, c in zip(got, caps))


@pytest.mark.parametrize("kind", ["trained", "random"])
def test_boxes_of_resident_images_in_three_slots(kind):
    """VSTAR_F_INTERNAL_PIXELS: crops of images resident in three different slots, cut and preprocessed on the GPU."""
    r = _rig(kind)
    slots = [3, 0, 17]
    imgs = [synthetic_image(900, 600, 31), synthetic_image(640, 480, 32), synthetic_image(1200, 500, 33)]
    for s, im in zip(slots, imgs):
        r.eng.set_image(im, s)
    boxes = [[0, 0, 900, 600], [100, 50, 324, 274], [0, 0, 1200, 500], [13, 27, 301, 455], [600, 0, 1200, 250],
             [450, 300, 900, 600], [0, 0, 320, 240], [5, 5, 229, 229]]
    sl = [3, 0, 17, 3, 17, 3, 0, 0]
    for n in (1, 3, 8):
        px = torch.from_numpy(r.eng.preprocess_only(boxes[:n], sl[:n])[0]).bfloat16()
        want = [r.solo(i, clip=px[i:i + 1], key="box") for i in range(n)]
        r.eng.preprocess_boxes(boxes[:n], sl[:n])
        got = r.eng.generate_batch(None, r.prompts[:n], CAP, -1, internal_pixels=True)
        assert got == want


def test_attention_path_does_not_depend_on_n():
    """16 heads: a 16-row step has 256 (row, head) pairs, past the 128 the dispatcher splits on its own.  The batched runner asks
    for a one-row step's decision, so the path — and on the random weights every token — is the solo decode's."""
    r = _rig("wide")
    assert r.cfg.llm_heads * N_MAX > 128
    want = [r.solo(i) for i in range(N_MAX)]
    solo_path = r.eng.gen_attn_path()
    assert r.eng.generate_batch(r.clip[:1], r.prompts[:1], CAP, -1) == want[:1]
    p1 = r.eng.gen_attn_path()
    assert r.eng.generate_batch(r.clip, r.prompts, CAP, -1) == want
    p16 = r.eng.gen_attn_path()
    assert solo_path == p1 == p16 == 2


@pytest.mark.parametrize("kind", ["trained", "random"])
def test_launch_by_launch_gives_the_same_tokens(kind):
    """Event profiling makes the graph path decline: the same n-row step, launch by launch."""
    r = _rig(kind)
    n = 5
    eos = r.an_eos()
    caps = [CAPS[(i + 1) % 4] for i in range(n)]
    want = [r.solo(i, cap=caps[i], eos=eos) for i in range(n)]
    want_full = [r.solo(i) for i in range(n)]
    r.eng.profile(True)
    try:
        got = r.eng.generate_batch(r.clip[:n], r.prompts[:n], caps, eos)
        got_full = r.eng.generate_batch(r.clip[:n], r.prompts[:n], CAP, -1)
        path = r.eng.gen_attn_path()
    finally:
        r.eng.profile(False)
    assert got == want and got_full == want_full and path == 2


@pytest.mark.parametrize("kind", ["trained", "random"])
def test_solo_launch_by_launch_gives_the_graph_tokens(kind):
    """vstar_vsm_generate under event profiling: the one-row step of the graph, launched by hand with the graph's key bound, so the
    same attention path and partition span — the tokens of the unprofiled solo decode (the rig's cache), no eos and eos + caps."""
    r = _rig(kind)
    n = 3
    eos = r.an_eos()
    runs = [(i, CAP, -1) for i in range(n)]
    runs += [(i, CAPS[(i + k) % 4], eos) for k in (0, 1) for i in range(n)]       # the caps of the two batched tests above
    want = [r.solo(i, cap=cap, eos=e) for i, cap, e in runs]                      # computed with profiling off
    r.eng.profile(True)
    try:
        got, paths = [], []
        for i, cap, e in runs:
            got.append(r.eng.generate(r.clip[i:i + 1], r.prompts[i], cap, e))
            paths.append(r.eng.gen_attn_path())
    finally:
        r.eng.profile(False)
    assert got == want
    assert paths == [2 if len(w) > 1 else -1 for w in want] and paths[:n] == [2] * n


def test_a_one_token_solo_decode_runs_no_step():
    r = _rig("random")
    assert r.eng.generate(r.clip[:1], r.prompts[0], CAP, -1) == r.solo(0) and r.eng.gen_attn_path() == 2
    assert r.eng.generate(r.clip[:1], r.prompts[0], 1, -1) == r.solo(0)[:1]
    assert r.eng.gen_attn_path() == -1                      # the prefill's arg-max alone: no decode step ran


def test_errors_are_refused_with_a_message_and_leave_the_engine_usable():
    r = _rig("random")
    n = 3
    want = [r.solo(i) for i in range(n)]
    assert r.eng.generate_batch(r.clip[:n], r.prompts[:n], CAP, -1) == want
    ctx = (r.cfg.n_img_tokens + r.cfg.max_text_len + 255) // 64 * 64
    no_img = [t for t in r.prompts[1] if t != -200]
    two_img = list(r.prompts[1]) + [-200]
    bad = [
        (r.clip[:0], [], CAP, "VSTAR_GEN_MAX_BATCH"),
        (torch.cat([r.clip, r.clip[:1]]), r.prompts + r.prompts[:1], CAP, "VSTAR_GEN_MAX_BATCH"),
        (r.clip[:n], [r.prompts[0], no_img, r.prompts[2]], CAP, "no image token"),
        (r.clip[:n], [r.prompts[0], two_img, r.prompts[2]], CAP, "more than one -200"),
        (r.clip[:n], r.prompts[:n], [CAP, ctx - len(r.prompts[1]) - r.cfg.n_img_tokens + 2, CAP], "exceed the decode context"),
    ]
    for clip, prompts, caps, msg in bad:
        with pytest.raises(_lib.VstarError, match=msg):
            r.eng.generate_batch(clip, prompts, caps, -1)
    # null arrays, straight at the C entry
    ids = np.ascontiguousarray(np.asarray(r.prompts[0], np.int32))
    off = np.asarray([0, len(ids)], np.int32)
    cap = np.asarray([CAP], np.int32)
    out, cnt = np.zeros((CAP,), np.int32), np.zeros((1,), np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    px = ctypes.c_void_p(r.clip[:1].contiguous().data_ptr())
    for args in ((None, p(ids), p(off), p(cap), p(out), p(cnt)), (px, None, p(off), p(cap), p(out), p(cnt)),
                 (px, p(ids), None, p(cap), p(out), p(cnt)), (px, p(ids), p(off), None, p(out), p(cnt)),
                 (px, p(ids), p(off), p(cap), None, p(cnt)), (px, p(ids), p(off), p(cap), p(out), None)):
        c, i, o, m, oi, no = args
        rc = r.eng.lib.vstar_vsm_generate_batch(r.eng.handle, 1, c, i, o, m, -1, 0, oi, no)
        assert rc == -1 and b"null" in r.eng.lib.vstar_last_error(r.eng.handle)
    # the engine is as it was: the batched call and the solo call give the tokens they gave before
    assert r.eng.generate_batch(r.clip[:n], r.prompts[:n], CAP, -1) == want
    assert r.eng.generate(r.clip[1:2], r.prompts[1], CAP, -1) == want[1]


def test_stream_on_the_engine_equals_the_per_sample_loop():
    """Three images, six samples, the cue branch forced at every expanded node, searches of 1 + 4 nodes: the stream (one batched
    decode for the six cue questions, one plain scoring step for their follow-ups) gives the loop's paths, context cues and
    detections bit for bit, and no crop needs the decode fallback."""
    r = _rig("trained")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        vsm = VSM(None, engine=r.eng, tokenizer=pp.SyntheticTokenizer(r.cfg.llm_vocab), strict_template=True)
    imgs = [synthetic_image(640, 480, 41), synthetic_image(700, 460, 42), synthetic_image(600, 600, 43)]
    names = ["kite", "red umbrella", "dog", "traffic light", "boat", "small bench"]
    samples = [(imgs[k % 3], names[k], None, 360) for k in range(6)]      # 360: the root expands, its four children do not
    kw = dict(confidence_high=2.0, confidence_low=0.0, target_cue_threshold=1e9, target_cue_threshold_minimum=1e9,
              noun_chunker=lambda p: [" ".join(p.split()[:3]) or "area"])
    vsm.group_prompts = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loop, paths = [], []
        for img, name, gt, sm in samples:
            st = {}
            loop.append(visual_search(vsm, img, name, gt, sm, speculate=False, stats=st, **kw))
            paths.append(st["search_path"])
        st = {"keep_paths": True}
        got = visual_search_stream(vsm, samples, window=6, stats=st, **kw)
    assert all(len(p) == 5 for p in paths)
    for a, b in zip(loop, got):
        assert a[1] == b[1] and a[2] == b[2] and a[0]["bbox"] == b[0]["bbox"]
        assert torch.equal(a[0]["detection_result"], b[0]["detection_result"])
    assert st["visit_orders"] == [[tuple(int(v) for v in p["bbox"]) for p in path] for path in paths]
    cues = [[p.get("context_cue") for p in path] for path in paths]
    assert st["context_cues"] == cues and all(c[0] is not None for c in cues)
    assert st["cue_requests"] == 6 and st["cue_calls"] < st["cue_requests"] and st["seg_calls"] < st["seg_requests"] == 6
    assert vsm.timers["generate_tokens"] > 0 and vsm.timers["generate_s"] > 0
    assert vsm.fallback_log == []
