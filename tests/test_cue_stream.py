"""The contextual-cue branch in the stream driver: the cue questions of all live searches of a round go to ONE batched decode
(`generate_boxes`), their locate follow-ups to ONE plain scoring step, and every search still decides what the per-sample loop decides.
CPU only: the VSM is a slot stand-in whose cue text and records are deterministic functions of (crop pixels, question)."""
import os
import re
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from vstar_amd import _lib, search
from vstar_amd.synthetic import synthetic_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORDS = ["shelf", "window", "bench", "counter", "road", "tree", "table", "wall"]


class _CueVSM:
    """Slot stand-in with the contextual-cue entries.  Everything it returns is a function of (the crop's pixels, the question), so
    the host-crop calls of the per-sample loop (`inference`, `inference_batch`) and the box calls of the stream (`generate_boxes`,
    `inference_boxes`) agree, the cue phrase differs per node, and with it the follow-up question.  Heat maps come in two scales
    (maxima around 24 and around 2.4) so that a threshold of 10 sends roughly half of the expanded nodes into the branch."""
    supports_gpu_preprocess = True
    supports_deferred_mismatch = False
    supports_device_reductions = True
    max_image_slots = 64

    def __init__(self, max_batch=8, fail_cue=False):
        self.cfg = SimpleNamespace(max_batch=max_batch)
        self.images, self.fail_cue = {}, fail_cue
        self.calls, self.gen_calls, self.seg_calls, self.solo_cue, self.solo_seg = [], [], [], [], []

    def set_image(self, image, slot=0):
        self.images[slot] = image

    @staticmethod
    def _key(crop):
        return zlib.crc32(np.asarray(crop.convert("RGB").resize((8, 8))).tobytes())

    def _crop_key(self, slot, b):
        return self._key(self.images[slot].crop((int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3]))))

    @staticmethod
    def _record(key, q):
        seed = zlib.crc32(repr((key, q)).encode())
        g = torch.Generator().manual_seed(seed % (2 ** 31))
        low = torch.randn(12, 12, generator=g) * (9.0 if seed % 2 else 0.9)
        boxes = torch.rand(32, 4, generator=g)
        scores = torch.sigmoid(torch.randn(32, 1, generator=g) * 1.5 - 2.5)
        return boxes, scores, low

    @staticmethod
    def _cue_text(key, q):
        s = zlib.crc32(repr(("cue", key, q)).encode())
        return f"The object is most likely to appear near the {_WORDS[s % 8]} {_WORDS[(s >> 8) % 8]} {s % 97}."

    # ---- the box entries (stream; also the detection crops of the per-sample loop) ----
    def inference_boxes(self, boxes, question, mode="detection", upsample=False, slots=None, **kw):
        qs = [question] * len(boxes) if isinstance(question, str) else list(question)
        sl = [0] * len(boxes) if slots is None else list(slots)
        assert len(boxes) <= self.cfg.max_batch * 2
        keys = [self._crop_key(s, b) for s, b in zip(sl, boxes)]
        (self.seg_calls if mode == "segmentation" else self.calls).append(
            [(self._key(self.images[s]), tuple(int(v) for v in b), q) for s, b, q in zip(sl, boxes, qs)])
        recs = [self._record(k, q) for k, q in zip(keys, qs)]
        return [r[2] for r in recs] if mode == "segmentation" else recs

    def generate_boxes(self, boxes, questions, slots=None, max_new_tokens=100):
        if self.fail_cue:
            raise RuntimeError("cue decode failure")
        qs = [questions] * len(boxes) if isinstance(questions, str) else list(questions)
        sl = [0] * len(boxes) if slots is None else list(slots)
        self.gen_calls.append([(self._key(self.images[s]), tuple(int(v) for v in b), q) for s, b, q in zip(sl, boxes, qs)])
        return [self._cue_text(self._crop_key(s, b), q) for s, b, q in zip(sl, boxes, qs)]

    # ---- the host-crop entries (the per-sample loop's two calls) ----
    def inference(self, image, question, mode="segmentation"):
        assert mode == "vqa"
        self.solo_cue.append(question)
        return self._cue_text(self._key(image), question)

    def inference_batch(self, images, question, mode="detection", upsample=True, **kw):
        assert mode == "segmentation" and not upsample and len(images) == 1
        self.solo_seg.append(question)
        return [self._record(self._key(images[0]), question)[2]]

    # ---- heat maps ----
    def upsample_heatmap(self, low, h, w):
        return torch.clamp(torch.nn.functional.interpolate(low[None, None], (h, w), mode="bilinear", align_corners=False)[0, 0], min=0)

    def _stats(self, low, h, w, rects):
        H = self.upsample_heatmap(torch.as_tensor(np.asarray(low)), h, w).double().numpy()
        return np.asarray([H.min(), H.max(), H.sum()] + [H[y:y + rh, x:x + rw].sum() for x, y, rw, rh in (rects or [])], np.float64)

    def heatmap_stats(self, low, h, w, rects=None):
        return self._stats(low, h, w, rects)

    def heatmap_stats_batch(self, items):
        return [self._stats(*it) for it in items]


class _NoGenerateVSM(_CueVSM):
    def __getattribute__(self, name):          # a stand-in WITHOUT the batched entry: hasattr() must say so
        if name == "generate_boxes":
            raise AttributeError(name)
        return super().__getattribute__(name)


def _samples(n_images=5, per_image=(1, 2, 1, 3, 1), seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_images):
        w, h = int(rng.integers(600, 1300)), int(rng.integers(500, 900))
        img = synthetic_image(w, h, 50 + k)
        for t in range(per_image[k % len(per_image)]):
            out.append((img, f"thing {k}-{t}", None, search.smallest_size_for(w, h, 4.0, 64)))
    return out


_THRESHOLDS = {
    "always": dict(target_cue_threshold=1e9, target_cue_threshold_minimum=1e9),
    "half": dict(target_cue_threshold=10.0, target_cue_threshold_decay=1.0, target_cue_threshold_minimum=10.0),
}
_LOOP = {}


def _kw(which):
    return dict(confidence_high=0.9, confidence_low=0.0, noun_chunker=lambda p: [p.strip()], **_THRESHOLDS[which])


def _loop(which):
    """The yardstick, once per threshold setting: visual_search per sample, its paths and its call log."""
    if which not in _LOOP:
        vsm, res, paths = _CueVSM(max_batch=8), [], []
        for img, name, gt, sm in _samples():
            st = {}
            res.append(search.visual_search(vsm, img, name, gt, sm, speculate=False, stats=st, **_kw(which)))
            paths.append(st["search_path"])
        _LOOP[which] = (res, paths, vsm)
    return _LOOP[which]


def _same(loop, paths, got, st):
    assert len(got) == len(loop)
    for a, b in zip(loop, got):
        assert a[1] == b[1] and a[2] == b[2] and a[0]["bbox"] == b[0]["bbox"]
        assert torch.equal(a[0]["detection_result"], b[0]["detection_result"])
    assert st["context_cues"] == [[p.get("context_cue") for p in path] for path in paths]
    assert st["visit_orders"] == [[tuple(int(v) for v in p["bbox"]) for p in path] for path in paths]


@pytest.mark.parametrize("which", ["always", "half"])
@pytest.mark.parametrize("window", [1, 3, 8])
def test_stream_batches_the_cue_branch_and_equals_the_loop(window, which):
    loop, paths, loop_vsm = _loop(which)
    n_cues = sum("context_cue" in p for path in paths for p in path)
    n_expanded = sum("heat_stats" in p for path in paths for p in path)
    assert len(loop_vsm.solo_cue) == len(loop_vsm.solo_seg) == n_cues > 0
    if which == "always":
        assert n_cues == n_expanded
    else:
        assert 0.2 < n_cues / n_expanded < 0.8
    # the phrase, and with it the follow-up question, differs from node to node
    assert len(set(loop_vsm.solo_seg)) > n_cues // 2
    vsm, st = _CueVSM(max_batch=8), {"keep_paths": True}
    got = search.visual_search_stream(vsm, _samples(), window=window, stats=st, **_kw(which))
    _same(loop, paths, got, st)
    assert not vsm.solo_cue and not vsm.solo_seg                      # nothing went through the per-sample calls
    assert st["cue_requests"] == st["seg_requests"] == n_cues
    assert st["cue_calls"] == len(vsm.gen_calls) and st["seg_calls"] == len(vsm.seg_calls)
    assert sum(len(c) for c in vsm.gen_calls) == n_cues == sum(len(c) for c in vsm.seg_calls)
    assert st["cue_batch_max"] == max(len(c) for c in vsm.gen_calls)
    # the same follow-up questions were asked, about the same crops
    assert sorted(q for c in vsm.seg_calls for _, _, q in c) == sorted(loop_vsm.solo_seg)
    if window >= 3:
        assert st["cue_calls"] < st["cue_requests"] and st["seg_calls"] < st["seg_requests"]
        assert any(len({img for img, _, _ in c}) > 1 for c in vsm.gen_calls)      # crops of different images in one decode
        assert st["cue_batch_max"] > 1
    else:
        assert st["cue_calls"] == st["cue_requests"] and st["seg_calls"] == st["seg_requests"]


@pytest.mark.parametrize("make", [lambda: (_CueVSM(max_batch=8), False), lambda: (_NoGenerateVSM(max_batch=8), True)],
                         ids=["cue_batch_off", "no_generate_boxes"])
def test_request_by_request_serving_gives_the_same_results(make):
    loop, paths, _ = _loop("always")
    (vsm, cue_batch), st = make(), {"keep_paths": True}
    got = search.visual_search_stream(vsm, _samples(), window=8, stats=st, cue_batch=cue_batch, **_kw("always"))
    _same(loop, paths, got, st)
    n_cues = sum("context_cue" in p for path in paths for p in path)
    assert st["cue_requests"] == st["cue_calls"] == n_cues == st["seg_requests"] == st["seg_calls"]
    assert len(vsm.solo_cue) == len(vsm.solo_seg) == n_cues and not vsm.gen_calls and not vsm.seg_calls


def test_many_targets_on_one_image_batch_their_cues():
    img = synthetic_image(1100, 700, 5)
    names = ["kite", "red umbrella", "dog", "traffic light"]
    kw = _kw("always")
    solo = _CueVSM(max_batch=8)
    loop = [search.visual_search(solo, img, n, None, 175, speculate=False, **kw) for n in names]
    vsm, st = _CueVSM(max_batch=8), {}
    many = search.visual_search_many(vsm, img, names, None, 175, stats=st, speculate=False, **kw)
    for a, b in zip(loop, many):
        assert a[1] == b[1] and a[2] == b[2] and a[0]["bbox"] == b[0]["bbox"]
        assert torch.equal(a[0]["detection_result"], b[0]["detection_result"])
    assert st["cue_requests"] == len(solo.solo_cue) and st["cue_calls"] < st["cue_requests"]
    assert len(vsm.gen_calls[0]) == len(names)


def test_a_failing_cue_decode_reaches_the_caller():
    vsm = _CueVSM(max_batch=8, fail_cue=True)
    with pytest.raises(RuntimeError, match="cue decode failure"):
        search.visual_search_stream(vsm, _samples(), window=4, **_kw("always"))


def test_header_binding_and_export_list_agree_on_the_batched_entry():
    src = open(os.path.join(ROOT, "include", "vstar_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+vstar_vsm_generate_batch\s*\(([^)]*)\)", code)
    assert m, "include/vstar_hip.h does not declare vstar_vsm_generate_batch"
    n_params = len([p for p in m.group(1).split(",") if p.strip()])
    assert "vstar_vsm_generate_batch" in _lib.EXPORTS
    assert int(re.search(r"#define\s+VSTAR_GEN_MAX_BATCH\s+(\d+)", code).group(1)) == _lib.GEN_MAX_BATCH == 16
    lib = _lib.load()
    fn = lib.vstar_vsm_generate_batch
    assert len(fn.argtypes) == n_params == 10 and fn.restype is _lib.c_int
