"""The stream driver's engine calls, pinned: tests/golden/stream_call_trace.json holds, per configuration, a digest of every call the
stand-in engines of tests/test_search.py and tests/test_cue_stream.py logged (order, arguments, batch composition), their upload and
statistics-call lists, and a digest of the driver's statistics.  `python tests/test_search_trace.py --write` records the fixture
(it was recorded on the commit before the driver was split into _ImageSlots / _pack_step / request types); the test re-records and
compares.  CPU only.  Also here: the unit tests of `_pack_step` and of the request dispatch."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402

from tests import test_cue_stream as TC  # noqa: E402
from tests import test_search as TS  # noqa: E402
from vstar_amd import search  # noqa: E402
from vstar_amd.synthetic import synthetic_image  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "stream_call_trace.json")
LOGS = ("calls", "gen_calls", "seg_calls")                 # stored as one digest per call
LISTS = ("uploads", "stat_calls")                          # stored literally
STAT_KEYS = ("searches", "crops_scored", "useful_crops", "engine_steps", "cue_requests", "cue_calls", "cue_batch_max", "seg_requests",
             "seg_calls", "visit_orders", "context_cues")
_NO_CUE = dict(confidence_low=0.0, target_cue_threshold=-1.0, target_cue_threshold_minimum=-1.0)


def _digest(obj) -> str:
    return hashlib.sha1(repr(obj).encode()).hexdigest()[:12]


class _TwoRankSlotVSM(TS._SlotVSM):
    """Claims a world of two ranks: the refill then blocks on a prefetched image, so the trace does not depend on thread timing."""

    def _dist(self):
        return 2, 0


class _TwoRankAsyncVSM(TS._AsyncSlotVSM):
    def _dist(self):
        return 2, 0


class _Loader:
    def __init__(self, k, img):
        self.key, self.img = ("file", k), img

    def __call__(self):
        return self.img


def _loader_samples():
    """Zero-argument loaders; the samples of one image share one loader."""
    by_img, out = {}, []
    for img, name, gt, sm in TS._stream_samples(n_images=6, per_image=(1, 2)):
        out.append((by_img.setdefault(id(img), _Loader(len(by_img), img)), name, gt, sm))
    return out


def _configs():
    """(name, function returning (vsm, stats)) for every pinned configuration."""
    def stream(make_vsm, samples, **kw):
        def run():
            vsm, st = make_vsm(), {"keep_paths": True}
            search.visual_search_stream(vsm, samples(), stats=st, **kw)
            return vsm, st
        return run

    def slots(n, **kw):
        def make():
            vsm = TS._SlotVSM(**kw)
            vsm.max_image_slots = n
            return vsm
        return make

    out = []
    for window, conf in [(1, .9), (3, .9), (8, .9), (8, 2.0), (4, .6)]:
        out.append((f"stream-w{window}-c{conf}", stream(lambda: TS._SlotVSM(max_batch=8), TS._stream_samples, window=window, prefetch=0,
                                                        confidence_high=conf, **_NO_CUE)))
    out.append(("stream-7-images-2-slots", stream(slots(2, max_batch=8), lambda: TS._stream_samples(n_images=7, per_image=(1,)),
                                                  window=6, prefetch=0, confidence_high=0.9, **_NO_CUE)))
    for which in ("always", "half"):
        for window in (1, 3, 8):
            out.append((f"cue-{which}-w{window}", stream(lambda: TC._CueVSM(max_batch=8), TC._samples, window=window, prefetch=0,
                                                         **TC._kw(which))))
    for spec in (False, True):
        def many(spec=spec):
            vsm, st = TS._BoxVSMStats(), {"keep_paths": True}
            img = synthetic_image(960, 640, 3)
            search.visual_search_many(vsm, img, ["kite", "red umbrella", "dog", "traffic light", "boat"], None,
                                      search.smallest_size_for(960, 640, 4.0), stats=st, batch_size=3, speculate=spec,
                                      confidence_high=0.97, **_NO_CUE)
            return vsm, st
        out.append((f"many-speculate-{spec}", many))

    def two_rank():
        vsm = _TwoRankSlotVSM(max_batch=4)
        vsm.max_image_slots = 3
        return vsm
    out.append(("loaders-prefetch-2", stream(two_rank, _loader_samples, window=3, prefetch=2, confidence_high=0.9, **_NO_CUE)))
    return out


def _async_loaders():
    """Asynchronous uploads into slots reserved ahead (blocking refill).  Which worker uploads first is a matter of timing, the slot
    each image gets is not: the uploads are compared as a sorted list of slots."""
    vsm, st = _TwoRankAsyncVSM(max_batch=4), {"keep_paths": True}
    vsm.max_image_slots = 4
    search.visual_search_stream(vsm, _loader_samples(), window=3, prefetch=2, stats=st, confidence_high=0.9, **_NO_CUE)
    vsm.uploads = sorted(vsm.uploads + [s for s, _ in vsm.async_uploads])
    assert st["async_uploads"] == len(vsm.async_uploads) > 0
    return vsm, st


def record():
    """{configuration: trace}, and {configuration: {log: [repr of each call]}} for the mismatch report."""
    trace, raw = {}, {}
    for name, run in _configs() + [("loaders-async-upload", _async_loaders)]:
        vsm, st = run()
        raw[name] = {log: [repr(c) for c in getattr(vsm, log)] for log in LOGS if hasattr(vsm, log)}
        trace[name] = {log: [_digest(c) for c in getattr(vsm, log)] for log in LOGS if hasattr(vsm, log)}
        trace[name].update({log: [int(v) for v in getattr(vsm, log)] for log in LISTS if hasattr(vsm, log)})
        trace[name]["stats"] = _digest([(k, st.get(k)) for k in STAT_KEYS])
    return trace, raw


def test_stream_call_trace_equals_the_recorded_one():
    want = json.load(open(FIXTURE))
    got, raw = record()
    assert sorted(got) == sorted(want)
    for name in want:
        for log in LOGS:
            a, b = want[name].get(log), got[name].get(log)
            if a != b:
                k = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                call = raw[name][log][k] if k < len(b) else "(no such call: %d recorded, %d now)" % (len(a), len(b))
                print(f"{name}: {log}[{k}] differs, now {call}")
                pytest.fail(f"{name}: {log}[{k}] is not the recorded call ({len(a)} recorded, {len(b)} now)")
        for log in LISTS + ("stats",):
            assert got[name].get(log) == want[name].get(log), f"{name}: {log}"


# ---------------- _pack_step ----------------
A, B = [0, 0, 10, 10], [5, 5, 10, 10]


def test_pack_step_groups_requests_for_one_crop_and_never_splits_them():
    assert search._pack_step([(0, A), (0, B), (0, A), (1, A), (0, A)], 2) == [[0, 2, 4], [1, 3]]


def test_pack_step_edges():
    assert search._pack_step([], 4) == []
    assert search._pack_step([(0, A), (0, B), (1, B)], 3) == [[0, 1, 2]]                 # exactly `cap` entries: one call
    assert search._pack_step([(2, A)] * 5, 2) == [[0, 1, 2, 3, 4]]                       # one crop, more requests than `cap`
    assert search._pack_step([(0, A), (1, A), (0, A), (1, A)], 8) == [[0, 2, 1, 3]]      # same box, different images: not merged
    assert search._pack_step([(0, A), (1, A), (0, A), (1, A)], 1) == [[0, 2], [1, 3]]


# ---------------- request kinds ----------------
def test_requests_are_types_and_an_unknown_one_raises():
    assert search.ScoreReq("scorer", [A]).boxes == [A] and search.StatsReq([1]).items == [1]
    assert search.CueReq(A, "q").question == search.SegReq(A, "q").question == "q"

    class Cue:
        def inference(self, image, question, mode):
            return (image.size, question, mode)

    img = synthetic_image(64, 48, 0)
    assert search._serve_one(Cue(), img, search.CueReq([0, 0, 20, 10], "where?")) == ((20, 10), "where?", "vqa")
    for bad in (("stats", []), ("score", None, [A]), None, "cue"):
        with pytest.raises(TypeError):
            search._serve_one(Cue(), img, bad)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_search_trace.py --write")
    with open(FIXTURE, "w") as f:
        json.dump(record()[0], f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(FIXTURE, ROOT))
