"""A stream of synthetic (image, target) searches at the 7B geometry WITH the contextual-cue branch: the cue threshold sits at the
median of the heat-map maxima observed in an untimed pass, so that about half of the expanded nodes take the branch.  Compares
visual_search_stream(cue_batch=True) — one batched decode and one scoring step per round for all live searches — with
cue_batch=False (one KV-cached decode and one one-crop step per cue, the per-sample loop's calls), alternated in this process.
Prints one JSON object: searches/s, cue_calls, cue_requests and the share of wall time spent generating, medians over --reps.

Synthetic weights: how often a real checkpoint takes the branch is not known here; this measures the cost of a cue, not its rate."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vstar_amd.config import VSMConfig  # noqa: E402
from vstar_amd.search import smallest_size_for, visual_search_stream  # noqa: E402
from vstar_amd.synthetic import synthetic_image  # noqa: E402
from vstar_amd.vsm import VSM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--targets-per-image", type=int, default=2)
ap.add_argument("--window", type=int, default=16)
ap.add_argument("--image", default="1920x1080")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--layers", type=int, default=0, help="LLaMA layers (0: the 7B model's 32)")
ap.add_argument("--out", default="")
args = ap.parse_args()
W, H = (int(v) for v in args.image.split("x"))

geo = dict(llm_layers=args.layers) if args.layers else {}
cfg = VSMConfig.seal_7b(224, max_batch=32, max_text_len=192, **geo)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    vsm = VSM(SimpleNamespace(version="synthetic", vision_tower="synthetic", conv_type="llava_v1", use_mm_start_end=True,
                              model_max_length=512), cfg=cfg, synthetic_seed=0, strict_template=False)
vsm.group_prompts = False                      # plain batches on both sides
smallest = smallest_size_for(W, H, 4.0)
n_img = max(args.samples // args.targets_per_image, 1)
images = [synthetic_image(W, H, 3000 + k) for k in range(n_img)]
samples = [(images[k], f"object {t}", None, smallest) for k in range(n_img) for t in range(args.targets_per_image)]
base = dict(confidence_high=2.0, confidence_low=0.0, speculate=False, window=args.window)      # exhaustive trees: the same work every run

# ---- untimed pass without the branch: the maxima of the heat maps the searches look at ----
maxima = []
inner = vsm.heatmap_stats_batch


def spy(items):
    res = inner(items)
    maxima.extend(float(r[1]) for r in res)
    return res


vsm.heatmap_stats_batch = spy
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    visual_search_stream(vsm, samples, target_cue_threshold=-1.0, target_cue_threshold_minimum=-1.0, **base)
vsm.heatmap_stats_batch = inner
thr = float(np.median(np.asarray(maxima)))
cue_kw = dict(target_cue_threshold=thr, target_cue_threshold_decay=1.0, target_cue_threshold_minimum=thr)

# cue_batch=False decodes through VSM.generate, which keeps no timer of its own
solo_gen = {"s": 0.0}
plain_generate = vsm.generate


def timed_generate(*a, **k):
    t0 = time.perf_counter()
    try:
        return plain_generate(*a, **k)
    finally:
        solo_gen["s"] += time.perf_counter() - t0


vsm.generate = timed_generate


def run(cue_batch):
    for k in vsm.timers:
        vsm.timers[k] = 0
    solo_gen["s"] = 0.0
    st = {}
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = visual_search_stream(vsm, samples, stats=st, cue_batch=cue_batch, **cue_kw, **base)
    dt = time.perf_counter() - t0
    gen_s = float(vsm.timers["generate_s"]) + solo_gen["s"]
    sig = [(r[1], r[2], tuple(r[0]["bbox"])) for r in res]
    return dict(seconds=dt, searches_per_s=len(samples) / dt, cue_requests=st["cue_requests"], cue_calls=st["cue_calls"],
                cue_batch_max=st["cue_batch_max"], seg_requests=st["seg_requests"], seg_calls=st["seg_calls"],
                crops_scored=st["crops_scored"], generate_s=gen_s, generate_share=gen_s / dt), sig


run(True), run(False)                           # warm-up of both paths (runners, graphs)
legs = {True: [], False: []}
same = True
for _ in range(args.reps):                      # alternated
    a, sa = run(True)
    b, sb = run(False)
    legs[True].append(a)
    legs[False].append(b)
    same = same and sa == sb


def med(rows):
    return {k: (round(statistics.median(r[k] for r in rows), 4) if isinstance(rows[0][k], float) else rows[0][k]) for k in rows[0]}


out = {"image": args.image, "samples": len(samples), "window": args.window, "llm_layers": cfg.llm_layers, "cue_threshold": round(thr, 4),
       "heat_map_maxima_seen": len(maxima), "reps": args.reps, "same_results": same,
       "cue_batch_true": med(legs[True]), "cue_batch_false": med(legs[False])}
out["speedup_searches_per_s"] = round(out["cue_batch_true"]["searches_per_s"] / out["cue_batch_false"]["searches_per_s"], 3)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
