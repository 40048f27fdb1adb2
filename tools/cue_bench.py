"""Contextual-cue text generation (VSM.inference mode='vqa', visual_search.py:427-443) at the 7B geometry.  Prints one JSON object.

Default: KV-cached decode (vstar_vsm_generate) vs the reference's literal schedule (one full prefill per new token).

--batch 1,2,4,8,16: the batched decode (vstar_vsm_generate_batch, n sequences in one device-resident loop) against n sequential
vstar_vsm_generate calls on the same pixels and prompts, both in this process, in alternated blocks; medians of tokens/s over the
whole call (towers and prefill included) and of ms per decode step (the call's time minus the time of the same call with one new
token, over the remaining steps).  The token lists of the two paths are compared as well.  VSTAR_DECODE_SPLIT_KV=0 in the
environment gives the un-split attention on both sides (a process reads it once)."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vstar_amd import preprocess as pp  # noqa: E402
from vstar_amd.config import VSMConfig  # noqa: E402
from vstar_amd.vsm import VSM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="", help="comma-separated batch sizes (<= 16) for the batched-vs-sequential comparison")
ap.add_argument("--new", type=int, default=int(os.environ.get("N_NEW", "100")), help="new tokens per sequence")
ap.add_argument("--reps", type=int, default=3, help="alternated blocks per batch size")
ap.add_argument("--layers", type=int, default=0, help="LLaMA layers (0: the 7B model's 32)")
ap.add_argument("--out", default="", help="also write the JSON here")
args = ap.parse_args()
n_new = args.new
batches = [int(b) for b in args.batch.split(",") if b]

geo = dict(llm_layers=args.layers) if args.layers else {}
cfg = VSMConfig.seal_7b(224, max_batch=max(batches + [1]), max_text_len=256, **geo)
vsm = VSM(SimpleNamespace(version="synthetic", vision_tower="synthetic", conv_type="llava_v1", use_mm_start_end=True,
                          model_max_length=512), cfg=cfg, synthetic_seed=0)
vsm.vsm_tokenizer.eos_token_id = -1       # random weights: never stop early, time exactly n_new tokens
rng = np.random.default_rng(0)


def emit(out):
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if not batches:
    img = Image.fromarray(rng.integers(0, 256, (600, 800, 3), dtype=np.uint8))
    q = pp.CUE_QUESTION.format("red umbrella")
    out = {"new_tokens": n_new, "prompt_rows": None}
    for name, uc, n in (("kv_cached", True, n_new), ("no_cache_reference_schedule", False, min(n_new, 20))):
        vsm.generate_ids(img, q, max_new_tokens=2, use_cache=uc)
        t0 = time.time()
        ids = vsm.generate_ids(img, q, max_new_tokens=n, use_cache=uc)
        dt = time.time() - t0
        assert len(ids) == n
        out[name] = {"tokens": n, "seconds": round(dt, 3), "ms_per_token": round(dt / n * 1e3, 2)}
    out["speedup_per_token"] = round(out["no_cache_reference_schedule"]["ms_per_token"] / out["kv_cached"]["ms_per_token"], 2)
    emit(out)
    sys.exit(0)

names = ["kite", "red umbrella", "small brown dog", "traffic light on the pole", "cup of coffee", "old wooden boat near the pier"]
N = max(batches)
imgs = [Image.fromarray(rng.integers(0, 256, (300 + 37 * i, 400 + 53 * i, 3), dtype=np.uint8)) for i in range(N)]
clip = torch.from_numpy(np.stack([pp.clip_preprocess(im, cfg.clip_image_size) for im in imgs])).bfloat16()
prompts = [pp.tokenizer_image_token(pp.build_prompt(pp.CUE_QUESTION.format(names[i % len(names)])), vsm.vsm_tokenizer) for i in range(N)]
eng = vsm.engine


def batched(n, new):
    t0 = time.perf_counter()
    toks = eng.generate_batch(clip[:n], prompts[:n], new, -1)          # returns after the stream is drained
    return time.perf_counter() - t0, toks


def sequential(n, new):
    t0 = time.perf_counter()
    toks = [eng.generate(clip[i:i + 1], prompts[i], new, -1) for i in range(n)]
    return time.perf_counter() - t0, toks


out = {"new_tokens": n_new, "reps": args.reps, "llm_layers": cfg.llm_layers, "split_kv_env": os.environ.get("VSTAR_DECODE_SPLIT_KV", "(unset: on)"),
       "batches": {}}
for n in batches:
    batched(n, 2), sequential(n, 2)                                    # builds the runners and the graph of this n
    tb, ts, tb1, ts1, same, path = [], [], [], [], True, -1
    for _ in range(args.reps):                                         # alternated blocks
        dt, a = batched(n, n_new)
        tb.append(dt)
        path = eng.gen_attn_path()
        dt, b = sequential(n, n_new)
        ts.append(dt)
        tb1.append(batched(n, 1)[0])
        ts1.append(sequential(n, 1)[0])
        same = same and a == b and all(len(x) == n_new for x in a)
    mb, ms, mb1, ms1 = (statistics.median(x) for x in (tb, ts, tb1, ts1))
    steps = max(n_new - 1, 1)
    out["batches"][str(n)] = {
        "attention_path": path,                                        # 2: split-KV pair, 1: one fused kernel per (row, head)
        "tokens_equal": same,
        "batched": {"seconds": round(mb, 4), "tokens_per_s": round(n * n_new / mb, 1), "ms_per_step": round((mb - mb1) / steps * 1e3, 3),
                    "prefill_seconds": round(mb1, 4), "seconds_all": [round(x, 4) for x in tb]},
        "sequential": {"seconds": round(ms, 4), "tokens_per_s": round(n * n_new / ms, 1),
                       "ms_per_step": round((ms - ms1) / steps / n * 1e3, 3), "prefill_seconds": round(ms1, 4),
                       "seconds_all": [round(x, 4) for x in ts]},
        "speedup_tokens_per_s": round(ms / mb, 2),
    }
emit(out)
