"""Micro-benchmark of the VQA-LLM engine at the 7B geometry (seeded random fp16 weights): image encoding, prefill,
KV-cached decode steps at several batch sizes, forked option scoring.  Prints one JSON object.

  python tools/vqa_bench.py [--out profiles/r01_vqa_bench.json] [--layers 32] [--sample]
--logprobs 0,5 runs `decode_logprobs` alone: greedy decode steps without and with the on-device log-probability stage (logprobs=0 /
logprobs=5), alternated in blocks of --steps at the --batches sizes, and each mode's tokens/s over the plain one's.
--contrast 4,8 runs `decode_contrast` alone: contrastive-search steps of one prompt with k candidates (forward_contrast_step: k forked
one-row sequences, the penalty / select / adopt kernels) alternated in blocks of --steps with greedy one-row steps of
the same prompt in the same process; tokens/s of both (one token per step either way) and their ratio.  Written to
profiles/vqa_contrast_bench.json unless --out says otherwise.
--guidance (alone): `decode_guidance` — guided decode steps against greedy steps at the same and at twice the batch.
--guide-kernels P (alone, under `rocprofv3 --kernel-trace --stats -- python tools/vqa_bench.py --guide-kernels P`): the guidance kernel
on P pairs next to the beam select on P rows.
--sample adds `decode_sample`: greedy and sampled decode steps (temperature 0.7, top_k 50, top_p 0.9: every pass of the
sampling kernel) alternated in blocks of --steps at the same batch sizes, and the sampled / greedy tokens/s ratio; with --warp a
third kind of block, the sampled step with min_p 0.05 and typical_p 0.9, and its cost over the plain sampled step.
--beams 1,2,4,8 adds `decode_beams`: beam-search steps of one prompt with k beams (forward_beam's select tail, the host scorer,
the KV ancestry reorder) alternated with greedy steps of k copies of the same prompt, and the beam / greedy step-time ratio.
--score 1,4,8,16 adds `score`: multiple-choice scoring of B questions (~300 cached rows, 4 options x 12 tokens) through
`VQA_LLM.multiple_choices_batch` (two engine calls, the losses reduced by the on-device scoring tail) alternated
in blocks with a loop of `VQA_LLM.option_losses` (one question at a time, logits to the host), questions/s of both and the
spread of the alternated blocks.  --only-score skips every other leg.
--score-kernels N (use with --layers 2 under `rocprofv3 --kernel-trace --stats -- python tools/vqa_bench.py ...`): 20 forward
calls with the arg-max tail and 20 with the scoring tail on N wanted rows, so that the trace's per-kernel statistics compare
score_rows_kernel with argmax_rows at that row count.
--decode-bits 0,8 or 0,8,4 runs `decode_bits` ALONE: one engine per mode in one process on the same weights — fp16, the int8
weight-only decode mode and the int4 group-scaled mode (§8.6) — greedy decode blocks of --steps alternated
--rounds times at every batch size; tokens/s and the effective weight stream of each (bytes a step actually reads: the quantised
block linears with their scales + the fp16 lm_head), the ratios against fp16 (and 4-bit against 8-bit) and the spread over the
rounds.  The yardsticks of the 4-bit mode are the same process's fp16 and 8-bit engines.
--kv-bits 0,8 runs `decode_kv` ALONE: for every weight mode of --decode-bits (default 0 alone) two engines in one
process on the same weights — the fp16 KV cache and the block-scaled fp8 cache — greedy decode blocks of --steps alternated --rounds
times at every batch size, each sequence holding --ctx cached positions (700: an image, a prompt and an answer; 1800: near the 2048
context); tokens/s of both (median over the blocks), their ratio, the spread, and the K/V bytes a step reads in each format.
--spec 1,3,6 runs `decode_spec` ALONE: one sequence (~300 cached positions), first a plain greedy decode of
--spec-tokens tokens, then for every draft length d and every share of corrupted draft positions in --spec-corrupt (a replay
drafter proposing that output: 1.0 = acceptance 0, 0.0 = acceptance 1) `VQA_LLM.speculative_decode` blocks alternated --rounds
times with `greedy_decode` blocks of the same process; tokens/s of both (median over the blocks), their ratio, the spread of the
blocks, the acceptance counters, and the device time of a verify step against its row count (1 .. 16 rows).
--rules: one engine, greedy decode steps with logits rules (repetition penalty + bigram ban over --ctx history tokens, DESIGN.md
§8.8) alternated with plain steps in blocks of --steps; device and wall ms per step of both and the host planning time.
--spec-kernels R (under `rocprofv3 --kernel-trace --stats -- python tools/vqa_bench.py --layers 2 --spec-kernels R`): 20 one-sequence
steps of R rows with the arg-max tail on R wanted rows and 20 with the greedy and the sampled verify tail, for the per-kernel
statistics of the verify kernels against argmax_rows_lp.
Decode steps are bound by the weight sweep (13.5 GB fp16 per step at 7B): `weights_GBps` = bytes of all LLaMA + lm_head
weights / device time of one step (HIP events inside the engine), against the ~8 TB/s HBM3E peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vstar_amd.config import VQAConfig  # noqa: E402
from vstar_amd.vqa import sampling_params  # noqa: E402
from vstar_amd.vqa_engine import Seq, VqaEngine  # noqa: E402
from vstar_amd.weights import random_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,4,16,32")
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--sample", action="store_true", help="add the sampled-decode leg next to greedy")
    ap.add_argument("--warp", action="store_true", help="--sample: add sampled blocks with min_p=0.05 and typical_p=0.9 (DESIGN.md §8.10)")
    ap.add_argument("--rounds", type=int, default=3, help="--sample / --beams: blocks alternated this many times")
    ap.add_argument("--beams", default="", help="comma-separated beam counts: add the beam-search leg next to greedy")
    ap.add_argument("--score", default="", help="comma-separated batch sizes: add the batched multiple-choice scoring leg")
    ap.add_argument("--only-score", action="store_true", help="run the --score leg alone")
    ap.add_argument("--decode-bits", default="", help="'0,8' or '0,8,4': fp16 against the int8 / int4 weight-only decode modes, alternated blocks (runs alone)")
    ap.add_argument("--kv-bits", default="", help="'0,8': the fp16 KV cache against the block-scaled fp8 cache, alternated blocks, crossed "
                    "with --decode-bits (runs alone)")
    ap.add_argument("--ctx", type=int, default=296, help="--kv-bits: cached positions per sequence when the decode blocks start")
    ap.add_argument("--spec", default="", help="comma-separated draft lengths: speculative against plain greedy decode (runs alone)")
    ap.add_argument("--spec-tokens", type=int, default=64, help="--spec: tokens decoded per block")
    ap.add_argument("--spec-corrupt", default="1.0,0.5,0.0", help="--spec: shares of corrupted draft positions")
    ap.add_argument("--rules", action="store_true", help="greedy decode steps with logits rules (repetition penalty + bigram ban over --ctx "
                    "history tokens) against plain ones, alternated blocks (runs alone)")
    ap.add_argument("--logprobs", default="", help="comma-separated n (e.g. '0,5'): greedy decode steps without and with the on-device "
                    "log-probability stage asking for n alternatives, alternated blocks (DESIGN.md 8.9; runs alone)")
    ap.add_argument("--contrast", default="", help="comma-separated candidate counts (e.g. '4,8'): contrastive-search steps against greedy "
                    "steps of the same process, alternated blocks (DESIGN.md 8.11; runs alone; default --out profiles/vqa_contrast_bench.json)")
    ap.add_argument("--guidance", action="store_true", help="guided decode steps (guidance_scale 1.5 against the image-free prompt, DESIGN.md "
                    "8.12) against greedy steps at the same batch and at twice the batch, alternated blocks (runs alone; default --out "
                    "profiles/vqa_guide_bench.json)")
    ap.add_argument("--guide-kernels", type=int, default=0, help="pairs: the guidance kernel on that many pairs of vocab-32001 rows and the "
                    "beam select on as many rows, 20 launches each, for a kernel trace (no engine is built)")
    ap.add_argument("--spec-kernels", type=int, default=0, help="rows: the arg-max and verify tails alone, for a kernel trace")
    ap.add_argument("--score-kernels", type=int, default=0, help="rows: the arg-max and scoring tails alone, for a kernel trace")
    a = ap.parse_args()
    score_b = [int(x) for x in a.score.split(",")] if a.score else []
    if a.only_score and not score_b:
        ap.error("--only-score needs --score B[,B...]")
    if a.guide_kernels:
        print(json.dumps({"guide_kernels": guide_kernels(a.guide_kernels)}))
        return
    if a.rules:
        out = {"decode_rules": decode_rules(a.layers, [int(x) for x in a.batches.split(",")], a.steps, a.rounds, a.ctx)}
        return finish(out, a)
    if a.kv_bits:
        if [int(x) for x in a.kv_bits.split(",")] != [0, 8]:
            ap.error("--kv-bits takes 0,8")
        wbits = [int(x) for x in a.decode_bits.split(",")] if a.decode_bits else [0]
        if not set(wbits) <= {0, 4, 8}:
            ap.error("--decode-bits takes 0, 8 and 4")
        out = {"decode_kv": decode_kv(a.layers, [int(x) for x in a.batches.split(",")], a.steps, a.rounds, wbits, a.ctx)}
        return finish(out, a)
    if a.decode_bits:
        bits = [int(x) for x in a.decode_bits.split(",")]
        if bits[0] != 0 or len(set(bits)) != len(bits) or not set(bits) <= {0, 4, 8} or len(bits) < 2:
            ap.error("--decode-bits takes 0 followed by 8, 4 or both")
        out = {"decode_bits": decode_bits(a.layers, [int(x) for x in a.batches.split(",")], a.steps, a.rounds, bits)}
        return finish(out, a)
    if a.spec or a.spec_kernels:
        out = decode_spec(a.layers, [int(x) for x in a.spec.split(",")] if a.spec else [], a.spec_tokens,
                          [float(x) for x in a.spec_corrupt.split(",")], a.rounds, a.spec_kernels)
        return finish(out, a)
    n_q = max(score_b + [1])                     # the scoring leg needs 5 KV slots and one feature slot per question
    cfg = VQAConfig.seal_7b(llm_layers=a.layers, max_slots=max(40, 5 * n_q), max_ctx=1024, max_rows=16384, max_images=max(8, n_q))
    t0 = time.time()
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, 0, torch.float16, share_layers=True))
    load_s = time.time() - t0
    H, M, V, L = cfg.llm_hidden, cfg.llm_mlp, cfg.llm_vocab, cfg.llm_layers
    wbytes = 2.0 * (L * (4 * H * H + 3 * H * M) + V * H)
    out = {"config": {"layers": L, "hidden": H, "vocab": V, "weights_GB": round(wbytes / 1e9, 2)}, "weights_load_s": round(load_s, 1)}
    if a.score_kernels:
        out["score_kernels"] = score_kernels(eng, cfg, a.score_kernels)
        print(json.dumps(out))
        return
    if a.only_score:
        out["score"] = score_leg(eng, cfg, score_b, a.rounds)
        return finish(out, a)
    g = torch.Generator().manual_seed(0)
    pix = torch.randn(3, 3, 224, 224, generator=g)
    eng.encode_images(pix, 0)
    t0 = time.time()
    for _ in range(3):
        eng.encode_images(pix, 0)
    out["encode_3_images_ms"] = round((time.time() - t0) / 3 * 1e3, 2)
    # prompt: 40 text ids + 1 long image (256 rows) + 2 long objects (512 rows) = 808 rows (the <=2-objects case), or short
    text = torch.randint(3, 30000, (40,), generator=g).tolist()
    long_rows = text[:10] + eng.feature_rows(0, True) + text[10:25] + eng.feature_rows(1, True) + eng.feature_rows(2, True) + text[25:]
    short_rows = text[:10] + eng.feature_rows(0, False) + text[10:25] + eng.feature_rows(1, True) + eng.feature_rows(2, True) + text[25:]
    plain_rows = text[:10] + eng.feature_rows(0, True) + text[10:]
    if a.logprobs:
        out["decode_logprobs"] = decode_logprobs(eng, plain_rows, [int(x) for x in a.batches.split(",")], a.steps, a.rounds,
                                                 [int(x) for x in a.logprobs.split(",")])
        return finish(out, a)
    if a.guidance:
        neg_rows = text[:10] + text[10:]             # the same prompt without its image rows: the language prior
        out["decode_guidance"] = decode_guidance(eng, plain_rows, neg_rows, [b for b in (int(x) for x in a.batches.split(",")) if 2 * b <= cfg.max_slots],
                                                 a.steps, a.rounds)
        a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vqa_guide_bench.json")
        return finish(out, a)
    if a.contrast:
        out["decode_contrast"] = decode_contrast(eng, plain_rows, [int(x) for x in a.contrast.split(",")], a.steps, a.rounds)
        a.out = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vqa_contrast_bench.json")
        return finish(out, a)
    res = {}
    for name, rows in (("plain_296", plain_rows), ("objects_584", short_rows)):
        for B in (1, 8):
            seqs = [Seq(rows, kv_slot=i) for i in range(B)]
            eng.forward(seqs, [(i, -1) for i in range(B)], logits=False)
            ms = []
            for _ in range(3):
                eng.forward(seqs, [(i, -1) for i in range(B)], logits=False)
                ms.append(eng.last_forward_ms())
            S = len(rows)
            flops = 2.0 * B * S * (L * (4 * H * H + 3 * H * M)) + 2.0 * B * L * S * S * H
            res[f"prefill_{name}_B{B}"] = {"ms": round(min(ms), 3), "TFLOPs": round(flops / min(ms) / 1e9, 1),
                                           "rows": B * S}
    out["prefill"] = res
    # decode: B sequences with ~300 cached positions each
    dec = {}
    for B in [int(x) for x in a.batches.split(",")]:
        seqs = [Seq(plain_rows, kv_slot=i) for i in range(B)]
        _, nxt = eng.forward(seqs, [(i, -1) for i in range(B)], logits=False)
        pos = len(plain_rows)
        dev, t0 = [], time.time()
        for s in range(a.steps):
            _, nxt = eng.forward([Seq([int(nxt[i])], kv_slot=i, past_len=pos) for i in range(B)], [(i, 0) for i in range(B)],
                                 logits=False)
            dev.append(eng.last_forward_ms())
            pos += 1
        wall = (time.time() - t0) / a.steps * 1e3
        d = float(np.median(dev))
        dec[f"B{B}"] = {"device_ms_per_step": round(d, 3), "wall_ms_per_step": round(wall, 3),
                        "tokens_per_s": round(B / wall * 1e3, 1), "weights_GBps": round(wbytes / d / 1e6, 0)}
    out["decode"] = dec
    if a.sample:
        out["decode_sample"] = decode_sample(eng, plain_rows, [int(x) for x in a.batches.split(",")], a.steps, a.rounds, a.warp)
    if a.beams:
        out["decode_beams"] = decode_beams(eng, plain_rows, [int(x) for x in a.beams.split(",")], a.steps, a.rounds)
    # option scoring: 4 options x 12 tokens forked from one question prefix
    eng.forward([Seq(short_rows, kv_slot=0)], [(0, -1)])
    P = len(short_rows)
    opts = [torch.randint(3, 30000, (12,), generator=g).tolist() for _ in range(4)]
    ms = []
    for _ in range(4):
        eng.forward([Seq(o, kv_slot=1 + j, past_len=P, prefix_slot=0) for j, o in enumerate(opts)],
                    [(j, t) for j in range(4) for t in range(11)])
        ms.append(eng.last_forward_ms())
    out["option_scoring_4x12_ms"] = round(min(ms), 3)
    if score_b:
        out["score"] = score_leg(eng, cfg, score_b, a.rounds)
    finish(out, a)


def finish(out, a):
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


_FWD_MS = [0.0]


def score_leg(eng, cfg, batches, rounds):
    """Questions/s of multiple-choice scoring: `multiple_choices_batch` (device tail, B questions per call pair) vs a loop of
    today's `option_losses` (host logits), alternated `rounds` times; both include the same image encoding and tokenisation."""
    from PIL import Image
    from vstar_amd.vqa import VQA_LLM
    llm = VQA_LLM(cfg=cfg, engine=eng)
    for name in ("forward", "forward_score"):     # sum the engine's own forward time per block (wall time also holds CLIP + host work)
        def timed(*a, _f=getattr(eng, name), **kw):
            r = _f(*a, **kw)
            _FWD_MS[0] += eng.last_forward_ms()
            return r
        setattr(eng, name, timed)
    rng = np.random.default_rng(0)
    words = ["red", "blue", "green", "mug", "table", "left", "right", "small", "large", "near", "behind", "cup"]
    samples = []
    for i in range(max(batches)):
        opts = [" ".join(words[(i + 3 * j + t) % len(words)] for t in range(8)) for j in range(4)]      # 8 words + ': ' / '</s>' pieces
        samples.append(dict(image=Image.fromarray(rng.integers(0, 256, (336, 336, 3), dtype=np.uint8)),
                            question=f"What is the colour of the mug number {i} on the table", options=opts))
    res = {}
    for B in batches:
        sub = samples[:B]
        plan = llm.score_continuations_batch(sub[:1])
        run = {"device": lambda: llm.multiple_choices_batch(sub),
               "host": lambda: [int(torch.stack(llm.option_losses(s["image"], s["question"], s["options"])).argmin()) for s in sub]}
        picks = {m: f() for m, f in run.items()}            # warm-up, and the two paths' choices
        t = {"device": [], "host": []}
        fwd = {"device": [], "host": []}         # the LLM side alone: device time of the forward calls of a block (HIP events)
        for _ in range(rounds):
            for m in ("device", "host"):
                _FWD_MS[0] = 0.0
                t0 = time.time()
                run[m]()
                t[m].append(time.time() - t0)
                fwd[m].append(_FWD_MS[0])
        leg = {"option_tokens": [len(v) for v in plan[0]], "same_choices": picks["device"] == picks["host"]}
        for m in ("device", "host"):
            med = float(np.median(t[m]))
            leg[m] = {"questions_per_s": round(B / med, 2), "block_ms": [round(x * 1e3, 1) for x in t[m]],
                      "spread": round((max(t[m]) - min(t[m])) / med, 3),
                      "forward_device_ms_per_block": [round(x, 2) for x in fwd[m]]}
        leg["device_over_host_questions_per_s"] = round(leg["device"]["questions_per_s"] / leg["host"]["questions_per_s"], 3)
        res[f"B{B}"] = leg
    return res


def decode_bits(layers, batches, steps, rounds, modes=(0, 8)):
    """fp16 engine against the int8 / int4 weight-only decode engines (same seeded weights), greedy steps of B sequences with ~300
    cached positions, blocks of `steps` alternated `rounds` times in one process."""
    engs = {}
    for bits in modes:
        cfg = VQAConfig.seal_7b(llm_layers=layers, max_slots=max(batches + [1]), max_ctx=1024, max_rows=16384,
                                max_images=1).with_decode_bits(bits)
        engs[bits] = VqaEngine(cfg, 0)
        engs[bits].load_state_dict(random_state_dict(cfg, 0, torch.float16, share_layers=True))
        assert engs[bits].decode_weight_bits() == bits
    H, M, V, L = cfg.llm_hidden, cfg.llm_mlp, cfg.llm_vocab, cfg.llm_layers
    blk = L * (4 * H * H + 3 * H * M)
    # (8: one fp32 scale per packed row; 4: half a byte per weight + one fp16 scale per 128 of them = 4.125 bits)
    wbytes = {0: 2.0 * (blk + V * H), 8: 1.0 * blk + 4.0 * L * (5 * H + 2 * M) + 2.0 * V * H,
              4: (0.5 + 2.0 / 128) * blk + 2.0 * V * H}
    wbytes = {b: wbytes[b] for b in modes}
    g = torch.Generator().manual_seed(0)
    rows = torch.randint(3, 30000, (296,), generator=g).tolist()
    res = {"config": {"layers": L, "hidden": H, "weights_GB_per_step": {str(b): round(w / 1e9, 2) for b, w in wbytes.items()}}}
    for B in batches:
        nxt, pos = {}, {}
        for bits, eng in engs.items():
            _, nxt[bits] = eng.forward([Seq(rows, kv_slot=i) for i in range(B)], [(i, -1) for i in range(B)], logits=False)
            pos[bits] = len(rows)
        want = [(i, 0) for i in range(B)]
        dev = {b: [] for b in modes}
        blocks = {b: [] for b in modes}
        for r in range(rounds + 1):                  # round 0 warms both engines up and is dropped
            for bits, eng in engs.items():
                t0 = time.time()
                d = []
                for s in range(steps):
                    _, nxt[bits] = eng.forward([Seq([int(nxt[bits][i])], kv_slot=i, past_len=pos[bits]) for i in range(B)], want, logits=False)
                    d.append(eng.last_forward_ms())
                    pos[bits] += 1
                if r:
                    blocks[bits].append((time.time() - t0) / steps * 1e3)
                    dev[bits] += d
        leg = {}
        for bits in modes:
            w, d = float(np.median(blocks[bits])), float(np.median(dev[bits]))
            leg[f"bits{bits}"] = {"device_ms_per_step": round(d, 3), "wall_ms_per_step": round(w, 3), "tokens_per_s": round(B / w * 1e3, 1),
                                  "wall_ms_per_step_blocks": [round(x, 3) for x in blocks[bits]],
                                  "spread": round((max(blocks[bits]) - min(blocks[bits])) / w, 3),
                                  "weights_GBps": round(wbytes[bits] / d / 1e6, 0)}
        for x, y in ((8, 0), (4, 0), (4, 8)):
            if x in modes and y in modes:
                leg[f"bits{x}_over_bits{y}_tokens_per_s"] = round(leg[f"bits{x}"]["tokens_per_s"] / leg[f"bits{y}"]["tokens_per_s"], 3)
                leg[f"bits{x}_over_bits{y}_device_time"] = round(leg[f"bits{x}"]["device_ms_per_step"] / leg[f"bits{y}"]["device_ms_per_step"], 3)
        res[f"B{B}"] = leg
    return res


def decode_kv(layers, batches, steps, rounds, weight_modes, ctx):
    """The fp16 KV cache against the block-scaled fp8 cache per weight mode: two engines on the same seeded weights,
    greedy steps of B sequences with `ctx` cached positions each, blocks of `steps` alternated `rounds` times in one process (round 0
    warms up and is dropped); the engines of a weight mode are released before the next mode is built."""
    import gc
    res = {}
    B_max = max(batches + [1])
    max_ctx = (ctx + (rounds + 1) * steps * len(batches) + 64 + 63) // 64 * 64
    g = torch.Generator().manual_seed(0)
    rows = torch.randint(3, 30000, (ctx,), generator=g).tolist()
    for wb in weight_modes:
        engs = {}
        for kvb in (0, 8):
            cfg = VQAConfig.seal_7b(llm_layers=layers, max_slots=B_max, max_ctx=max_ctx, max_rows=max(16384, ctx * 8),
                                    max_images=1).with_decode_bits(wb).with_kv_bits(kvb)
            engs[kvb] = VqaEngine(cfg, 0)
            engs[kvb].load_state_dict(random_state_dict(cfg, 0, torch.float16, share_layers=True))
            assert engs[kvb].decode_weight_bits() == wb and engs[kvb].kv_cache_format() == (1 if kvb else 0)
        H, L = cfg.llm_hidden, cfg.llm_layers
        leg_w = {"config": {"layers": L, "hidden": H, "ctx": ctx, "max_ctx": max_ctx,
                            "kv_cache_GB": {str(k): round(e.kv_cache_bytes() / 1e9, 2) for k, e in engs.items()}}}
        for B in batches:
            nxt, pos = {}, {}
            for kvb, eng in engs.items():
                for i0 in range(0, B, 8):                     # prefill in chunks of 8 sequences (max_rows)
                    n = min(8, B - i0)
                    _, t = eng.forward([Seq(rows, kv_slot=i0 + i) for i in range(n)], [(i, -1) for i in range(n)], logits=False)
                    nxt[kvb] = t if i0 == 0 else np.concatenate([nxt[kvb], t])
                pos[kvb] = len(rows)
            want = [(i, 0) for i in range(B)]
            dev = {k: [] for k in engs}
            blocks = {k: [] for k in engs}
            for r in range(rounds + 1):
                for kvb, eng in engs.items():
                    t0 = time.time()
                    d = []
                    for s in range(steps):
                        _, nxt[kvb] = eng.forward([Seq([int(nxt[kvb][i])], kv_slot=i, past_len=pos[kvb]) for i in range(B)], want, logits=False)
                        d.append(eng.last_forward_ms())
                        pos[kvb] += 1
                    if r:
                        blocks[kvb].append((time.time() - t0) / steps * 1e3)
                        dev[kvb] += d
            leg = {"positions": [len(rows), pos[0]]}
            for kvb in engs:
                w, d = float(np.median(blocks[kvb])), float(np.median(dev[kvb]))
                per_row = 132 if kvb else 256                 # bytes of one cached row of K (or V)
                kv_gb = 2.0 * L * B * cfg.llm_heads * (len(rows) + pos[kvb]) / 2 * per_row / 1e9
                leg[f"kv{kvb}"] = {"device_ms_per_step": round(d, 3), "wall_ms_per_step": round(w, 3), "tokens_per_s": round(B / w * 1e3, 1),
                                   "wall_ms_per_step_blocks": [round(x, 3) for x in blocks[kvb]],
                                   "spread": round((max(blocks[kvb]) - min(blocks[kvb])) / w, 3), "kv_GB_per_step": round(kv_gb, 3)}
            leg["kv8_over_kv0_tokens_per_s"] = round(leg["kv8"]["tokens_per_s"] / leg["kv0"]["tokens_per_s"], 3)
            leg["kv8_over_kv0_device_time"] = round(leg["kv8"]["device_ms_per_step"] / leg["kv0"]["device_ms_per_step"], 3)
            leg_w[f"B{B}"] = leg
        res[f"bits{wb}"] = leg_w
        engs.clear()
        del eng
        gc.collect()
    return res


def decode_rules(layers, batches, steps, rounds, ctx):
    """Greedy decode steps with logits rules against plain ones: one engine, B sequences whose history is `ctx`
    text ids, repetition_penalty 1.2 + no_repeat_ngram_size 2 planned over that history plus what was generated; blocks of `steps`
    alternated `rounds` times in one process (round 0 warms up and is dropped).  Per batch: device ms per step of both (HIP events
    inside the engine: the edit launch is inside the bracket), wall ms per step, and the host time of plan + pack per step, which the
    ruled wall time contains."""
    from vstar_amd.logits import LogitRules
    B_max = max(batches + [1])
    max_ctx = (ctx + (rounds + 1) * steps * 2 * len(batches) + 64 + 63) // 64 * 64
    cfg = VQAConfig.seal_7b(llm_layers=layers, max_slots=B_max, max_ctx=max_ctx, max_rows=max(16384, ctx * 8), max_images=1)
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, 0, torch.float16, share_layers=True))
    rules = LogitRules(repetition_penalty=1.2, no_repeat_ngram_size=2)
    g = torch.Generator().manual_seed(0)
    res = {"config": {"layers": cfg.llm_layers, "hidden": cfg.llm_hidden, "vocab": cfg.llm_vocab, "history": ctx,
                      "rules": "repetition_penalty=1.2, no_repeat_ngram_size=2", "edit_capacity": eng.logit_edit_capacity()}}
    for B in batches:
        hist = [torch.randint(3, 30000, (ctx,), generator=g).tolist() for _ in range(B)]
        nxt = None
        for i0 in range(0, B, 8):                             # prefill in chunks of 8 sequences (max_rows)
            n = min(8, B - i0)
            _, t = eng.forward([Seq(hist[i0 + i], kv_slot=i0 + i) for i in range(n)], [(i, -1) for i in range(n)], logits=False)
            nxt = t if i0 == 0 else np.concatenate([nxt, t])
        pos, want = ctx, [(i, 0) for i in range(B)]
        dev, blocks, plan_ms, ids_per_step = {0: [], 1: []}, {0: [], 1: []}, [], []
        for r in range(rounds + 1):
            for on in (0, 1):
                t0, d = time.time(), []
                for s in range(steps):
                    for i in range(B):
                        hist[i].append(int(nxt[i]))
                    edits = None
                    if on:
                        tp = time.time()
                        edits = LogitRules.pack([rules.plan(hist[i], pos + 1 - ctx, None, i) for i in range(B)])
                        if r:
                            plan_ms.append((time.time() - tp) * 1e3)
                            ids_per_step.append(int(edits[0][-1]))
                    _, nxt = eng.forward([Seq([hist[i][-1]], kv_slot=i, past_len=pos) for i in range(B)], want, logits=False, edits=edits)
                    d.append(eng.last_forward_ms())
                    pos += 1
                if r:
                    blocks[on].append((time.time() - t0) / steps * 1e3)
                    dev[on] += d
        leg = {"positions": [ctx, pos], "host_plan_pack_ms_per_step": round(float(np.median(plan_ms)), 3),
               "edit_ids_per_step": int(np.median(ids_per_step))}
        for on, name in ((0, "plain"), (1, "rules")):
            w, d = float(np.median(blocks[on])), float(np.median(dev[on]))
            leg[name] = {"device_ms_per_step": round(d, 3), "wall_ms_per_step": round(w, 3),
                         "wall_ms_per_step_blocks": [round(x, 3) for x in blocks[on]],
                         "spread": round((max(blocks[on]) - min(blocks[on])) / w, 3)}
        leg["rules_minus_plain_device_ms"] = round(leg["rules"]["device_ms_per_step"] - leg["plain"]["device_ms_per_step"], 3)
        leg["rules_over_plain_wall"] = round(leg["rules"]["wall_ms_per_step"] / leg["plain"]["wall_ms_per_step"], 3)
        res[f"B{B}"] = leg
    return res


def decode_spec(layers, ds, n_tok, corrupts, rounds, kernel_rows):
    """Speculative against plain greedy decode of one sequence in one process (see the module docstring)."""
    from vstar_amd.spec import ReplayDrafter
    from vstar_amd.vqa import VQA_LLM
    cfg = VQAConfig.seal_7b(llm_layers=layers, max_slots=2, max_ctx=1024, max_rows=16384, max_images=1)
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, 0, torch.float16, share_layers=True))
    llm = VQA_LLM(cfg=cfg, engine=eng)
    llm.eos_token_id = -1                        # seeded random weights: no stop token, every block decodes n_tok tokens
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(3, 30000, (296,), generator=g).tolist()
    P = len(prompt)
    res = {"config": {"layers": cfg.llm_layers, "hidden": cfg.llm_hidden, "prompt_rows": P, "tokens_per_block": n_tok}}
    if kernel_rows:
        R = kernel_rows
        eng.forward([Seq(prompt, kv_slot=0)], [(0, -1)], logits=False)
        step, want = [Seq(prompt[:R], kv_slot=0, past_len=P)], [(0, r) for r in range(R)]
        draft = prompt[1:R] + [-1]
        for _ in range(20):
            eng.forward(step, want, logits=False)
            eng.forward_verify(step, want, [0, R], draft)
            eng.forward_verify(step, want, [0, R], draft, [sampling_params(0.7, 50, 0.9, seed=1, step=r) for r in range(R)])
        res["spec_kernels"] = {"rows": R, "calls": 20}
        return res
    seq = lambda: [Seq(prompt, kv_slot=0)]       # noqa: E731
    plain = llm.greedy_decode(seq(), [P], n_tok)
    # device time of one verify step against its row count (the drafts are wrong: only the step's cost is measured)
    rows_ms = {}
    for R in (1, 2, 4, 7, 8, 9, 16):
        step, want = [Seq(prompt[:R], kv_slot=0, past_len=P)], [(0, r) for r in range(R)]
        ms = []
        for _ in range(6):
            eng.forward_verify(step, want, [0, R], prompt[1:R] + [-1])
            ms.append(eng.last_forward_ms())
        rows_ms[str(R)] = round(float(np.median(ms[1:])), 3)
    res["verify_step_device_ms_by_rows"] = rows_ms
    legs = {}
    for d in ds:
        for c in corrupts:
            drafter = ReplayDrafter([prompt], plain, cfg.llm_vocab, corrupt=c, seed=d)
            run = {"greedy": lambda: llm.greedy_decode(seq(), [P], n_tok),
                   "spec": lambda: llm.speculative_decode(seq(), [P], [prompt], n_tok, d, None, drafter)}
            t = {"greedy": [], "spec": []}
            outs = {}
            for r in range(rounds + 1):          # round 0 warms up and is dropped
                for m in ("greedy", "spec"):
                    t0 = time.time()
                    outs[m] = run[m]()
                    if r:
                        t[m].append(time.time() - t0)
            st = dict(llm.spec_stats)
            leg = {"stats": st, "acceptance": round(st["accepted"] / max(st["drafted"], 1), 3),
                   "tokens_per_call": round(st["tokens"] / st["calls"], 3),
                   "agreement_with_greedy": round(sum(x == y for x, y in zip(outs["spec"][0], outs["greedy"][0])) / n_tok, 4)}
            for m in ("greedy", "spec"):
                med = float(np.median(t[m]))
                leg[m] = {"tokens_per_s": round(len(outs[m][0]) / med, 1), "block_ms": [round(x * 1e3, 1) for x in t[m]],
                          "spread": round((max(t[m]) - min(t[m])) / med, 3)}
            leg["spec_over_greedy_tokens_per_s"] = round(leg["spec"]["tokens_per_s"] / leg["greedy"]["tokens_per_s"], 3)
            legs[f"d{d}_corrupt{c}"] = leg
    res["decode_spec"] = legs
    return res


def score_kernels(eng, cfg, n):
    """The arg-max tail and the scoring tail on n wanted rows of one 300-row prompt, 20 calls each (for a kernel trace)."""
    g = torch.Generator().manual_seed(0)
    eng.encode_images(torch.randn(1, 3, 224, 224, generator=g), 0)
    rows = torch.randint(3, 30000, (44,), generator=g).tolist() + eng.feature_rows(0, True)
    seqs, want = [Seq(rows, kv_slot=0)], [(0, t % len(rows)) for t in range(n)]
    tg = torch.randint(0, cfg.llm_vocab, (n,), generator=g).numpy()
    for _ in range(20):
        if n <= 256:
            eng.forward(seqs, want, logits=False)
        eng.forward_score(seqs, want, tg, rank=True)
    return {"rows": n, "calls": 20}


def decode_sample(eng, rows, batches, steps, rounds, warp=False):
    """Greedy vs sampled decode steps of B sequences, alternated in blocks of `steps` (same KV positions advance).  warp: a third
    kind of block, the sampled step with min_p = 0.05 and typical_p = 0.9 behind top-k / top-p (every added pass of the kernel)."""
    from vstar_amd.vqa import warper_params
    modes = ("greedy", "sample", "warp") if warp else ("greedy", "sample")
    wrec = warper_params(min_p=0.05, typical_p=0.9)
    res = {}
    for B in batches:
        seqs = [Seq(rows, kv_slot=i) for i in range(B)]
        _, nxt = eng.forward(seqs, [(i, -1) for i in range(B)], logits=False)
        pos = len(rows)
        want = [(i, 0) for i in range(B)]
        dev = {m: [] for m in modes}
        wall = {m: 0.0 for m in modes}
        for r in range(rounds):
            for mode in modes:
                t0 = time.time()
                for s in range(steps):
                    step = [Seq([int(nxt[i])], kv_slot=i, past_len=pos) for i in range(B)]
                    if mode == "greedy":
                        _, nxt = eng.forward(step, want, logits=False)
                    else:
                        nxt = eng.forward_sample(step, want, [sampling_params(0.7, 50, 0.9, seed=i, step=r * steps + s)
                                                              for i in range(B)], **(dict(warpers=wrec) if mode == "warp" else {}))
                    dev[mode].append(eng.last_forward_ms())
                    pos += 1
                wall[mode] += time.time() - t0
        leg = {}
        for mode in modes:
            w = wall[mode] / (rounds * steps) * 1e3
            leg[mode] = {"device_ms_per_step": round(float(np.median(dev[mode])), 3), "wall_ms_per_step": round(w, 3),
                         "tokens_per_s": round(B / w * 1e3, 1)}
        leg["sample_over_greedy_tokens_per_s"] = round(leg["sample"]["tokens_per_s"] / leg["greedy"]["tokens_per_s"], 4)
        leg["sample_minus_greedy_device_ms"] = round(leg["sample"]["device_ms_per_step"] - leg["greedy"]["device_ms_per_step"], 4)
        if warp:
            leg["warp_over_sample_tokens_per_s"] = round(leg["warp"]["tokens_per_s"] / leg["sample"]["tokens_per_s"], 4)
            leg["warp_minus_sample_device_ms"] = round(leg["warp"]["device_ms_per_step"] - leg["sample"]["device_ms_per_step"], 4)
        res[f"B{B}"] = leg
    return res


def decode_logprobs(eng, rows, batches, steps, rounds, ns):
    """Greedy decode steps of B sequences without (`off`) and with the log-probability stage (`n<k>`: logprobs=k),
    alternated in blocks of `steps` (the same KV positions advance; the tokens are the same in every mode)."""
    modes = ["off"] + [f"n{n}" for n in ns]
    res = {}
    for B in batches:
        seqs = [Seq(rows, kv_slot=i) for i in range(B)]
        _, nxt = eng.forward(seqs, [(i, -1) for i in range(B)], logits=False)
        eng.forward(seqs, [(i, -1) for i in range(B)], logits=False, logprobs=max(ns))      # (the stage's buffers exist before the timing)
        pos = len(rows)
        want = [(i, 0) for i in range(B)]
        dev = {m: [] for m in modes}
        wall = {m: 0.0 for m in modes}
        for r in range(rounds):
            for m in modes:
                t0 = time.time()
                for s in range(steps):
                    step = [Seq([int(nxt[i])], kv_slot=i, past_len=pos) for i in range(B)]
                    nxt = eng.forward(step, want, logits=False, **({} if m == "off" else {"logprobs": int(m[1:])}))[1]
                    dev[m].append(eng.last_forward_ms())
                    pos += 1
                wall[m] += time.time() - t0
        leg = {}
        for m in modes:
            w = wall[m] / (rounds * steps) * 1e3
            leg[m] = {"device_ms_per_step": round(float(np.median(dev[m])), 3), "wall_ms_per_step": round(w, 3),
                      "tokens_per_s": round(B / w * 1e3, 1)}
        for m in modes[1:]:
            leg[m]["over_off_tokens_per_s"] = round(leg[m]["tokens_per_s"] / leg["off"]["tokens_per_s"], 4)
            leg[m]["minus_off_device_ms"] = round(leg[m]["device_ms_per_step"] - leg["off"]["device_ms_per_step"], 4)
        res[f"B{B}"] = leg
    return res


def guide_kernels(pairs, vocab=32001, reps=20):
    """The guidance kernel through its door on `pairs` pairs of random fp16 rows (gamma 1.5, every other pair with the plausibility cut at
    beta 0.1) and the beam select on `pairs` rows of the same matrix, `reps` launches each: the rows of a `rocprofv3 --kernel-trace
    --stats` run of their own (guide_rows_kernel next to beam_rows_kernel, the same row pass over one row)."""
    import ctypes
    from vstar_amd import _lib
    lib = _lib.load()
    ld = (vocab + 255) // 256 * 256
    x0 = (torch.randn(2 * pairs, ld, generator=torch.Generator().manual_seed(0)) * 3).half().cuda()
    cond, neg = np.arange(pairs, dtype=np.int32), np.arange(pairs, 2 * pairs, dtype=np.int32)
    sc = np.full(pairs, 1.5, np.float32)
    lb = np.where(np.arange(pairs) % 2 == 1, np.float32(np.log(0.1)), np.float32(-np.inf)).astype(np.float32)
    p = lambda arr: ctypes.c_void_p(arr.ctypes.data)      # noqa: E731
    for _ in range(reps):
        x = x0.clone()
        _lib.check_vqa(lib.vstar_vqa_guide_rows(ctypes.c_void_p(x.data_ptr()), _lib.F16, 2 * pairs, vocab, ld, pairs, p(cond), p(neg), p(sc), p(lb)))
    scores, goff = np.zeros(pairs, np.float32), np.arange(pairs + 1, dtype=np.int32)
    cs, ct, cr = np.empty((pairs, 2), np.float32), np.empty((pairs, 2), np.int32), np.empty((pairs, 2), np.int32)
    for _ in range(reps):
        _lib.check_vqa(lib.vstar_vqa_op_beam_select(ctypes.c_void_p(x0.data_ptr()), _lib.F16, pairs, vocab, ld, p(scores), pairs, p(goff), 2,
                                                    p(cs), p(ct), p(cr), None))
    return {"pairs": pairs, "vocab": vocab, "launches_each": reps}


def decode_guidance(eng, rows, neg_rows, batches, steps, rounds, gamma=1.5):
    """Guided decode steps of B samples (B output rows + B negative rows in one call, then the guidance kernel) against two yardsticks of
    the same process: greedy steps of B sequences, and greedy steps of 2 B sequences — the floor, as a guided step is a 2 B-row step plus
    one kernel.  Slots 0 .. B-1 hold the prompt, slots B .. 2B-1 the image-free prompt; blocks of `steps` alternated `rounds` times,
    every slot advancing from its own position.  tokens/s counts emitted tokens: B per guided and greedy step, 2 B per greedy2 step."""
    modes = ("greedy", "greedy2", "guided")
    res = {}
    for B in batches:
        seqs = [Seq(rows, kv_slot=i) for i in range(B)] + [Seq(neg_rows, kv_slot=B + i) for i in range(B)]
        want2 = [(i, 0) for i in range(2 * B)]
        g = (np.arange(B, 2 * B, dtype=np.int32), np.float32(gamma), np.float32(-np.inf))
        _, nxt = eng.forward(seqs, [(i, -1) for i in range(2 * B)], logits=False)
        eng.forward(seqs, [(i, -1) for i in range(2 * B)], logits=False, guidance=g)      # (the stage's buffers exist before the timing)
        nxt = [int(t) for t in nxt]
        pos = [len(rows)] * B + [len(neg_rows)] * B
        dev = {m: [] for m in modes}
        wall = {m: 0.0 for m in modes}
        for r in range(rounds + 1):                  # (round 0 warms up and is dropped)
            for m in modes:
                t0 = time.time()
                for s in range(steps):
                    idx = range(B) if m == "greedy" else range(2 * B)
                    step = [Seq([nxt[i if m != "guided" else i % B]], kv_slot=i, past_len=pos[i]) for i in idx]
                    if m == "guided":
                        tok = eng.forward(step, want2, logits=False, guidance=g)[1]
                        for i in range(B):
                            nxt[i] = int(tok[i])
                    else:
                        tok = eng.forward(step, want2[:len(step)], logits=False)[1]
                        for j, i in enumerate(idx):
                            nxt[i] = int(tok[j])
                    for i in idx:
                        pos[i] += 1
                    if r:
                        dev[m].append(eng.last_forward_ms())
                if r:
                    wall[m] += time.time() - t0
        leg = {"gamma": gamma, "prompt_rows": len(rows), "negative_rows": len(neg_rows), "steps_per_block": steps, "blocks": rounds}
        for m in modes:
            w = wall[m] / (rounds * steps) * 1e3
            leg[m] = {"device_ms_per_step": round(float(np.median(dev[m])), 3), "wall_ms_per_step": round(w, 3),
                      "tokens_per_s": round((2 * B if m == "greedy2" else B) / w * 1e3, 1)}
        leg["guided_over_greedy_tokens_per_s"] = round(leg["guided"]["tokens_per_s"] / leg["greedy"]["tokens_per_s"], 4)
        leg["guided_minus_greedy2_device_ms"] = round(leg["guided"]["device_ms_per_step"] - leg["greedy2"]["device_ms_per_step"], 4)
        leg["guided_minus_greedy2_wall_ms"] = round(leg["guided"]["wall_ms_per_step"] - leg["greedy2"]["wall_ms_per_step"], 4)
        res[f"B{B}"] = leg
    return res


def decode_contrast(eng, rows, ks, steps, rounds, alpha=0.6):
    """Contrastive-search steps of one prompt with k candidates (owner slot k, candidate c in slot k + c: k forked one-row sequences,
    then the penalty, select and adopt kernels) vs greedy one-row steps of the same prompt (slot 0), alternated in blocks of `steps`.
    Both emit one token per step; the history grows from len(rows) positions."""
    res = {}
    P = len(rows)
    for k in ks:
        slots = list(range(k, 2 * k))
        _, nxt = eng.forward([Seq(rows, kv_slot=0)], [(0, -1)], logits=False)
        tok, prob = eng.forward_contrast_begin([Seq(rows, kv_slot=slots[0])], [(0, -1)], k)
        state = {"nxt": nxt, "ct": tok[0].copy(), "cp": prob[0].copy(), "gpos": P, "cpos": P}

        def one(mode):
            if mode == "greedy":
                _, state["nxt"] = eng.forward([Seq([int(state["nxt"][0])], kv_slot=0, past_len=state["gpos"])], [(0, 0)], logits=False)
                state["gpos"] += 1
            else:
                step = [Seq([int(state["ct"][c])], kv_slot=slots[c], past_len=state["cpos"], prefix_slot=slots[0]) for c in range(k)]
                sel, ntok, nprob = eng.forward_contrast_step(step, [0, k], state["cp"], alpha, k)
                state["ct"], state["cp"] = ntok[0].copy(), nprob[0].copy()
                state["cpos"] += 1

        for mode in ("greedy", "contrast"):      # warm-up: code objects, the k-row kernels' first launches
            one(mode)
            one(mode)
        dev = {"greedy": [], "contrast": []}
        wall = {"greedy": 0.0, "contrast": 0.0}
        for r in range(rounds):
            for mode in ("greedy", "contrast"):
                t0 = time.time()
                for s in range(steps):
                    one(mode)
                    dev[mode].append(eng.last_forward_ms())
                wall[mode] += time.time() - t0
        leg = {"alpha": alpha, "prompt_rows": P, "steps_per_block": steps, "blocks": rounds}
        for mode in ("greedy", "contrast"):
            w = wall[mode] / (rounds * steps) * 1e3
            leg[mode] = {"device_ms_per_step": round(float(np.median(dev[mode])), 3), "wall_ms_per_step": round(w, 3),
                         "tokens_per_s": round(1e3 / w, 1)}
        leg["contrast_over_greedy_tokens_per_s"] = round(leg["contrast"]["tokens_per_s"] / leg["greedy"]["tokens_per_s"], 4)
        leg["contrast_over_greedy_device_ms"] = round(leg["contrast"]["device_ms_per_step"] / leg["greedy"]["device_ms_per_step"], 4)
        res[f"k{k}"] = leg
    return res


def decode_beams(eng, rows, beams, steps, rounds):
    """Beam-search steps (k beams of one prompt, slots k .. 2k-1: select tail + host scorer + ancestry reorder) vs greedy steps
    of k copies of the prompt (slots 0 .. k-1), alternated in blocks of `steps`.  EOS is disabled (id -1) so that every step
    runs all k beams."""
    from vstar_amd.beam import BeamSearch
    res = {}
    P = len(rows)
    for k in beams:
        g_slots, b_slots = list(range(k)), list(range(k, 2 * k))
        _, nxt = eng.forward([Seq(rows, kv_slot=s) for s in g_slots], [(i, -1) for i in range(k)], logits=False)
        bs = BeamSearch(k, P, -1, 10 ** 9)
        cs, ct, cr, _ = eng.forward_beam([Seq(rows, kv_slot=b_slots[0])], [(0, -1)] * k, bs.scores, [0, k], 2 * k)
        gpos = bpos = P
        goff = [0, k]
        dev = {"greedy": [], "beam": []}
        wall = {"greedy": 0.0, "beam": 0.0}
        for r in range(rounds):
            for mode in ("greedy", "beam"):
                t0 = time.time()
                for s in range(steps):
                    if mode == "greedy":
                        _, nxt = eng.forward([Seq([int(nxt[i])], kv_slot=g_slots[i], past_len=gpos) for i in range(k)],
                                             [(i, 0) for i in range(k)], logits=False)
                        gpos += 1
                    else:
                        par = bs.process(cs[0], ct[0], cr[0])
                        eng.kv_reorder(b_slots, [b_slots[p] for p in par], 0, bpos)
                        cs, ct, cr, _ = eng.forward_beam([Seq([bs.tokens[b][-1]], kv_slot=b_slots[b], past_len=bpos) for b in range(k)],
                                                         [(b, 0) for b in range(k)], bs.scores, goff, 2 * k)
                        bpos += 1
                    dev[mode].append(eng.last_forward_ms())
                wall[mode] += time.time() - t0
        leg = {}
        for mode in ("greedy", "beam"):
            w = wall[mode] / (rounds * steps) * 1e3
            leg[mode] = {"device_ms_per_step": round(float(np.median(dev[mode])), 3), "wall_ms_per_step": round(w, 3),
                         "tokens_per_s": round(k / w * 1e3, 1)}
        leg["beam_over_greedy_step_time"] = round(leg["beam"]["wall_ms_per_step"] / leg["greedy"]["wall_ms_per_step"], 4)
        leg["beam_minus_greedy_device_ms"] = round(leg["beam"]["device_ms_per_step"] - leg["greedy"]["device_ms_per_step"], 4)
        res[f"k{k}"] = leg
    return res


if __name__ == "__main__":
    main()
