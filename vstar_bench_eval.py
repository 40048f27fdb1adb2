#!/usr/bin/env python
"""V*Bench end-to-end entry point (reference: vstar_bench_eval.py:168-293), both models on the HIP engines:
the SEAL VQA-LLM (`vstar_amd.vqa.VQA_LLM`, fp16, KV-cached) and the visual-search model (`vstar_amd.vsm.VSM`, bf16).
`--vqa-model-path` / `--vsm-model-path` are local HF checkpoint directories (there is no hub access in this environment);
`--vqa-llm module:factory` substitutes another object with the reference's VQA_LLM interface.
"""
from __future__ import annotations

import argparse
import importlib
import sys


def parse_args(argv):
    p = argparse.ArgumentParser()
    p.add_argument("--vqa-model-path", type=str, default="craigwu/seal_vqa_7b")
    p.add_argument("--vqa-model-base", type=str, default=None)
    p.add_argument("--conv_type", default="v1", type=str)
    p.add_argument("--benchmark-folder", type=str, default="vstar_bench")
    p.add_argument("--vsm-model-path", type=str, default="craigwu/seal_vsm_7b")
    p.add_argument("--output-path", type=str, default="eval_result.json")
    p.add_argument("--minimum_size_scale", default=4.0, type=float)
    p.add_argument("--minimum_size", default=224, type=int)
    p.add_argument("--vision-tower", dest="vision_tower", default=None, help="local openai/clip-vit-large-patch14 directory")
    p.add_argument("--vqa-llm", default=None, help="module:factory providing another VQA-LLM implementation")
    p.add_argument("--vsm-factory", default=None, help="module:factory(args, device) providing another VSM implementation")
    p.add_argument("--device", default=0, type=int)
    p.add_argument("--vqa-decode-bits", dest="vqa_decode_bits", default=0, type=int, choices=[0, 4, 8],
                   help="8: the VQA-LLM's int8 weight-only decode mode (DESIGN.md 8.4); 4: its int4 group-scaled mode (8.6); "
                        "0: fp16 weights everywhere")
    p.add_argument("--vqa-kv-bits", dest="vqa_kv_bits", default=0, type=int, choices=[0, 8],
                   help="8: the VQA-LLM's block-scaled fp8 KV cache (MX e4m3, blocks of 32: 132 bytes per cached row instead of 256; "
                        "DESIGN.md 8.7); 0: the fp16 cache.  Independent of --vqa-decode-bits")
    p.add_argument("--search-window", dest="search_window", default=0, type=int, help="concurrent visual searches per engine batch "
                   "(cross-image lock step); 0 = one engine batch, 1 = one image at a time like the reference")
    p.add_argument("--vqa-batch", dest="vqa_batch", default=1, type=int, help="questions per VQA-LLM engine call in the free-form and "
                   "option-ranking passes (free_form_batch / multiple_choices_batch, option losses reduced on the device); 1 = one "
                   "question at a time like the reference.  The free-form pass sends at most min(N, max_slots, max_images) questions per call; the "
                   "option-ranking pass splits a batch by itself when it exceeds max_slots / max_images / max_rows")
    p.add_argument("--vqa-repetition-penalty", dest="vqa_repetition_penalty", default=1.0, type=float, help="theta > 0: HF's "
                   "repetition_penalty on the free-form pass, applied to the logits on the device (DESIGN.md 8.8); 1.0 = off")
    p.add_argument("--vqa-no-repeat-ngram", dest="vqa_no_repeat_ngram", default=0, type=int, help="n > 0: HF's no_repeat_ngram_size "
                   "on the free-form pass (DESIGN.md 8.8); 0 = off")
    p.add_argument("--vqa-spec-tokens", dest="vqa_spec_tokens", default=0, type=int, help="d > 0 (<= 15): the free-form pass decodes "
                   "speculatively with up to d prompt-lookup draft tokens per step (DESIGN.md 8.5; 3 keeps every kernel of a one-row "
                   "step at 7B); 0 = the plain greedy decode")
    p.add_argument("--vqa-logprobs", dest="vqa_logprobs", default=None, type=int, help="N in [0, 32]: the free-form pass also records, per "
                   "question, the mean log-probability of the answer's tokens and the per-token arrays (log-probability, rank, the N most "
                   "likely alternatives), computed on the device (DESIGN.md 8.9), as `freeform_logprobs` of the result record; off "
                   "(default) writes exactly the records without it")
    p.add_argument("--vqa-penalty-alpha", dest="vqa_penalty_alpha", default=None, type=float, help="alpha in (0, 1]: the free-form pass "
                   "decodes by contrastive search (HF's penalty_alpha) with --vqa-top-k candidates per step, the degeneration penalty and "
                   "the pick on the device (DESIGN.md 8.11); off (default) is the greedy decode")
    p.add_argument("--vqa-top-k", dest="vqa_top_k", default=None, type=int, help="K in [2, 32]: the candidates per step of "
                   "--vqa-penalty-alpha (each question then takes K KV slots); required with it, ignored without")
    p.add_argument("--vqa-guidance-scale", dest="vqa_guidance_scale", default=None, type=float, help="G >= 0: the free-form pass decodes "
                   "every question against the same prompt without the image (classifier-free guidance / visual contrastive decoding, "
                   "HF's guidance_scale), the two logits rows combined on the device (DESIGN.md 8.12); each question then takes 2 KV "
                   "slots; off (default) or 1 is the plain decode")
    p.add_argument("--vqa-plausibility-beta", dest="vqa_plausibility_beta", default=0.0, type=float, help="B in [0, 1]: with "
                   "--vqa-guidance-scale, tokens whose probability under the un-guided row is below B times its maximum are dropped "
                   "(the adaptive plausibility constraint); 0 = off")
    p.add_argument("--engine-comm", nargs="?", const="on", default="auto", choices=["auto", "on", "off"],
                   help="world > 1 on GPUs: gather the per-step records with the C-ABI's own RCCL communicator on the engine stream "
                   "(vstar_allgather_results) instead of torch.distributed.  auto (default, round 6): used when the communicator comes up "
                   "and its self-check against torch.distributed passes on every rank, otherwise every rank falls back together; off = "
                   "torch.distributed")
    return p.parse_args(argv)


def main(argv):
    """Single process: `python vstar_bench_eval.py ...`.  One node, N GPUs (BASELINE configs 3/4):
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 vstar_bench_eval.py ...` — one process
    per GPU, weights replicated, each visual-search engine step crop-sharded with an RCCL all-gather of the records."""
    args = parse_args(argv)
    from vstar_amd.dist import finalize, init_from_env
    world, rank, local_rank = init_from_env()
    finished = False
    try:
        if world > 1:
            args.device = local_rank
        if args.vqa_llm:
            mod, fn = args.vqa_llm.split(":")
            vqa_llm = getattr(importlib.import_module(mod), fn)(args)
        else:
            from vstar_amd.vqa import VQA_LLM
            vqa_llm = VQA_LLM(args, device=local_rank if world > 1 else args.device, decode_weight_bits=args.vqa_decode_bits or None,
                              kv_cache_bits=args.vqa_kv_bits or None)
        from vstar_amd.bench_eval import eval_model, make_vsm
        vsm = None
        if args.vsm_factory:
            mod, fn = args.vsm_factory.split(":")
            vsm = getattr(importlib.import_module(mod), fn)(args, local_rank)
        elif world > 1:
            vsm = make_vsm(args, local_rank)
        if args.engine_comm != "off" and vsm is not None and world > 1:
            from vstar_amd.dist import maybe_engine_comm
            maybe_engine_comm(vsm)
        eval_model(args, vqa_llm, vsm, world=world, rank=rank)
        finished = True
    finally:
        finalize(finished)


if __name__ == "__main__":
    main(sys.argv[1:])
