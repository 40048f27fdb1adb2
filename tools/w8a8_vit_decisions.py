"""What VSMConfig.vit_w8a8 does to the scheduler's decisions: over 64 crops of the bench batch at the 7B geometry with trained-like
weights (share_layers=True), how often the W8A8 engine — LLaMA linears only (llm_w8a8 = 1), and with the CLIP / OWL-ViT tower linears
on the fp8 MFMA too (+ vit_w8a8 = 1) — picks the bf16 engine's arg-max box, takes the same side of the confidence / cue thresholds
and ranks the four children in the same order (tests/_parity.py::decisions / decision_agreement, as tests/test_w8a8_decisions_gpu.py
uses them).  Writes JSON (default profiles/w8a8_vit_decisions.json; the committed file sits next to profiles/r04_w8a8_decisions*.json).
usage: python tools/w8a8_vit_decisions.py [--out FILE] [--weights trained_like|random]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _parity import decision_agreement, decisions  # noqa: E402
from vstar_amd import preprocess as pp  # noqa: E402
from vstar_amd import provenance  # noqa: E402
from vstar_amd.config import VSMConfig  # noqa: E402
from vstar_amd.engine import VstarEngine  # noqa: E402
from vstar_amd.synthetic import bench_inputs  # noqa: E402
from vstar_amd.weights import random_state_dict, template_chain, trained_like_state_dict  # noqa: E402

B, T, ROUNDS = 32, 64, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w8a8_vit_decisions.json"))
    ap.add_argument("--weights", default="trained_like", choices=["trained_like", "random"])
    args = ap.parse_args()
    os.environ.pop("VSTAR_W8A8_VIT", None)               # the configs below decide
    dev = torch.device("cuda:0")
    modes = {"bf16": dict(), "llm_w8a8": dict(llm_w8a8=1), "llm_w8a8+vit_w8a8": dict(llm_w8a8=1, vit_w8a8=1)}
    base = VSMConfig.seal_7b(336, max_batch=B, max_text_len=T + 1)
    if args.weights == "trained_like":
        sd = trained_like_state_dict(base, seed=0, dtype=torch.bfloat16, share_layers=True, chain=template_chain(pp.SyntheticTokenizer(base.llm_vocab)))
    else:
        sd = random_state_dict(base, seed=0, dtype=torch.bfloat16, share_layers=True)
    dec, active = {}, {}
    for name, kw in modes.items():
        eng = VstarEngine(VSMConfig.seal_7b(336, max_batch=B, max_text_len=T + 1, **kw), 0)
        eng.load_state_dict(sd)
        dec[name] = []
        for r in range(ROUNDS):
            clip, owl, ids, loc, verify = bench_inputs(base, B, T, rank=r)
            o = eng.score_batch(clip.to(dev), owl.to(dev), ids, loc, verify_pos=verify)
            dec[name] += [decisions(o["pred_logits"][b, :, 0], o["pred_boxes"][b], o["low_res_masks"][b, 0]) for b in range(B)]
        active[name] = {"w8a8_vit_active": eng.w8a8_vit_active(), "w8a8_mx_active": eng.w8a8_mx_active()}
        eng.close()
    tops = np.asarray([d["top_score"] for d in dec["bf16"]])
    smax = np.asarray([d["score_max"] for d in dec["bf16"]])
    thr = ((0.5, 0.3, float(np.median(tops))), (6.0, 4.2, 3.0, float(np.median(smax))))
    report = {"weights": args.weights, "share_layers": True, "crops": len(dec["bf16"]), "kernel_source_hash": provenance.checked_hash(), "engines": active,
              "llm_w8a8_vs_bf16": decision_agreement(dec["llm_w8a8"], dec["bf16"], *thr),
              "llm_w8a8+vit_w8a8_vs_bf16": decision_agreement(dec["llm_w8a8+vit_w8a8"], dec["bf16"], *thr),
              "llm_w8a8+vit_w8a8_vs_llm_w8a8": decision_agreement(dec["llm_w8a8+vit_w8a8"], dec["llm_w8a8"], *thr)}
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
