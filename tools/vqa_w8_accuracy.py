"""Logits error and option rankings of the int8 weight-only decode mode, or with --bits 4 of the int4 group-scaled
mode (§8.6), or with --kv-bits 8 of the block-scaled fp8 KV cache (§8.7, fp16 weights), against the unquantised fp16 engine on the inputs of tests/golden/vqa_tiny_*.npz.  Reported, not asserted: the weights
are seeded random numbers, which says little about a trained checkpoint.  Prints one JSON object.

  python tools/vqa_w8_accuracy.py [--out profiles/vqa_w8_accuracy.json]
  python tools/vqa_w8_accuracy.py --bits 4 [--out profiles/vqa_w4_accuracy.json]
  python tools/vqa_w8_accuracy.py --kv-bits 8 [--out profiles/vqa_kv8_accuracy.json]
"""
import argparse
import ast
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_vqa_golden import make_inputs  # noqa: E402
from vstar_amd.config import VQAConfig  # noqa: E402
from vstar_amd.vqa_engine import Seq, VqaEngine  # noqa: E402
from vstar_amd.weights import random_state_dict  # noqa: E402


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def load_case(path):
    """The golden file's configuration and the inputs it was produced from, regenerated from its seeds."""
    z = np.load(path)
    cfg = VQAConfig.tiny(**ast.literal_eval(str(z["cfg_kw"])))
    n_obj = int(z["n_obj"])
    pix, ids, opts = make_inputs(cfg, int(z["input_seed"]), n_obj, len(z["ids"]), z["opt_lens"].tolist())
    assert ids == z["ids"].tolist() and np.concatenate(opts).tolist() == z["opts"].tolist()
    il = None if z["images_long"][0] < 0 else [bool(b) for b in z["images_long"]]
    ol = None if z["objects_long"][0] < 0 else [bool(b) for b in z["objects_long"]]
    return z, cfg, pix, ids, opts, n_obj, il, ol


def run(cfg, wseed, pix, ids, opts, n_obj, il, ol):
    eng = VqaEngine(cfg, 0)
    eng.load_state_dict(random_state_dict(cfg, seed=wseed, dtype=torch.float16))
    eng.encode_images(pix, 0)
    rows = eng.expand_ids(ids, [0], list(range(1, 1 + n_obj)), il, ol)
    S = len(rows)
    q_logits, _ = eng.forward([Seq(rows, kv_slot=0)], [(0, -1)])                       # prefill: the tile kernels
    o_logits, _ = eng.forward([Seq(o, kv_slot=1 + j, past_len=S, prefix_slot=0) for j, o in enumerate(opts)],
                              [(j, t) for j, o in enumerate(opts) for t in range(len(o))])      # <= 64 rows: the decode kernels
    losses, k = [], 0
    for o in opts:
        lg = torch.cat([torch.from_numpy(q_logits[-1:]), torch.from_numpy(o_logits[k:k + len(o) - 1])], 0)
        k += len(o)
        losses.append(float(torch.nn.functional.cross_entropy(lg.float(), torch.tensor(o))))
    del eng
    return q_logits, o_logits, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--bits", type=int, default=8, choices=[4, 8], help="the quantised mode compared with fp16")
    ap.add_argument("--kv-bits", type=int, default=0, choices=[0, 8], help="8: compare the fp8 KV cache (fp16 weights) with fp16 instead")
    a = ap.parse_args()
    out = {}
    B, w = (a.bits, f"w{a.bits}") if not a.kv_bits else ("kv8", "kv8")
    mode = lambda cfg, b: cfg if b == 0 else (cfg.with_kv_bits(8) if b == "kv8" else cfg.with_decode_bits(b))      # noqa: E731
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "vqa_tiny_*.npz"))):
        z, cfg, pix, ids, opts, n_obj, il, ol = load_case(path)
        res = {b: run(mode(cfg, b), int(z["weight_seed"]), pix, ids, opts, n_obj, il, ol) for b in (0, B)}
        rank = {b: np.argsort(res[b][2]).tolist() for b in (0, B)}
        out[os.path.basename(path)] = {
            f"q_logits_rel_l2_{w}_vs_fp16": rel_l2(res[B][0], res[0][0]), f"opt_logits_rel_l2_{w}_vs_fp16": rel_l2(res[B][1], res[0][1]),
            "q_logits_rel_l2_fp16_vs_golden": rel_l2(res[0][0][-1], z["q_logits_last"]),
            f"q_logits_rel_l2_{w}_vs_golden": rel_l2(res[B][0][-1], z["q_logits_last"]),
            "losses_fp16": [round(x, 4) for x in res[0][2]], f"losses_{w}": [round(x, 4) for x in res[B][2]],
            "losses_golden": np.asarray(z["losses"]).round(4).tolist(),
            "ranking_fp16": rank[0], f"ranking_{w}": rank[B], "ranking_golden": np.argsort(z["losses"]).tolist(),
            "ranking_survives": rank[B] == np.argsort(z["losses"]).tolist()}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
