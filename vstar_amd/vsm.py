"""Drop-in for the reference's `VSM` wrapper class (visual_search.py:142-225) on top of the HIP engine.

Same constructor argument (the `parse_args` namespace: version, vision_tower, conv_type, use_mm_start_end,
model_max_length) and the same `inference(image, question, mode)` return conventions:
  'detection'    -> (pred_boxes [2304,4] cpu, sigmoid scores [2304,1] cpu in BFLOAT16, heatmap [h,w] clamped >= 0)
                    (the reference returns det_result['pred_logits'][0].sigmoid().cpu() of a bf16 tensor, visual_search.py:225:
                    the bf16 rounding of the sigmoid creates TIES among the top scores and the scheduler's argmax() / `>`
                    thresholds act on those rounded values, so the scores keep that dtype here)
  'segmentation' -> heatmap [h,w]
  'vqa'          -> str            (greedy decode WITHOUT a KV cache, exactly like the reference: one full prefill per
                                    generated token, VSM.py:151 `use_cache=False`; used only by the contextual-cue branch)
plus `inference_batch` (many crops, one engine pass) which is what the batched search scheduler calls.

Difference in mechanism, not in result: the reference runs HF greedy `generate` with use_cache=False and reads the
hidden state at the token before [LOC] from the LAST step (VSM.py:451-473).  Under causal attention that state equals
the one from a single prefill over prompt + "Sure, [LOC]." provided greedy decoding emits exactly that template; the
engine returns argmax(lm_head(h)) at the answer positions so that this is CHECKED per crop (`template_ok`).
"""
from __future__ import annotations

import os
import time
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from ._lib import GEN_MAX_BATCH, RESULT_FLOATS
from .config import VSMConfig
from .dist import allgather_numpy, allgather_records, pad_count, shard_indices
from .engine import VstarEngine
from .preprocess import (ANSWER_TEMPLATE, IMAGE_TOKEN_INDEX, LOCATE_QUESTION, SyntheticTokenizer, build_prompt, clip_preprocess,
                         owl_preprocess, tokenizer_image_token)
from .weights import load_checkpoint_dir, random_state_dict, template_chain, trained_like_state_dict


def _scores(logits: np.ndarray) -> torch.Tensor:
    """sigmoid of the (bf16-valued) class logits, evaluated and rounded in bfloat16 like the reference's tensor op."""
    return torch.from_numpy(np.ascontiguousarray(logits)).to(torch.bfloat16).sigmoid()


class TemplateMismatch(RuntimeError):
    """Kept for callers that caught it in round 1; no longer raised: a failed template check now falls back to the reference's
    own stepwise greedy decode (see VSM._decode_fallback)."""


class DeferredMismatch:
    """Placeholder result of a crop whose teacher-forced template check failed inside a SPECULATIVE batch.  The reference only
    ever evaluates crops it visits, so the stepwise-decode fallback (and the IndexError it may end in) is postponed until the
    search actually consumes the node (`_NodeScorer.get` calls `resolve()`); unvisited speculative crops cost nothing."""

    def __init__(self, fn):
        self._fn, self._done, self._value = fn, False, None

    def resolve(self):
        if not self._done:
            self._value = self._fn()          # may raise IndexError exactly like visual_search.py:209-225
            self._done = True
        return self._value


def w8a8_padded_len(L: int, n_img_tokens: int, max_text_len: int) -> int:
    """W8A8 (config 5): the block-scaled chain needs the step's rows to be a multiple of 256 (csrc/mx.hpp).  Right padding has no side
    effects (causal mask: it cannot reach the scored positions), so the spliced length S = L - 1 + P is rounded up to a multiple of
    8 — with the usual 32- / 64-crop batches the rows then ARE a multiple of 256, for at most 7 more positions per crop (1 %)."""
    Lpad = L + (-(L - 1 + n_img_tokens)) % 8
    return Lpad if Lpad <= max_text_len else L


class VSM:
    def __init__(self, args=None, *, engine: Optional[VstarEngine] = None, tokenizer=None, cfg: Optional[VSMConfig] = None,
                 device: int = 0, synthetic_seed: Optional[int] = None, strict_template: Optional[bool] = None):
        """`args`: the reference's argparse namespace.  If `args.version` is a local HF checkpoint directory (and
        `args.vision_tower` a local CLIP directory) real weights + tokenizer are loaded; otherwise pass
        `synthetic_seed` to run seeded random weights of the same architecture (benchmarks / tests)."""
        self.conv_type = getattr(args, "conv_type", "llava_v1")
        self.use_mm_start_end = getattr(args, "use_mm_start_end", True)
        if self.conv_type not in ("llava_v1", "llava_llama_2"):
            raise ValueError(f"unknown conv_type {self.conv_type!r} (visual_search.py:47: llava_v1 | llava_llama_2)")
        version = getattr(args, "version", None)
        real = version is not None and os.path.isdir(str(version))
        answers_template = False
        if engine is not None:
            self.engine = engine
            self.cfg = engine.cfg
        else:
            self.cfg = cfg or VSMConfig.seal_7b(224)
            self.engine = VstarEngine(self.cfg, device)
            if real:
                sd = load_checkpoint_dir(version, getattr(args, "vision_tower"))
            elif synthetic_seed is not None:
                # seeded weights with a trained checkpoint's statistics whose greedy decode answers locate prompts of the
                # SyntheticTokenizer with "Sure, [LOC]." (round 4): the default strict_template=True path runs on them
                sd = trained_like_state_dict(self.cfg, seed=synthetic_seed, dtype=torch.bfloat16, share_layers=True,
                                             chain=template_chain(SyntheticTokenizer(self.cfg.llm_vocab), conv_type=self.conv_type,
                                                                  use_mm_start_end=self.use_mm_start_end))
                answers_template = tokenizer is None
            else:
                raise FileNotFoundError(
                    f"checkpoint directory {version!r} not found and no synthetic_seed given (there is no hub access here)")
            self.engine.load_state_dict(sd)
        if tokenizer is not None:
            self.vsm_tokenizer = tokenizer
        elif real:
            from transformers import AutoTokenizer
            self.vsm_tokenizer = AutoTokenizer.from_pretrained(version, model_max_length=getattr(args, "model_max_length", 512),
                                                               padding_side="right", use_fast=False)
            self.vsm_tokenizer.pad_token = self.vsm_tokenizer.unk_token
        else:
            self.vsm_tokenizer = SyntheticTokenizer(self.cfg.llm_vocab)
        self.loc_token_idx = self.vsm_tokenizer("[LOC]", add_special_tokens=False).input_ids[0]
        self.strict_template = (real or answers_template) if strict_template is None else strict_template
        self.last_template_ok: Optional[np.ndarray] = None
        self.fallback_log: List[dict] = []      # one entry per stepwise-decode fallback (diagnostics / tests)
        import threading
        self._upload_lock = threading.Lock()
        self.timers = {"preprocess_s": 0.0, "engine_s": 0.0, "gather_s": 0.0, "post_s": 0.0, "crops": 0, "engine_calls": 0,
                       "generate_s": 0.0, "generate_tokens": 0, "generate_calls": 0}      # the batched cue decodes

    # ---- cost model of a scoring step (vstar_amd.search.SpeculationPolicy) ----
    step_ms_table = None    # {crops per rank: ms}; None = the policy's built-in MI355X measurements

    def calibrate_step_ms(self, batches=(1, 2, 4, 8, 16, 32), repeats: int = 2) -> dict:
        """Measures t(B) — one full scoring step of B crops on THIS engine and GPU — for the speculation cost model and stores it
        in `step_ms_table`.  Synthetic pixels and ids of the current geometry; ~1 s at the 7B geometry."""
        import time as _t
        cfg = self.cfg
        table = {}
        g = torch.Generator().manual_seed(0)
        ids1 = self._ids(LOCATE_QUESTION.format("object"))
        for B in batches:
            if B > cfg.max_batch:
                break
            clip = torch.randn(B, 3, cfg.clip_image_size, cfg.clip_image_size, generator=g).bfloat16()
            owl = torch.randn(B, 3, cfg.owl_image_size, cfg.owl_image_size, generator=g).bfloat16()
            ids = np.tile(ids1[0][None], (B, 1))
            loc = np.full((B,), ids1[1], np.int32)
            best = None
            for _ in range(repeats + 1):
                t0 = _t.perf_counter()
                self.engine.score_batch(clip, owl, ids, loc, raw=True)
                dt = (_t.perf_counter() - t0) * 1e3
                best = dt if best is None else min(best, dt)
            table[int(B)] = round(best, 3)
        # crop-sharded ranks must plan IDENTICAL batches (VSM._score_sharded deals crop i to rank i % world): a per-rank measured
        # table would let timing noise pick different speculative crops on different ranks and the all-gather would mismatch or
        # hang.  Every rank takes rank 0's table.
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            box = [table]
            dist.broadcast_object_list(box, src=0)
            table = {int(k): float(v) for k, v in box[0].items()}
        self.step_ms_table = table
        return table

    # ---- multi-GPU plumbing ----
    shard_crops = True      # False: this process scores every crop itself even when a process group exists (sample-level DP)

    def _dist(self):
        import torch.distributed as dist
        if self.shard_crops and dist.is_available() and dist.is_initialized():
            return dist.get_world_size(), dist.get_rank()
        return 1, 0

    def _score_sharded(self, n: int, score_chunk) -> np.ndarray:
        """Data-parallel scoring of n crops: crop i belongs to rank i % world; `score_chunk(sel, out_dev)` scores
        the crops `sel` of this rank (returning [len(sel), R] host records, or writing them into the device tensor `out_dev`).
        With the nccl backend (= RCCL over xGMI) the fixed-size records never leave HBM before the exchange: the engine writes
        them into a device buffer (VSTAR_F_DEVICE_OUTPUT), ONE all_gather_into_tensor moves them, and a single D2H copy of the
        gathered set follows.  gloo (CPU tests) and the single-process case use host records."""
        import torch.distributed as dist
        world, rank = self._dist()
        mine = shard_indices(n, rank, world)
        per = pad_count(n, world)
        mb = self.cfg.max_batch
        # a group of ONE nccl rank (bench.py --rccl-selfcheck, tests) still takes the device path: same code as N > 1
        grouped = self.shard_crops and dist.is_available() and dist.is_initialized()
        on_device = grouped and dist.get_backend() == "nccl"
        if on_device:
            local = torch.zeros((per, RESULT_FLOATS), dtype=torch.float32, device=f"cuda:{self.engine.device}")
        else:
            local = np.zeros((per, RESULT_FLOATS), dtype=np.float32)
        for s0 in range(0, len(mine), mb):
            sel = mine[s0:s0 + mb]
            t1 = time.perf_counter()
            if on_device:
                score_chunk(sel, local[s0:s0 + len(sel)])
            else:
                local[s0:s0 + len(sel)] = score_chunk(sel, None)
            self.timers["engine_s"] += time.perf_counter() - t1
            self.timers["crops"] += len(sel)
            self.timers["engine_calls"] = self.timers.get("engine_calls", 0) + 1
        t2 = time.perf_counter()
        if on_device and getattr(self.engine, "comm_world", 0) == world and getattr(self, "use_engine_comm", True):
            # the C-ABI's own collective (vstar_allgather_results: ncclAllGather on the engine's stream, queued behind the kernels
            # that wrote the records)
            from .dist import reorder_gathered
            records = reorder_gathered(self.engine.allgather_results(local), world, n).cpu().numpy()
        elif on_device:
            records = allgather_records(local, n).cpu().numpy()
        elif world == 1:
            records = local[:n]
        else:
            records = allgather_numpy(local, n, device="cpu")
        self.timers["gather_s"] += time.perf_counter() - t2
        return records

    # ---- prompt -> ids with the answer teacher-forced ----
    def _ids(self, question: str) -> Tuple[np.ndarray, int, List[int], List[int]]:
        prompt = build_prompt(question, self.use_mm_start_end, conv_type=self.conv_type)
        full = build_prompt(question, self.use_mm_start_end, answer=ANSWER_TEMPLATE, conv_type=self.conv_type)
        ids_p = tokenizer_image_token(prompt, self.vsm_tokenizer)
        ids_f = tokenizer_image_token(full, self.vsm_tokenizer)
        if ids_f[: len(ids_p)] != ids_p:
            # tokenisation merged across the "ASSISTANT:" boundary; tokenise the answer on its own
            ans = self.vsm_tokenizer(" " + ANSWER_TEMPLATE, add_special_tokens=False).input_ids
            ids_f = ids_p + list(ans)
        if ids_f.count(self.loc_token_idx) != 1:
            raise ValueError("the teacher-forced answer must contain exactly one [LOC] token")
        loc_col = ids_f.index(self.loc_token_idx)
        P = self.cfg.n_img_tokens
        # spliced positions whose next-token argmax must reproduce the answer tokens up to and including [LOC]
        first_ans = len(ids_p)
        ver_cols = list(range(first_ans, loc_col + 1))
        ver_pos = [c - 1 + (P - 1) for c in ver_cols]
        ver_tok = [ids_f[c] for c in ver_cols]
        return np.asarray(ids_f, dtype=np.int32), loc_col - 1 + (P - 1), ver_pos, ver_tok

    @torch.inference_mode()
    def inference_batch(self, images: Sequence[Image.Image], question: str, mode: str = "detection",
                        upsample: bool = True, defer_mismatch: bool = False):
        """Scores all `images` (crops) for one question in engine batches of cfg.max_batch.  Returns a list of per-crop
        results in the `inference` convention (with `upsample=False` the heatmap slot holds the 192x192 low-res logits).
        Crops whose teacher-forced template check fails are re-run through the stepwise greedy decode (reference semantics);
        with `defer_mismatch=True` that happens lazily (the slot holds a DeferredMismatch)."""
        assert mode in ("vqa", "segmentation", "detection")
        if mode == "vqa":
            if len(images) > 1 and hasattr(self.engine, "generate_batch"):      # several crops: one batched decode, the same tokens
                return [self._gen_text(t) for t in self.generate_ids_batch(images, question)]
            return [self.generate(im, question) for im in images]
        ids, loc_pos, ver_pos, ver_tok = self._ids(question)
        nv = min(len(ver_pos), 8)
        ver_pos, ver_tok = ver_pos[-nv:], ver_tok[-nv:]
        n = len(images)
        ids_b = lambda B: np.tile(ids[None], (B, 1))  # noqa: E731

        def score_chunk(sel, out_dev):
            chunk = [images[i] for i in sel]
            B = len(chunk)
            t0 = time.perf_counter()
            clip = torch.from_numpy(np.stack([clip_preprocess(im, self.cfg.clip_image_size) for im in chunk])).bfloat16()
            owl = torch.from_numpy(np.stack([owl_preprocess(im, self.cfg.owl_image_size) for im in chunk])).bfloat16()
            dt = time.perf_counter() - t0
            self.timers["preprocess_s"] += dt
            self.timers["engine_s"] -= dt               # _score_sharded times the whole chunk as engine time
            kw = {"out_dev": out_dev} if out_dev is not None else {}
            return self.engine.score_batch(clip, owl, ids_b(B), np.full((B,), loc_pos, np.int32),
                                           verify_pos=np.tile(np.asarray(ver_pos, np.int32)[None], (B, 1)), raw=True, **kw)
        records = self._score_sharded(n, score_chunk)
        res = self.engine.unpack(records, nv)
        ok_all = [(res["tf_argmax"] == np.asarray(ver_tok, np.int32)[None]).all(axis=1)] if n else []
        out: List = []
        for b, im in enumerate(images):
            w, h = im.size
            low = res["low_res_masks"][b, 0]
            heat = torch.from_numpy(self.engine.upsample_mask(low, h, w)) if upsample else torch.from_numpy(low.copy())
            if mode == "segmentation":
                out.append(heat)
            else:
                boxes = torch.from_numpy(res["pred_boxes"][b].copy())
                scores = _scores(res["pred_logits"][b])
                out.append((boxes, scores, heat))
        self.last_template_ok = np.concatenate(ok_all) if ok_all else np.zeros((0,), bool)
        self._handle_mismatches(out, lambda b: images[b], question, mode, upsample, defer_mismatch)
        return out

    # ---- GPU-side preprocessing path: the image lives in HBM, crops are boxes ----
    supports_deferred_mismatch = True

    @property
    def supports_device_reductions(self) -> bool:
        return hasattr(self.engine, "heatmap_stats")

    @property
    def supports_gpu_preprocess(self) -> bool:
        return hasattr(self.engine, "score_boxes") and hasattr(self.engine, "set_image")

    def set_image(self, image: Image.Image, slot: int = 0) -> None:
        """Uploads `image` into the engine's image slot `slot`; `inference_boxes(..., slots=...)` then scores crops of any
        resident image in one batch (cross-image lock-step search)."""
        if not hasattr(self, "_images"):
            self._images = {}
        self._images[int(slot)] = image
        if slot == 0:
            self._image = image
            self.engine.set_image(image)
        else:
            self.engine.set_image(image, int(slot))

    @property
    def supports_async_upload(self) -> bool:
        return hasattr(self.engine, "set_image_async")

    def set_image_async(self, image: Image.Image, slot: int) -> None:
        """set_image for a slot no live search uses yet, without stalling the scoring stream (engine.set_image_async).  Called by the
        stream search's prefetch thread while the main thread is inside an engine step."""
        if not hasattr(self, "_images"):
            self._images = {}
        self._images[int(slot)] = image
        if slot == 0:
            self._image = image
        with self._upload_lock:                 # the engine's staging ring serves one upload at a time
            self.engine.set_image_async(image, int(slot))

    def release_image(self, slot: int = 0) -> None:
        """The stream driver recycled `slot`: drop the host-side PIL image kept for the decode fallback (a 4K RGB image is 25 MB;
        64 slots of them were never released).  The device copy is simply overwritten by the next set_image."""
        imgs = getattr(self, "_images", None)
        if imgs is not None:
            imgs.pop(int(slot), None)
        # slot 0 doubles as the single-image API's slot (set_image(image) + inference_boxes without `slots`): its host copy stays
        # until the next set_image overwrites it, so that a later inference_boxes on the still-resident device image can take the
        # decode fallback (it crashed on None).  One image, not one per slot.

    @torch.inference_mode()
    def inference_boxes(self, boxes_xywh: Sequence[Sequence[float]], question, mode: str = "detection",
                        upsample: bool = True, defer_mismatch: bool = False, slots: Optional[Sequence[int]] = None):
        """Like inference_batch for crops `image.crop((int(x), int(y), int(x+w), int(y+h)))` of the image given to
        set_image(), but crop / pad / resize / normalise run on the GPU (bit-identical to the PIL + HF-processor path).
        `question` is one string for all boxes or one string PER box (several search targets sharing a batch): shorter
        prompts are right-padded to the longest — under the causal mask the padding cannot reach the scored positions.
        `slots` (one image slot per box, see set_image) lets the boxes belong to DIFFERENT resident images."""
        assert mode in ("segmentation", "detection")
        n_boxes = len(boxes_xywh)
        slot_arr = None if slots is None else np.asarray(list(slots), np.int32).reshape(-1)
        assert slot_arr is None or len(slot_arr) == n_boxes
        qs = [question] * n_boxes if isinstance(question, str) else list(question)
        assert len(qs) == n_boxes
        per_q = {q: self._ids(q) for q in dict.fromkeys(qs)}
        nv = min(min(len(v[2]) for v in per_q.values()), 8)
        Lmax = max(len(v[0]) for v in per_q.values())
        if Lmax > self.cfg.max_text_len:
            raise ValueError(f"prompt of {Lmax} tokens exceeds max_text_len={self.cfg.max_text_len}")
        if getattr(self.cfg, "llm_w8a8", 0):
            Lmax = w8a8_padded_len(Lmax, self.cfg.n_img_tokens, self.cfg.max_text_len)
        ids_rows = np.zeros((n_boxes, Lmax), np.int32)
        loc_rows = np.zeros((n_boxes,), np.int32)
        ver_rows = np.zeros((n_boxes, nv), np.int32)
        tok_rows = np.zeros((n_boxes, nv), np.int32)
        for i, q in enumerate(qs):
            ids, loc_pos, ver_pos, ver_tok = per_q[q]
            ids_rows[i, :len(ids)] = ids
            loc_rows[i] = loc_pos
            ver_rows[i] = ver_pos[-nv:]
            tok_rows[i] = ver_tok[-nv:]
        xyxy = np.asarray([[int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])] for b in boxes_xywh], np.int32)
        n = len(xyxy)

        def score_chunk(sel, out_dev):
            kw = {"out_dev": out_dev} if out_dev is not None else {}
            if slot_arr is not None:
                kw["slots"] = slot_arr[sel]
            return self.engine.score_boxes(xyxy[sel], ids_rows[sel], loc_rows[sel], verify_pos=ver_rows[sel], raw=True, **kw)
        records = self._score_boxes_grouped(xyxy, qs, per_q, nv, slot_arr) if self.group_prompts else None
        if records is None:
            records = self._score_sharded(n, score_chunk)
        res = self.engine.unpack(records, nv)
        self.last_template_ok = (res["tf_argmax"] == tok_rows).all(axis=1)
        out: List = []
        for b in range(n):
            w, h = int(xyxy[b, 2] - xyxy[b, 0]), int(xyxy[b, 3] - xyxy[b, 1])
            low = res["low_res_masks"][b, 0]
            heat = torch.from_numpy(self.engine.upsample_mask(low, h, w)) if upsample else torch.from_numpy(low.copy())
            if mode == "segmentation":
                out.append(heat)
            else:
                out.append((torch.from_numpy(res["pred_boxes"][b].copy()),
                            _scores(res["pred_logits"][b]), heat))
        # the fallback decodes from the host-side crop (bit-identical pixels: test_gpu_preprocess_is_bit_identical...)
        def img_of(b):
            im = self._image if slot_arr is None else getattr(self, "_images", {}).get(int(slot_arr[b]))
            if im is None:
                raise RuntimeError("decode fallback needs the host copy of the image, but slot "
                                   f"{0 if slot_arr is None else int(slot_arr[b])} was released (release_image) — call set_image again")
            return im
        self._handle_mismatches(out, lambda b: img_of(b).crop(tuple(int(v) for v in xyxy[b])), qs, mode, upsample,
                                defer_mismatch)
        return out

    # several prompts on the same crop share the LLaMA prefix (vstar_vsm_score_grouped).  False = plain batches; True = group the
    # crops that appear with >= 2 prompts in a call; "always" = every locate-template prompt goes through the grouped entry point,
    # also alone, so that a (crop, prompt) record never depends on what else was in the call (visual_search_many's lock-step mode)
    group_prompts = True

    def _template_lcp(self) -> List[int]:
        """Token ids shared by ALL locate prompts (system prompt, image token, "Please locate the"): the common start of the
        prompts of two object names that differ from their first token on.  The grouped layout always splits a prompt HERE, never
        at the longest common prefix of whatever prompts happen to share a call, so a record does not depend on its company."""
        if getattr(self, "_tpl", None) is None:
            a = list(map(int, self._ids(LOCATE_QUESTION.format("zebra"))[0]))
            b = list(map(int, self._ids(LOCATE_QUESTION.format("anchor"))[0]))
            n = 0
            while n < min(len(a), len(b)) and a[n] == b[n]:
                n += 1
            self._tpl = a[:n]
        return self._tpl

    def _score_boxes_grouped(self, xyxy: np.ndarray, qs: List[str], per_q: dict, nv: int,
                             slot_arr: Optional[np.ndarray] = None) -> Optional[np.ndarray]:
        """Multi-target batches (visual_search_many scores the same crops for several targets): every crop that appears with
        T >= 2 distinct prompts is scored ONCE through the vision towers and the shared positions of the LLaMA sequence — system
        prompt, image tokens and the template's "Please locate the" — plus one 32-row suffix block per prompt
        (engine.score_grouped).  Returns the records in the caller's order, or None when the batch does not qualify (single
        prompt unless group_prompts == "always", a process group that shards crops, an engine without the entry point).
        Prompts that do not start with the locate template, or whose remainder exceeds 32 tokens, take the plain path."""
        if not hasattr(self.engine, "score_grouped") or self._dist()[0] > 1:
            return None
        always = self.group_prompts == "always"
        uq = list(per_q)
        if len(uq) < 2 and not always:
            return None
        tpl = self._template_lcp()
        lcp = len(tpl)
        if IMAGE_TOKEN_INDEX not in tpl:
            return None
        P = self.cfg.n_img_tokens
        Lc = lcp - 1 + P                                            # shared spliced positions
        seqs = {q: list(map(int, per_q[q][0])) for q in uq}
        ok = {q: sq[:lcp] == tpl and 1 <= len(sq) - lcp <= 32 and per_q[q][1] >= Lc and min(per_q[q][2][-nv:], default=Lc) >= Lc
              for q, sq in seqs.items()}
        if not any(ok.values()):
            return None
        Ls = max(len(seqs[q]) - lcp for q in uq if ok[q])
        info = {}
        for q in uq:
            if ok[q]:
                sq = seqs[q]
                _, loc_pos, ver_pos, _ = per_q[q]
                info[q] = (sq[lcp:] + [0] * (Ls - (len(sq) - lcp)), loc_pos - Lc, [v - Lc for v in ver_pos[-nv:]])
        # crops -> the prompts they are scored for (in first-seen order); group crops with the same prompt tuple
        by_box: dict = {}
        single: List[int] = []
        keys = list(map(tuple, xyxy.tolist())) if slot_arr is None else \
            [tuple(b) + (int(sl),) for b, sl in zip(xyxy.tolist(), slot_arr.tolist())]     # a crop = (box, image slot)
        for i, (b, q) in enumerate(zip(keys, qs)):
            if ok[q]:
                by_box.setdefault(b, {}).setdefault(q, []).append(i)
            else:
                single.append(i)
        # crops are batched by HOW MANY prompts they carry, not by which ones: the suffix ids are per (crop, prompt), so crops of
        # different images with different targets share one call.  (Round 3 grouped by the exact prompt tuple: a window of 32
        # searches for 32 different objects became 32 one-crop calls — ADVICE r3.)
        by_T: dict = {}
        for b, d in by_box.items():
            by_T.setdefault(len(d), []).append(b)
        if not always and all(T < 2 for T in by_T):
            return None
        records = np.zeros((len(qs), RESULT_FLOATS), np.float32)
        prefix = np.asarray(tpl, np.int32)
        mb = self.cfg.max_batch
        rows_cap = mb * (self.cfg.max_text_len - 1 + P)             # activation rows the engine holds
        R0 = (Lc + 127) // 128 * 128
        for T, boxes in by_T.items():
            if (T < 2 and not always) or T > mb or R0 + 32 * T > rows_cap:
                single += [i for b in boxes for q in by_box[b] for i in by_box[b][q]]
                continue
            per_call = max(1, min(mb // T, rows_cap // (R0 + 32 * T)))
            for c0 in range(0, len(boxes), per_call):
                chunk = boxes[c0:c0 + per_call]
                G = len(chunk)
                suf = np.asarray([[info[q][0] for q in by_box[b]] for b in chunk], np.int32).reshape(G, T, Ls)
                loc_in = np.asarray([[info[q][1] for q in by_box[b]] for b in chunk], np.int32).reshape(G, T)
                ver_in = np.asarray([[info[q][2] for q in by_box[b]] for b in chunk], np.int32).reshape(G, T, nv)
                t1 = time.perf_counter()
                _lib_boxes = np.asarray([c[:4] for c in chunk], np.int32)
                if slot_arr is None:
                    self.engine.preprocess_boxes(_lib_boxes)
                else:
                    self.engine.preprocess_boxes(_lib_boxes, np.asarray([c[4] for c in chunk], np.int32))
                rec = self.engine.score_grouped(None, None, prefix, suf, loc_in, ver_in if nv else None, raw=True, internal_pixels=True)
                self.timers["engine_s"] += time.perf_counter() - t1
                self.timers["crops"] += G * T
                self.timers["engine_calls"] = self.timers.get("engine_calls", 0) + 1
                self.timers["grouped_records"] = self.timers.get("grouped_records", 0) + G * T
                for gi, b in enumerate(chunk):
                    for t, q in enumerate(by_box[b]):
                        for i in by_box[b][q]:
                            records[i] = rec[gi * T + t]
        if single:
            single = sorted(single)
            sel_all = np.asarray(single)
            ids_rows = np.zeros((len(single), max(len(per_q[qs[i]][0]) for i in single)), np.int32)
            for k, i in enumerate(single):
                ids = per_q[qs[i]][0]
                ids_rows[k, :len(ids)] = ids
            for s0 in range(0, len(single), mb):
                sl = slice(s0, s0 + mb)
                idx = sel_all[sl]
                t1 = time.perf_counter()
                skw = {} if slot_arr is None else {"slots": slot_arr[idx]}
                records[idx] = self.engine.score_boxes(xyxy[idx], ids_rows[sl], np.asarray([per_q[qs[i]][1] for i in idx], np.int32),
                                                       verify_pos=np.asarray([per_q[qs[i]][2][-nv:] for i in idx], np.int32), raw=True, **skw)
                self.timers["engine_s"] += time.perf_counter() - t1
                self.timers["crops"] += len(idx)
                self.timers["engine_calls"] = self.timers.get("engine_calls", 0) + 1
        return records

    def heatmap_stats(self, low_res, h: int, w: int, rects_xywh=None) -> np.ndarray:
        """On-device decision statistics of a heat map (no full-resolution materialisation)."""
        low = low_res.numpy() if isinstance(low_res, torch.Tensor) else np.asarray(low_res)
        t0 = time.perf_counter()
        out = self.engine.heatmap_stats(low, h, w, rects_xywh)
        self.timers["post_s"] += time.perf_counter() - t0
        return out

    def heatmap_stats_batch(self, items) -> List[np.ndarray]:
        """Several heatmap_stats in one engine call: items = [(low_res, h, w, rects_xywh), ...]."""
        t0 = time.perf_counter()
        conv = [(m.numpy() if isinstance(m, torch.Tensor) else np.asarray(m), h, w, r) for m, h, w, r in items]
        out = self.engine.heatmap_stats_batch(conv) if hasattr(self.engine, "heatmap_stats_batch") else \
            [self.engine.heatmap_stats(m, h, w, r) for m, h, w, r in conv]
        self.timers["post_s"] += time.perf_counter() - t0
        return out

    def _handle_mismatches(self, out: List, crop_of, question, mode: str, upsample: bool, defer: bool) -> None:
        """Per-crop consequence of the teacher-forced template check (`last_template_ok`).

        The single-prefill result is exact only if greedy decoding emits "Sure, [LOC]." (module docstring).  For a crop where
        it would not, the reference's result is whatever `generate()` produces (VSM.py:451-473): the engine therefore falls
        back to the stepwise greedy decode for THAT crop — `_decode_fallback` — and raises the reference's IndexError when no
        [LOC] is emitted.  `strict_template=False` (seeded random weights, whose decode is noise) keeps the teacher-forced
        result and warns instead."""
        ok = self.last_template_ok
        if ok is None or ok.all():
            return
        bad = [int(b) for b in np.nonzero(~ok)[0]]
        if not self.strict_template:
            warnings.warn(f"{len(bad)}/{len(out)} crops: greedy decoding would not emit '{ANSWER_TEMPLATE}' (teacher-forced "
                          "argmax check failed) - tolerated because strict_template=False (synthetic weights)")
            return
        for b in bad:
            q = question if isinstance(question, str) else question[b]
            fn = (lambda b=b, q=q: self._decode_fallback(crop_of(b), q, mode, upsample))
            out[b] = DeferredMismatch(fn) if defer else fn()

    @torch.inference_mode()
    def _decode_fallback(self, image: Image.Image, question: str, mode: str, upsample: bool = True):
        """Reference semantics for a crop whose greedy decode is NOT the template (VSM.py:451-553 + visual_search.py:208-225):
        decode stepwise (KV-cached greedy = the tokens `generate(use_cache=False)` emits), find the [LOC] tokens in the output,
        and score the crop with the GENERATED answer teacher-forced — under causal attention the hidden state in front of a
        [LOC] equals the one of the reference's last decode step.  Like the reference, boxes/logits come from the FIRST [LOC]
        (`det_result[...][0]`) and the mask from the LAST (`pred_mask[-1]`); no [LOC] at all -> IndexError (`pred_mask[-1]` on
        an empty tensor)."""
        prompt_ids = tokenizer_image_token(build_prompt(question, self.use_mm_start_end, conv_type=self.conv_type), self.vsm_tokenizer)
        gen = self.generate_ids(image, question, max_new_tokens=100)
        locs = [i for i, t in enumerate(gen) if t == self.loc_token_idx]
        self.fallback_log.append({"question": question, "generated": list(gen), "loc_positions": locs})
        if not locs:
            raise IndexError("index -1 is out of bounds for dimension 0 with size 0 "
                             "(greedy decoding emitted no [LOC] token: visual_search.py:209-225 fails the same way)")
        P = self.cfg.n_img_tokens
        ids = prompt_ids + list(gen[:locs[-1] + 1])         # tokens after the last [LOC] cannot influence it (causal)
        if len(ids) > self.cfg.max_text_len:
            raise ValueError(f"prompt + generated answer ({len(ids)} tokens) exceeds max_text_len={self.cfg.max_text_len}")
        pos = lambda k: len(prompt_ids) + k - 1 + (P - 1)   # spliced position of the state that predicts gen[k]  # noqa: E731
        rows = [locs[0]] if locs[0] == locs[-1] else [locs[0], locs[-1]]
        B = len(rows)
        clip = torch.from_numpy(clip_preprocess(image, self.cfg.clip_image_size)).bfloat16()[None].repeat(B, 1, 1, 1)
        owl = torch.from_numpy(owl_preprocess(image, self.cfg.owl_image_size)).bfloat16()[None].repeat(B, 1, 1, 1)
        nv = min(locs[-1] + 1, 8)
        ver_k = list(range(locs[-1] + 1 - nv, locs[-1] + 1))
        res = self.engine.score_batch(clip, owl, np.tile(np.asarray(ids, np.int32)[None], (B, 1)),
                                      np.asarray([pos(k) for k in rows], np.int32),
                                      verify_pos=np.tile(np.asarray([pos(k) for k in ver_k], np.int32)[None], (B, 1)))
        if not (res["tf_argmax"][0] == np.asarray([gen[k] for k in ver_k], np.int32)).all():
            warnings.warn("stepwise decode and teacher-forced prefill disagree on an arg-max (near-tie under bf16 rounding)")
        w, h = image.size
        low = res["low_res_masks"][B - 1, 0]
        heat = torch.from_numpy(self.engine.upsample_mask(low, h, w)) if upsample else torch.from_numpy(low.copy())
        if mode == "segmentation":
            return heat
        return (torch.from_numpy(res["pred_boxes"][0].copy()), _scores(res["pred_logits"][0]), heat)

    @torch.inference_mode()
    def generate_ids(self, image: Image.Image, question: str, max_new_tokens: int = 100, use_cache: bool = True) -> List[int]:
        """Greedy decoding for mode='vqa' (VSM.py:451-458, max_new_tokens=100 from visual_search.py:204).  Stops at EOS.
        use_cache=True (default): prompt prefilled once, then one KV-cached decode step per token on the engine
        (vstar_vsm_generate).  use_cache=False: the reference's literal schedule (generate(use_cache=False)): every new token
        costs one full CLIP + LLaMA prefill over the sequence so far.  Both return the same arg-max tokens."""
        ids = tokenizer_image_token(build_prompt(question, self.use_mm_start_end, conv_type=self.conv_type), self.vsm_tokenizer)
        clip = torch.from_numpy(clip_preprocess(image, self.cfg.clip_image_size)).bfloat16()[None]
        P = self.cfg.n_img_tokens
        eos = getattr(self.vsm_tokenizer, "eos_token_id", 2)
        if use_cache and hasattr(self.engine, "generate"):
            room = self.cfg.max_text_len - len(ids)
            if room <= 0:
                return []
            return self.engine.generate(clip, ids, min(max_new_tokens, room), eos)
        new: List[int] = []
        for _ in range(max_new_tokens):
            if len(ids) >= self.cfg.max_text_len:
                break
            last = len(ids) - 1 + (P - 1)          # spliced position of the last token
            res = self.engine.score_batch(clip, None, np.asarray([ids], np.int32), np.asarray([last], np.int32),
                                          verify_pos=np.asarray([[last]], np.int32), skip_owl=True)
            nxt = int(res["tf_argmax"][0, 0])
            ids.append(nxt)
            new.append(nxt)
            if nxt == eos:
                break
        return new

    def _gen_text(self, new: List[int]) -> str:
        text = self.vsm_tokenizer.batch_decode([new], skip_special_tokens=True)[0]
        return text.replace("\n", "").replace("  ", " ").strip()      # visual_search.py:217-219

    @torch.inference_mode()
    def generate(self, image: Image.Image, question: str, max_new_tokens: int = 100) -> str:
        return self._gen_text(self.generate_ids(image, question, max_new_tokens))

    # ---- the same decode for several crops at once (vstar_vsm_generate_batch): the cue questions of a stream round ----
    def _gen_requests(self, questions, n: int, max_new_tokens: int):
        """Per request the prompt ids and the cap min(max_new_tokens, max_text_len - len(ids)) of generate_ids (<= 0: no room)."""
        qs = [questions] * n if isinstance(questions, str) else list(questions)
        assert len(qs) == n
        per_q = {q: tokenizer_image_token(build_prompt(q, self.use_mm_start_end, conv_type=self.conv_type), self.vsm_tokenizer)
                 for q in dict.fromkeys(qs)}
        prompts = [per_q[q] for q in qs]
        return prompts, [min(max_new_tokens, self.cfg.max_text_len - len(p)) for p in prompts]

    def _generate_chunks(self, n: int, prompts, caps, chunk: int, run) -> List[List[int]]:
        """run(sel, prompts, caps) -> token lists for the requests `sel` that have room, at most `chunk` per engine call."""
        out: List[List[int]] = [[] for _ in range(n)]
        live = [i for i in range(n) if caps[i] > 0]
        eos = getattr(self.vsm_tokenizer, "eos_token_id", 2)
        for c0 in range(0, len(live), chunk):
            sel = live[c0:c0 + chunk]
            t0 = time.perf_counter()
            toks = run(sel, [prompts[i] for i in sel], [caps[i] for i in sel], eos)
            self.timers["generate_s"] = self.timers.get("generate_s", 0.0) + time.perf_counter() - t0
            self.timers["generate_tokens"] = self.timers.get("generate_tokens", 0) + sum(len(t) for t in toks)
            self.timers["generate_calls"] = self.timers.get("generate_calls", 0) + 1
            for i, t in zip(sel, toks):
                out[i] = t
        return out

    @torch.inference_mode()
    def generate_ids_batch(self, images: Sequence[Image.Image], questions, max_new_tokens: int = 100) -> List[List[int]]:
        """generate_ids for several host crops in one batched decode: entry i is generate_ids(images[i], question i)."""
        n = len(images)
        prompts, caps = self._gen_requests(questions, n, max_new_tokens)

        def run(sel, pr, cp, eos):
            clip = torch.from_numpy(np.stack([clip_preprocess(images[i], self.cfg.clip_image_size) for i in sel])).bfloat16()
            return self.engine.generate_batch(clip, pr, cp, eos)
        return self._generate_chunks(n, prompts, caps, GEN_MAX_BATCH, run)

    @torch.inference_mode()
    def generate_boxes(self, boxes_xywh: Sequence[Sequence[float]], questions, slots: Optional[Sequence[int]] = None,
                       max_new_tokens: int = 100) -> List[str]:
        """generate() for crops `image.crop((int(x), int(y), int(x+w), int(y+h)))` of resident images (set_image; `slots`: one
        image slot per box, None = slot 0), cut and preprocessed on the GPU and decoded together.  `questions`: one string or one
        per box.  More than min(16, max_batch) requests run in chunks.  With several ranks every rank decodes the whole batch: the
        tokens are deterministic, so there is nothing to exchange."""
        n = len(boxes_xywh)
        prompts, caps = self._gen_requests(questions, n, max_new_tokens)
        xyxy = np.asarray([[int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1] + b[3])] for b in boxes_xywh], np.int32).reshape(-1, 4)
        slot_arr = None if slots is None else np.asarray(list(slots), np.int32).reshape(-1)
        assert slot_arr is None or len(slot_arr) == n

        def run(sel, pr, cp, eos):
            self.engine.preprocess_boxes(xyxy[sel], None if slot_arr is None else slot_arr[sel])
            return self.engine.generate_batch(None, pr, cp, eos, internal_pixels=True)
        new = self._generate_chunks(n, prompts, caps, min(GEN_MAX_BATCH, int(self.cfg.max_batch)), run)
        return [self._gen_text(t) if caps[i] > 0 else "" for i, t in enumerate(new)]

    @torch.inference_mode()
    def inference(self, image: Image.Image, question: str, mode: str = "segmentation"):
        """Same contract as the reference's VSM.inference (visual_search.py:174-225)."""
        return self.inference_batch([image], question, mode)[0]

    def upsample_heatmap(self, low_res, h: int, w: int) -> torch.Tensor:
        """192x192 mask logits -> [h, w] heatmap, bilinear align_corners=False + clamp(min=0), on the GPU
        (VSM.py:534-537 + visual_search.py:223-224)."""
        low = low_res.numpy() if isinstance(low_res, torch.Tensor) else np.asarray(low_res)
        t0 = time.perf_counter()
        out = torch.from_numpy(self.engine.upsample_mask(low, h, w))
        self.timers["post_s"] += time.perf_counter() - t0
        return out
