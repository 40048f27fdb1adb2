"""`VQA_LLM` — drop-in for the reference class of the same name (vstar_bench_eval.py:38-165) on the HIP engine.

Same constructor role, same methods and return conventions:
    get_patch / get_object_crop ............ vstar_bench_eval.py:49-77
    free_form_inference(image, question, ...) -> str ................ :78-113   (temperature 0: greedy; > 0: sampled on the device)
    multiple_choices_inference(image, question, options, ...) -> int  :115-165  (shared-prefix option scoring)
plus `score_continuations` / `option_losses_batch` / `multiple_choices_batch`, the same scoring for many questions per engine call
with the log-likelihoods reduced on the device, and a batched form (`free_form_batch`) that decodes many samples in one engine call per step — the reference runs batch 1; on an MI355X a decode step is bound by the 13.5 GB weight sweep, so sequences are
advanced together.

MI355X-first differences that do not change results: the question prefix of the multiple-choice scoring is prefilled
once and every option forks its KV slot (no copy, no re-prefill); image/object features stay in HBM and are spliced by
row index; only the logits rows that are needed come back to the host.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from PIL import Image

from ._lib import VqaSampling, VqaWarpers
from .config import IMAGE_TOKEN_INDEX, OBJECT_TOKEN_INDEX, VQAConfig
from .logits import BEAM_RULES_MESSAGE, LogitRules, rules_from_kwargs
from .preprocess import CLIP_MEAN, CLIP_STD, SyntheticTokenizer, _normalise
from .vqa_engine import Seq, TokenLogprobs, VqaEngine, check_logprobs

DEFAULT_IMAGE_TOKEN = "<image>"
DEFAULT_OBJECT_TOKEN = "<object>"

# conv_templates["v1"] = conv_vicuna_v1 (LLaVA/llava/conversation.py:252-262), SeparatorStyle.TWO (:51-60)
V1_SYSTEM = ("A chat between a curious user and an artificial intelligence assistant. "
             "The assistant gives helpful, detailed, and polite answers to the user's questions.")
V1_ROLES = ("USER", "ASSISTANT")
V1_SEP, V1_SEP2 = " ", "</s>"


def v1_prompt(user: str, answer: Optional[str] = None) -> str:
    ret = V1_SYSTEM + V1_SEP + V1_ROLES[0] + ": " + user + V1_SEP
    return ret + V1_ROLES[1] + (": " + answer + V1_SEP2 if answer else ":")


def tokenizer_image_object_token(prompt: str, tokenizer) -> List[int]:
    """Tokenises the text between the <image> / <object> markers separately and joins the pieces with the -200 / -300
    placeholders, keeping one BOS (LLaVA/llava/mm_utils.py:64-88)."""
    pieces: List[str] = []
    marks: List[int] = []
    for gi, group in enumerate(prompt.split(DEFAULT_IMAGE_TOKEN)):
        for oi, piece in enumerate(group.split(DEFAULT_OBJECT_TOKEN)):
            if pieces:
                # the reference's separator list is [image] + [object] * (n-1): the first boundary is the image one
                marks.append(IMAGE_TOKEN_INDEX if len(marks) == 0 else OBJECT_TOKEN_INDEX)
            pieces.append(piece)
    toks = [tokenizer(p).input_ids for p in pieces]
    bos = getattr(tokenizer, "bos_token_id", None)
    has_bos = bool(toks and toks[0] and toks[0][0] == bos)
    ids: List[int] = [bos] if has_bos else []
    for i, t in enumerate(toks):
        if i > 0:
            ids.append(marks[i - 1])
        ids.extend(t[1:] if has_bos else t)
    return ids


def resolve_seed(seed: Optional[int]) -> int:
    """The Philox key of a sampled decode: `seed` itself, or (None) one drawn from torch's default CPU generator."""
    if seed is None:
        return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    return int(seed)


def sampling_params(temperature: float, top_k: Optional[int] = 50, top_p: Optional[float] = None, seed: int = 0,
                    stream: int = 0, step: int = 0) -> VqaSampling:
    """One row's vstar_vqa_sampling record with HF 4.31's conventions: temperature > 0; top_k None / 0 = off (HF default 50);
    top_p None or >= 1 = off."""
    if not temperature > 0:
        raise ValueError(f"sampling needs temperature > 0, got {temperature}")
    top_k = 0 if top_k is None else int(top_k)
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0 (0 / None = off), got {top_k}")
    top_p = 1.0 if top_p is None else float(top_p)
    if not top_p >= 0:
        raise ValueError(f"top_p must be in [0, 1], got {top_p}")
    mask = (1 << 64) - 1
    return VqaSampling(temperature=float(temperature), top_k=min(top_k, 2 ** 31 - 1), top_p=min(top_p, 1.0),
                       step=step & 0xffffffff, seed=int(seed) & mask, stream=int(stream) & mask)


def warper_params(min_p: Optional[float] = None, typical_p: Optional[float] = None, epsilon_cutoff: Optional[float] = None,
                  eta_cutoff: Optional[float] = None) -> Optional[VqaWarpers]:
    """One row's vstar_vqa_warpers record with HF's conventions and validation: min_p None / 0 = off, else in
    [0, 1]; typical_p None or >= 1 = off, else > 0; epsilon_cutoff and eta_cutoff None / 0 = off, else in (0, 1).  None when all
    four are off: the caller then makes the plain call."""
    min_p = 0.0 if min_p is None else float(min_p)
    if not 0 <= min_p <= 1:
        raise ValueError(f"min_p must be in [0, 1] (0 / None = off), got {min_p}")
    typical_p = 1.0 if typical_p is None else float(typical_p)
    if not typical_p > 0:
        raise ValueError(f"typical_p must be > 0 (None or >= 1 = off), got {typical_p}")
    cut = {}
    for name, v in (("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)):
        v = 0.0 if v is None else float(v)
        if not 0 <= v < 1:
            raise ValueError(f"{name} must be in (0, 1) (0 / None = off), got {v}")
        cut[name] = v
    typical_p = min(typical_p, 1.0)
    if min_p == 0 and typical_p >= 1 and cut["epsilon_cutoff"] == 0 and cut["eta_cutoff"] == 0:
        return None
    return VqaWarpers(min_p=min_p, typical_p=typical_p, epsilon_cutoff=cut["epsilon_cutoff"], eta_cutoff=cut["eta_cutoff"])


def check_spec_tokens(d) -> int:
    """The draft length of a speculative decode: an integer in [0, 15] (0 = off)."""
    if isinstance(d, bool) or int(d) != d or not 0 <= int(d) <= 15:
        raise ValueError(f"the number of speculative draft tokens must be an integer in [0, 15], got {d!r}")
    return int(d)


CONTRAST_MAX_K = 32      # VSTAR_VQA_MAX_TOP_LOGPROBS: the candidates of one contrastive-search step


def check_contrast(penalty_alpha, top_k, *, sampled: bool, num_beams: int, speculative: int, rules, logprobs,
                   sampled_name: str = "temperature > 0") -> Optional[float]:
    """The contrastive-search arguments of free_form_batch / generate (HF: penalty_alpha > 0, top_k > 1, greedy, one beam): None when
    the mode is off (penalty_alpha None or 0), else alpha.  ValueError for a value out of range or a combination that contradicts
    itself, NotImplementedError for the combinations that are follow-ups."""
    if penalty_alpha is None:
        return None
    alpha = float(penalty_alpha)
    if not 0 <= alpha <= 1:
        raise ValueError(f"penalty_alpha must be in [0, 1] (None / 0 = off), got {penalty_alpha!r}")
    if alpha == 0:
        return None
    if top_k is None or isinstance(top_k, bool) or int(top_k) != top_k or not 2 <= int(top_k) <= CONTRAST_MAX_K:
        raise ValueError(f"top_k is the number of candidates of contrastive search (penalty_alpha > 0) and must be an integer in "
                         f"[2, {CONTRAST_MAX_K}], got {top_k!r} (the sampling default 50 has to be overridden, as with HF generate)")
    if speculative:
        raise ValueError("speculative decoding (speculative > 0) cannot be combined with contrastive search (penalty_alpha > 0)")
    if sampled:
        raise NotImplementedError(f"contrastive search (penalty_alpha > 0) with {sampled_name} is not implemented: HF's contrastive "
                                  "search is a greedy mode")
    if num_beams > 1:
        raise NotImplementedError("contrastive search (penalty_alpha > 0) with num_beams > 1 is not implemented")
    if rules is not None and rules.active:
        raise NotImplementedError("contrastive search (penalty_alpha > 0) with logits rules (repetition_penalty, no_repeat_ngram_size, "
                                  "bad_words_ids, min_new_tokens, suppress_tokens, allowed_tokens_fn) is not implemented: a follow-up")
    if logprobs is not None:
        raise NotImplementedError("contrastive search (penalty_alpha > 0) with logprobs is not implemented: a follow-up")
    return alpha


def check_guidance(guidance_scale, plausibility_beta=0, *, negative_given: bool = False, num_beams: int = 1, speculative: int = 0,
                   penalty_alpha=None):
    """The guidance arguments of free_form_batch / generate (HF: guidance_scale, negative_prompt_ids): None when the
    mode is off (guidance_scale None or 1, as in HF), else (gamma, log_beta) — the fp32 pair every guided engine call carries, log_beta
    = float32(log(plausibility_beta)), -inf for beta 0 (no plausibility cut).  ValueError for a value out of range (gamma negative or
    not finite, beta outside [0, 1]) and for a negative prompt or a plausibility_beta > 0 without a guidance_scale (negative_given:
    the caller got a negative_question / negative_image / negative_prompt_ids); NotImplementedError for the combinations that are
    out of scope: beam search, speculative decoding, contrastive search."""
    beta = float(plausibility_beta)
    if not 0 <= beta <= 1:
        raise ValueError(f"plausibility_beta must be in [0, 1] (0 = off), got {plausibility_beta!r}")
    if guidance_scale is None:
        if negative_given:
            raise ValueError("a negative prompt (negative_question / negative_image / negative_prompt_ids) needs a guidance_scale")
        if beta > 0:
            raise ValueError("plausibility_beta > 0 needs a guidance_scale")
        return None
    gamma = float(guidance_scale)
    if not 0 <= gamma <= float(np.finfo(np.float32).max):
        raise ValueError(f"guidance_scale must be finite and >= 0 (None / 1 = off), got {guidance_scale!r}")
    if gamma == 1:
        return None
    if num_beams > 1:
        raise NotImplementedError("guided decoding (guidance_scale) with num_beams > 1 is not implemented")
    if speculative:
        raise NotImplementedError("guided decoding (guidance_scale) with speculative decoding is not implemented")
    if penalty_alpha is not None and float(penalty_alpha) != 0:
        raise NotImplementedError("guided decoding (guidance_scale) with contrastive search (penalty_alpha > 0) is not implemented")
    with np.errstate(divide="ignore"):
        return gamma, float(np.float32(np.log(np.float64(beta))))


def _warp_kw(min_p, typical_p, epsilon_cutoff, eta_cutoff) -> dict:
    """The `warpers=` keyword of the engine's sampled calls; empty when all four are off (the plain call)."""
    w = warper_params(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    return {} if w is None else dict(warpers=w)


def _with_step(p: VqaSampling, step: int) -> VqaSampling:
    return VqaSampling(temperature=p.temperature, top_k=p.top_k, top_p=p.top_p, step=step & 0xffffffff, seed=p.seed,
                       stream=p.stream)


class _ImageProcessor:
    """The slice of CLIPImageProcessor the evaluation touches (vstar_bench_eval.py:75-76,88,125,191)."""
    image_mean = list(CLIP_MEAN)
    image_std = list(CLIP_STD)

    def __init__(self, size: int = 224):
        self.crop_size = {"height": size, "width": size}
        self.size = size

    def preprocess(self, image: Image.Image, return_tensors: str = "pt"):
        img = image.convert("RGB")
        w, h = img.size
        short, long_ = (w, h) if w <= h else (h, w)
        ns, nl = self.size, int(self.size * long_ / short)
        nw, nh = (ns, nl) if w <= h else (nl, ns)
        img = img.resize((nw, nh), resample=Image.BICUBIC)
        left, top = (nw - self.size) // 2, (nh - self.size) // 2
        img = img.crop((left, top, left + self.size, top + self.size))
        return {"pixel_values": [torch.from_numpy(_normalise(np.asarray(img)))]}


class VQA_LLM:
    def __init__(self, args=None, cfg: Optional[VQAConfig] = None, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 tokenizer=None, engine: Optional[VqaEngine] = None, device: int = 0, decode_weight_bits: Optional[int] = None,
                 kv_cache_bits: Optional[int] = None):
        """args: the reference's namespace (vqa_model_path, conv_type).  With a local checkpoint directory the weights and
        tokenizer are read from it; offline pass `state_dict` (+ optionally `tokenizer`).  decode_weight_bits=8 builds the
        engine in the int8 weight-only decode mode, 4 in the int4 group-scaled mode (§8.6: translated to
        decode_weight_format=1 by VQAConfig.with_decode_bits); None = what `cfg` says, 0 by default.  kv_cache_bits=8 builds it
        with the block-scaled fp8 KV cache (§8.7; VQAConfig.with_kv_bits), independently of the weight mode; None = what `cfg` says."""
        import os
        from .weights import load_vqa_checkpoint_dir, vqa_config_from_dir
        path = getattr(args, "vqa_model_path", None) if args is not None else None
        real = engine is None and state_dict is None and path is not None and os.path.isdir(str(path))
        if real:                      # load_pretrained_model(model_path, None, name) (builder.py:26-151), local files only
            cfg = cfg or vqa_config_from_dir(path)
            state_dict = load_vqa_checkpoint_dir(path, getattr(args, "vision_tower", None))
            if tokenizer is None:
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(path, use_fast=False)
                tokenizer.add_tokens(["<im_patch>"], special_tokens=True)      # mm_use_im_patch_token default (builder.py:131-133)
        self.cfg = cfg or (engine.cfg if engine is not None else VQAConfig.seal_7b())
        if decode_weight_bits is not None and decode_weight_bits != self.cfg.decode_bits():
            if engine is not None:
                raise ValueError("decode_weight_bits is fixed when the engine is built: pass it in the engine's VQAConfig")
            self.cfg = self.cfg.with_decode_bits(decode_weight_bits)
        if kv_cache_bits is not None and kv_cache_bits != self.cfg.kv_bits():
            if engine is not None:
                raise ValueError("kv_cache_bits is fixed when the engine is built: pass it in the engine's VQAConfig")
            self.cfg = self.cfg.with_kv_bits(kv_cache_bits)
        self.conv_type = getattr(args, "conv_type", "v1") if args is not None else "v1"
        if self.conv_type != "v1":
            raise ValueError("only the 'v1' conversation template of the reference evaluation is implemented")
        self.tokenizer = tokenizer or SyntheticTokenizer(self.cfg.llm_vocab)
        self.image_processor = _ImageProcessor(self.cfg.clip_image_size)
        self.context_len = 2048
        if engine is None:
            if state_dict is None:
                raise FileNotFoundError(f"VQA-LLM checkpoint directory {path!r} not found and no state_dict given "
                                        "(there is no hub access here; the engine has no CPU fallback)")
            engine = VqaEngine(self.cfg, device)
            engine.load_state_dict(state_dict)
        self.engine = engine
        self.model = SimpleNamespace(config=SimpleNamespace(vocab_size=self.cfg.llm_vocab))
        self.eos_token_id = getattr(self.tokenizer, "eos_token_id", 2)
        self.spec_stats: Dict[str, int] = {}       # counters of the last speculative_decode (empty until one has run)

    # ---- vstar_bench_eval.py:49-77 ----
    def get_patch(self, bbox, image_width, image_height, patch_size=224, patch_scale=None):
        object_width, object_height = int(np.ceil(bbox[2])), int(np.ceil(bbox[3]))
        cx, cy = int(bbox[0] + bbox[2] / 2), int(bbox[1] + bbox[3] / 2)
        if patch_scale is None:
            pw, ph = max(object_width, patch_size), max(object_height, patch_size)
        else:
            pw, ph = int(object_width * patch_scale), int(object_height * patch_scale)
        left = max(0, cx - pw // 2)
        right = min(left + pw, image_width)
        top = max(0, cy - ph // 2)
        bottom = min(top + ph, image_height)
        return [left, top, right, bottom]

    def get_object_crop(self, image, bbox, patch_scale):
        box = self.get_patch(bbox, image.width, image.height, patch_scale=patch_scale)
        crop = image.crop((box[0], box[1], box[2], box[3]))
        crop = crop.resize((self.image_processor.crop_size["width"], self.image_processor.crop_size["height"]))
        return self.image_processor.preprocess(crop, return_tensors="pt")["pixel_values"][0]

    # ---- shared plumbing ----
    def _encode(self, image, object_crops, first_slot: int):
        """Features of one sample into consecutive feature slots: image first, then its object crops."""
        pix = [self.image_processor.preprocess(image, return_tensors="pt")["pixel_values"][0]]
        n_obj = 0
        if object_crops is not None and len(object_crops) > 0:
            pix += [torch.as_tensor(c) for c in object_crops]
            n_obj = len(object_crops)
        if first_slot + 1 + n_obj > self.cfg.max_images:
            raise ValueError(f"{1 + n_obj} images/object crops exceed the engine's feature table (max_images="
                             f"{self.cfg.max_images}); build the engine with a larger VQAConfig.max_images")
        self.engine.encode_images(torch.stack(pix, 0), first_slot)
        return [first_slot], list(range(first_slot + 1, first_slot + 1 + n_obj))

    def _question_rows(self, question: str, img_slots, obj_slots, images_long, objects_long, answer: Optional[str] = None):
        ids = tokenizer_image_object_token(v1_prompt(DEFAULT_IMAGE_TOKEN + "\n" + question, answer), self.tokenizer)
        return ids, self.engine.expand_ids(ids, img_slots, obj_slots, images_long, objects_long)

    # ---- free-form answer (vstar_bench_eval.py:78-113) ----
    def free_form_inference(self, image, question, temperature=0, top_p=None, num_beams=1, max_new_tokens=200,
                            object_crops=None, images_long=None, objects_long=None, *, top_k=50, seed=None, speculative=0,
                            draft_fn=None, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
                            suppress_tokens=None, allowed_tokens_fn=None, logprobs=None, min_p=None, typical_p=None,
                            epsilon_cutoff=None, eta_cutoff=None, penalty_alpha=None, guidance_scale=None, negative_question=None,
                            negative_image=None, plausibility_beta=0) -> str:
        """temperature 0: greedy (the evaluation's setting).  temperature > 0: model.generate(do_sample=True, temperature,
        top_k, top_p) as in HF 4.31, drawn on the device; `seed` (None: drawn from torch's default CPU generator,
        so torch.manual_seed makes runs reproducible) keys the Philox stream of the draws.  num_beams > 1 (temperature 0): HF
        4.31 beam search; beam sampling (num_beams > 1 with temperature > 0) is not implemented.
        min_p, typical_p, epsilon_cutoff, eta_cutoff: HF's warpers of these names, applied on the device behind top-k / top-p in
        HF's order (`warper_params`); ignored at temperature 0, as top_p is.
        speculative = d > 0: speculative decoding with up to d (<= 15) draft tokens per step from `draft_fn` (default: prompt
        lookup, vstar_amd/spec.py), greedy or sampled; 0 is the plain decode.
        repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_new_tokens, suppress_tokens, allowed_tokens_fn: HF generate's
        logits processors of these names (allowed_tokens_fn = prefix_allowed_tokens_fn), applied to the logits on the device ahead
        of the pick (vstar_amd/logits.py); the defaults mean no rules, and num_beams > 1 with a rule raises.
        logprobs = n in [0, 32]: self.generated_logprobs[0] then holds, per generated token, its log-probability and rank and the n
        best alternatives (`TokenLogprobs`), aligned with self.generated_ids[0]; the returned text is unchanged.
        penalty_alpha in (0, 1] (temperature 0, num_beams 1): HF 4.31 contrastive search with top_k (2 .. 32, to be given) candidates
        per step, the degeneration penalty and the pick on the device (`contrastive_decode`); None / 0: off.
        guidance_scale = gamma (None / 1: off, as in HF): guided decoding against a negative prompt (classifier-free guidance / visual
        contrastive decoding), greedy or sampled: a second sequence is decoded in lock-step in a KV slot of its own
        and every step's logits become gamma * (log_softmax(row) - log_softmax(negative row)) + log_softmax(negative row) on the device,
        ahead of the logits rules.  The negative prompt is the same v1 prompt of negative_question (None: the question) with every
        <image> / <object> placeholder left out (negative_image None: the language prior), or with negative_image (a PIL image) in
        place of the image, the object crops kept.  plausibility_beta in [0, 1] (0: off): tokens whose probability under the
        un-guided row is below beta times its maximum are dropped (-inf)."""
        return self.free_form_batch([dict(image=image, question=question, object_crops=object_crops, images_long=images_long,
                                          objects_long=objects_long)], max_new_tokens, temperature=temperature, top_p=top_p,
                                    top_k=top_k, seed=seed, num_beams=num_beams, speculative=speculative, draft_fn=draft_fn,
                                    repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                    bad_words_ids=bad_words_ids, min_new_tokens=min_new_tokens, suppress_tokens=suppress_tokens,
                                    allowed_tokens_fn=allowed_tokens_fn, logprobs=logprobs, min_p=min_p, typical_p=typical_p,
                                    epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, penalty_alpha=penalty_alpha,
                                    guidance_scale=guidance_scale, negative_question=negative_question, negative_image=negative_image,
                                    plausibility_beta=plausibility_beta)[0]

    def free_form_batch(self, samples: Sequence[dict], max_new_tokens: int = 200, *, temperature=0, top_p=None, top_k=50,
                        seed=None, num_beams: int = 1, length_penalty: float = 1.0, early_stopping=False, speculative: int = 0,
                        draft_fn=None, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words_ids=None, min_new_tokens=0,
                        suppress_tokens=None, allowed_tokens_fn=None, logprobs=None, min_p=None, typical_p=None,
                        epsilon_cutoff=None, eta_cutoff=None, penalty_alpha=None, guidance_scale=None, negative_question=None,
                        negative_image=None, plausibility_beta=0) -> List[str]:
        """Decode of several samples at once: one prefill call, then one engine call per generated position.  temperature 0:
        greedy; temperature > 0: sampled, sample i with seed samples[i].get("seed", seed + i) (stream 0), so element i equals a
        single free_form_inference call with that seed.  num_beams = k > 1: beam search, the k beams of sample i in KV slots
        i*k .. i*k+k-1 (n*k <= max_slots), one group per sample in every step's forward.  speculative = d > 0 (num_beams 1):
        `speculative_decode` with up to d drafts per sequence and step; 0 (default) is the plain path.  The logits rules
        (repetition_penalty .. allowed_tokens_fn, see free_form_inference) apply to every sample, sample i with batch_id i and
        its own history; all at their defaults: no edits are built and the engine calls are the plain ones.
        logprobs = n in [0, 32] (num_beams 1): self.generated_logprobs becomes a list with one `TokenLogprobs` per sample, aligned
        with self.generated_ids — per generated token its log-probability and rank under the (edited, un-warped) distribution it was
        picked from and the n best alternatives, computed on the device; None (default): self.generated_logprobs is
        None and the engine calls are the plain ones.  The returned texts are the same either way.
        min_p, typical_p, epsilon_cutoff, eta_cutoff (temperature > 0; ignored by the greedy decode): the further warpers of
        DESIGN.md §8.10 for every sample; all off (the default): the engine calls are the plain ones.
        penalty_alpha in (0, 1] (temperature 0, num_beams 1, no rules, no logprobs, not speculative): contrastive search with
        top_k (2 .. 32) candidates, the k candidate slots of sample i in KV slots i*k .. i*k+k-1 (n*k <= max_slots), one group per
        sample in every step's forward (`contrastive_decode`); None / 0 (default): off, every call is as before.
        guidance_scale, negative_question, negative_image, plausibility_beta (see free_form_inference; num_beams 1, not speculative, no
        penalty_alpha): sample i decodes in KV slot 2 i and its negative sequence in slot 2 i + 1 (2 n <= max_slots);
        both are prefilled in the one prefill call and take the chosen token at every step, in one engine call; a sample's dict may
        carry its own negative_question / negative_image.  A negative_image takes one more feature slot per sample.  None / 1
        (default): off, every call is as before."""
        cfg, eng = self.cfg, self.engine
        n = len(samples)
        if num_beams < 1:
            raise ValueError(f"num_beams must be >= 1, got {num_beams}")
        rules = rules_from_kwargs(repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_new_tokens, suppress_tokens,
                                  allowed_tokens_fn)
        if rules is not None and num_beams > 1:
            raise NotImplementedError(BEAM_RULES_MESSAGE)
        speculative = check_spec_tokens(speculative)
        neg_given = negative_question is not None or negative_image is not None or \
            any(s.get("negative_question") is not None or s.get("negative_image") is not None for s in samples)
        guide = check_guidance(guidance_scale, plausibility_beta, negative_given=neg_given, num_beams=num_beams, speculative=speculative,
                               penalty_alpha=penalty_alpha)
        if guide is not None and 2 * n > cfg.max_slots:
            raise ValueError(f"{n} guided samples need {2 * n} KV slots (one more per sample for its negative sequence); the engine "
                             f"has max_slots={cfg.max_slots} (build it with a larger VQAConfig.max_slots)")
        if speculative and num_beams > 1:
            raise ValueError("speculative decoding (speculative > 0) cannot be combined with beam search (num_beams > 1)")
        if num_beams > 1 and temperature > 0:
            raise NotImplementedError("beam sampling (num_beams > 1 with temperature > 0) is not implemented")
        if n * num_beams > cfg.max_slots:
            raise ValueError(f"{n} samples x {num_beams} beams need {n * num_beams} KV slots; the engine has max_slots="
                             f"{cfg.max_slots} (build it with a larger VQAConfig.max_slots)")
        if temperature < 0:
            raise ValueError(f"temperature must be >= 0 (0 = greedy), got {temperature}")
        logprobs = check_logprobs(logprobs)
        if logprobs is not None and num_beams > 1:
            raise NotImplementedError("logprobs with beam search (num_beams > 1) is not implemented: beam hypotheses carry their "
                                      "own scores, and exposing those is a follow-up")
        alpha = check_contrast(penalty_alpha, top_k, sampled=temperature > 0, num_beams=num_beams, speculative=speculative,
                               rules=rules, logprobs=logprobs)
        k_slots = int(top_k) if alpha is not None else 2 if guide is not None else num_beams      # KV slots per sample
        if alpha is not None and n * k_slots > cfg.max_slots:
            raise ValueError(f"{n} samples x {k_slots} candidates need {n * k_slots} KV slots; the engine has max_slots="
                             f"{cfg.max_slots} (build it with a larger VQAConfig.max_slots)")
        warp = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
        if temperature > 0:
            warper_params(**warp)                      # (validated before any engine work)
            base = resolve_seed(seed)
            params = [sampling_params(temperature, top_k, top_p, s.get("seed", base + i)) for i, s in enumerate(samples)]
        seqs, lens, id_lens, text_ids, neg_seqs = [], [], [], [], []
        fslot = 0
        for i, s in enumerate(samples):
            crops = s.get("object_crops")
            img_slots, obj_slots = self._encode(s["image"], crops, fslot)
            fslot += 1 + len(obj_slots)
            ids, rows = self._question_rows(s["question"], img_slots, obj_slots, s.get("images_long"), s.get("objects_long"))
            seqs.append(Seq(rows, kv_slot=i * k_slots))
            lens.append(len(rows))
            id_lens.append(len(ids))
            text_ids.append([t for t in ids if t >= 0])
            if guide is not None:
                neg_q, neg_img = s.get("negative_question", negative_question), s.get("negative_image", negative_image)
                nids = ids if neg_q is None else self._question_rows(neg_q, img_slots, obj_slots, s.get("images_long"), s.get("objects_long"))[0]
                if neg_img is None:       # the language prior: no image, no object crops
                    nrows = [t for t in nids if t >= 0]
                else:                     # the caller's degraded image in a feature slot of its own, the same crops
                    if fslot + 1 > cfg.max_images:
                        raise ValueError(f"the negative image needs one more feature slot than max_images={cfg.max_images}")
                    eng.encode_images(self.image_processor.preprocess(neg_img, return_tensors="pt")["pixel_values"][0][None], fslot)
                    nrows = eng.expand_ids(nids, [fslot], obj_slots, s.get("images_long"), s.get("objects_long"))
                    fslot += 1
                if len(nrows) > len(rows) and len(nrows) + max_new_tokens > cfg.max_ctx:
                    raise ValueError(f"the negative prompt ({len(nrows)} rows) plus max_new_tokens exceeds max_ctx={cfg.max_ctx}")
                neg_seqs.append(Seq(nrows, kv_slot=i * k_slots + 1))
        guide = None if guide is None else (neg_seqs,) + guide
        if alpha is not None:
            res = self.contrastive_decode(seqs, lens, max_new_tokens, alpha, k_slots)
        elif speculative:
            res = self.speculative_decode(seqs, lens, text_ids, max_new_tokens, speculative,
                                          params if temperature > 0 else None, draft_fn, rules, logprobs=logprobs,
                                          **(warp if temperature > 0 else {}))
        elif num_beams > 1:
            outs = self.beam_decode(seqs, lens, id_lens, max_new_tokens, num_beams, length_penalty, early_stopping)
            res = [o[0] for o in outs]
        elif temperature > 0:
            res = self.sample_decode(seqs, lens, max_new_tokens, params, rules, text_ids, logprobs=logprobs, guide=guide, **warp)
        else:
            res = self.greedy_decode(seqs, lens, max_new_tokens, rules, text_ids, logprobs=logprobs, guide=guide)
        self.generated_ids, self.generated_logprobs = res if logprobs is not None else (res, None)
        texts = []
        for ids in self.generated_ids:
            out = self.tokenizer.batch_decode([ids], skip_special_tokens=True)[0].strip()
            if out.endswith(V1_SEP2):
                out = out[:-len(V1_SEP2)]
            texts.append(out.strip())
        return texts

    def _edits(self, rules: Optional[LogitRules], rows):
        """The packed edits of one engine call: rows = one (history ids, n_generated, batch_id) per wanted row; None without
        active rules (the call is then the plain one)."""
        if rules is None or not rules.active:
            return None
        return LogitRules.pack([rules.plan(h, g, self.eos_token_id, b) for h, g, b in rows])

    def _with_negatives(self, guide, call):
        """The chooser of `_decode` for `call(step, want, idx, t, edits, **kw)`.  guide None: `call` itself.  guide = (neg_seqs, gamma,
        log_beta): every engine call also carries the negative sequence of each of its sequences — neg_seqs[i], the
        negative prompt of sequence i in a KV slot of its own, at the prefill; afterwards the same new token at the negative
        sequence's own position — with its last row wanted behind the output rows, and `guidance=` pairs output row j with it."""
        if guide is None:
            return call
        neg_seqs, gamma, log_beta = guide
        neg_pos = [s.past_len + len(s.rows) for s in neg_seqs]

        def choose(step, want, idx, t, edits):
            m = len(step)
            if t == 0:
                negs = [neg_seqs[i] for i in idx]
            else:
                negs = [Seq(list(step[j].rows), kv_slot=neg_seqs[i].kv_slot, past_len=neg_pos[i]) for j, i in enumerate(idx)]
                for i in idx:
                    neg_pos[i] += 1
            g = (np.arange(m, 2 * m, dtype=np.int32), np.float32(gamma), np.float32(log_beta))
            return call(list(step) + negs, list(want) + [(m + j, -1) for j in range(m)], idx, t, edits, guidance=g)
        return choose

    def greedy_decode(self, seqs: Sequence[Seq], lens: Sequence[int], max_new_tokens: int, rules: Optional[LogitRules] = None,
                      histories=None, logprobs=None, guide=None):
        """model.generate(do_sample=False, use_cache=True) for every sequence.  rules + histories, logprobs: see `_decode`; guide: see
        `_with_negatives` (None: the plain engine calls)."""
        if logprobs is None:
            return self._decode(seqs, lens, max_new_tokens, self._with_negatives(
                guide, lambda step, want, idx, t, edits, **kw: self.engine.forward(step, want, logits=False, edits=edits, **kw)[1]), rules, histories)
        return self._decode(seqs, lens, max_new_tokens, self._with_negatives(
            guide, lambda step, want, idx, t, edits, **kw: self.engine.forward(step, want, logits=False, edits=edits, logprobs=logprobs, **kw)[1:]),
            rules, histories, logprobs)

    def sample_decode(self, seqs: Sequence[Seq], lens: Sequence[int], max_new_tokens: int, params, rules: Optional[LogitRules] = None,
                      histories=None, logprobs=None, *, min_p=None, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, guide=None):
        """model.generate(do_sample=True, use_cache=True): params[i] (`_lib.VqaSampling`) drives sequence i; the Philox step
        of a draw is the index of the token it generates (0 = the token drawn from the prefill's last row).  rules + histories,
        logprobs: see `_decode`.  min_p .. eta_cutoff: `warper_params`, the same record for every sequence;
        all off: the engine calls are the plain ones.  guide: see `_with_negatives` (None: the plain engine calls)."""
        wkw = _warp_kw(min_p, typical_p, epsilon_cutoff, eta_cutoff)

        def choose(step, want, idx, t, edits, **kw):
            return self.engine.forward_sample(step, want, [_with_step(params[i], t) for i in idx], edits=edits, logprobs=logprobs, **wkw, **kw)
        return self._decode(seqs, lens, max_new_tokens, self._with_negatives(guide, choose), rules, histories, logprobs)

    def speculative_decode(self, seqs: Sequence[Seq], lens: Sequence[int], ids: Sequence[Sequence[int]], max_new_tokens: int,
                           d: int, params=None, draft_fn=None, rules: Optional[LogitRules] = None, logprobs=None, *, min_p=None,
                           typical_p=None, epsilon_cutoff=None, eta_cutoff=None):
        """Speculative decoding: greedy (params None) or sampled (params[i] drives sequence i as in
        `sample_decode`).  ids[i]: the un-expanded text ids of sequence i (placeholders left out) — what the drafter sees, with
        the generated tokens appended.  Every engine call feeds each live sequence the rows [cur, draft_0 .. draft_{k-1}] at
        past_len = pos, k <= d drafts from draft_fn (default `spec.prompt_lookup_draft`); the verify tail returns the accepted
        count a and a + 1 tokens, and pos += a + 1.  The rows of rejected drafts stay in the cache behind pos and are overwritten
        by the next call.  k is cut so that the sequence's context, the call's rows (max_rows, 256 wanted rows) and
        max_new_tokens are respected.  The tokens are those of the logits of the verify forward: greedy picks their arg-max,
        sampled draws follow their kept distribution.  rules (vstar_amd/logits.py): every wanted row's logits are
        edited ahead of its choice with the plan of ITS history — row r of a group sees ids[i] + out + drafts[:r] and n_generated
        = len(out) + r, what a plain decode would see once those drafts are accepted; batch_id = i.
        logprobs = n: returns (ids, records), records[i] a `TokenLogprobs` with one entry per generated token of sequence i — of a
        verify step the entries of the a + 1 tokens that hold (cut at an EOS like the tokens), the -1 rows dropped.
        min_p .. eta_cutoff (sampled only; greedy ignores them): `warper_params`, the same record for every row.
        self.spec_stats = calls / drafted / accepted / tokens of this run."""
        from .spec import prompt_lookup_draft
        cfg, eng = self.cfg, self.engine
        d = check_spec_tokens(d)
        draft_fn = draft_fn or prompt_lookup_draft
        if rules is not None and not rules.active:
            rules = None
        n = len(seqs)
        want0 = [(i, -1) for i in range(n)]
        ed0 = self._edits(rules, [(list(ids[i]), 0, i) for i in range(n)])
        logprobs = check_logprobs(logprobs)
        lpkw = {} if logprobs is None else dict(logprobs=logprobs)      # (without: the engine calls are the plain ones)
        if params is not None:
            lpkw.update(_warp_kw(min_p, typical_p, epsilon_cutoff, eta_cutoff))
        if params is None:
            first = eng.forward(seqs, want0, logits=False, edits=ed0, **lpkw)[1:]
        else:
            first = eng.forward_sample(seqs, want0, [_with_step(params[i], 0) for i in range(n)], edits=ed0, **lpkw)
            first = first if logprobs is not None else (first,)
        lps = [[first[1].rows(slice(i, i + 1))] for i in range(n)] if logprobs is not None else None
        first = first[0]
        stats = dict(calls=1, drafted=0, accepted=0, tokens=0)
        out: List[List[int]] = [[int(first[i])] for i in range(n)]
        pos = list(lens)
        row_cap = min(cfg.max_rows, 256)

        def alive(i):       # the stop rule of _decode: EOS, the token budget, or a full context
            return out[i][-1] != self.eos_token_id and len(out[i]) < max_new_tokens and pos[i] + 1 < cfg.max_ctx

        live = [i for i in range(n) if alive(i)]
        while live:
            spare = row_cap - len(live)                 # rows left for drafts once every live sequence has its current token
            step, wanted, groups, draft, prm, plan_rows = [], [], [0], [], [], []
            for j, i in enumerate(live):
                k = min(d, max_new_tokens - len(out[i]) - 1, cfg.max_ctx - pos[i] - 2, max(spare, 0))
                guess: List[int] = []
                if k > 0:
                    for t in list(draft_fn(list(ids[i]) + out[i], k))[:k]:
                        t = int(t)
                        if not 0 <= t < cfg.llm_vocab:   # a drafter's id the model does not have: the draft ends there
                            break
                        guess.append(t)
                spare -= len(guess)
                rows = [out[i][-1]] + guess
                step.append(Seq(rows, kv_slot=seqs[i].kv_slot, past_len=pos[i]))
                wanted += [(j, r) for r in range(len(rows))]
                groups.append(groups[-1] + len(rows))
                draft += guess + [-1]
                if params is not None:
                    prm += [_with_step(params[i], len(out[i]) + r) for r in range(len(rows))]
                stats["drafted"] += len(guess)
                if rules is not None:
                    base = list(ids[i]) + out[i]
                    plan_rows += [(base + guess[:r], len(out[i]) + r, i) for r in range(len(rows))]
            acc, tok, *rec = eng.forward_verify(step, wanted, groups, draft, prm if params is not None else None,
                                                edits=self._edits(rules, plan_rows), **lpkw)
            stats["calls"] += 1
            for j, i in enumerate(live):
                a = int(acc[j])
                new = [int(t) for t in tok[groups[j]:groups[j] + a + 1]]
                stats["accepted"] += a
                pos[i] += a + 1
                if self.eos_token_id in new:            # the sequence ends at its first EOS
                    new = new[:new.index(self.eos_token_id) + 1]
                out[i] += new
                if lps is not None:
                    lps[i].append(rec[0].rows(slice(groups[j], groups[j] + len(new))))
            live = [i for i in live if alive(i)]
        stats["tokens"] = sum(len(o) for o in out)
        self.spec_stats = stats
        if lps is not None:
            return out, [TokenLogprobs.concat(l, logprobs) for l in lps]
        return out

    def beam_decode(self, seqs: Sequence[Seq], lens: Sequence[int], id_lens: Sequence[int], max_new_tokens: int, num_beams: int,
                    length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1) -> List[List[List[int]]]:
        """model.generate(num_beams=k, do_sample=False) (HF 4.31 beam_search) for every sequence: seqs[i] (the
        prompt rows, prefilled into slot seqs[i].kv_slot = beam 0) owns slots kv_slot .. kv_slot+k-1; lens[i] = its KV rows,
        id_lens[i] = its un-expanded input_ids length (the lengths of the contract).  One forward per step advances the k beams of
        every unfinished sequence, the device returns each sequence's 2k candidates, the host scorer (vstar_amd/beam.py) picks
        the next beams and the KV ancestry is reordered — K/V never move.  Returns, per sequence, the num_return_sequences best
        generated id lists (EOS-terminated / EOS-padded as 4.31's finalize)."""
        from .beam import BeamSearch
        cfg, eng, k = self.cfg, self.engine, num_beams
        n = len(seqs)
        slots = [[s.kv_slot + b for b in range(k)] for s in seqs]
        if any(sl[-1] >= cfg.max_slots for sl in slots) or len({x for sl in slots for x in sl}) != n * k:
            raise ValueError(f"{n} sequences x {k} beams need {n * k} distinct KV slots below max_slots={cfg.max_slots}")
        if 2 * k > k * cfg.llm_vocab:
            raise ValueError("2 * num_beams candidates exceed num_beams x vocabulary")
        bs = [BeamSearch(k, id_lens[i], self.eos_token_id, id_lens[i] + max_new_tokens, length_penalty, early_stopping)
              for i in range(n)]
        goff = lambda m: np.arange(m + 1, dtype=np.int32) * k       # noqa: E731
        # start: the prompt's last row k times, scores [0, -1e9, ...] (4.31's beam_scores initialisation)
        cs, ct, cr, _ = eng.forward_beam([Seq(list(s.rows), kv_slot=s.kv_slot) for s in seqs], [(i, -1) for i in range(n) for _ in range(k)],
                                         np.concatenate([b.scores for b in bs]), goff(n), 2 * k)
        pos = list(lens)
        live = list(range(n))
        while live:
            dst, src = [], []
            for j, i in enumerate(live):
                parents = bs[i].process(cs[j], ct[j], cr[j])
                dst += slots[i]
                src += [slots[i][p] for p in parents]
            eng.kv_reorder(dst, src, 0, max(pos[i] for i in live))
            live = [i for i in live if not bs[i].done and len(bs[i].tokens[0]) < max_new_tokens and pos[i] + 1 < cfg.max_ctx]
            if not live:
                break
            step = [Seq([bs[i].tokens[b][-1]], kv_slot=slots[i][b], past_len=pos[i]) for i in live for b in range(k)]
            cs, ct, cr, _ = eng.forward_beam(step, [(j, 0) for j in range(len(step))], np.concatenate([bs[i].scores for i in live]),
                                             goff(len(live)), 2 * k)
            for i in live:
                pos[i] += 1
        return [b.finalize(num_return_sequences) for b in bs]

    def contrastive_decode(self, seqs: Sequence[Seq], lens: Sequence[int], max_new_tokens: int, alpha: float, k: int) -> List[List[int]]:
        """model.generate(penalty_alpha=alpha, top_k=k, do_sample=False) (HF 4.31 contrastive_search) for every
        sequence: seqs[i] (the prompt rows) is prefilled into its slot seqs[i].kv_slot, the OWNER, and owns the slots kv_slot ..
        kv_slot+k-1.  The begin call fills the owner's hidden history and returns the k most probable first tokens; every further
        engine call feeds the k candidates of every unfinished sequence as k one-row forks of its owner — candidate c writes slot
        kv_slot+c — and on the device takes their degeneration penalty against the history, picks the winner, appends its hidden
        row, moves its K/V row into the owner and returns the winner's index and its k next candidates: one engine call per
        generated position, T tokens = one prefill + T steps.  alpha = 0 is the greedy decode.  A sequence stops at EOS, at
        max_new_tokens or when its context is full."""
        cfg, eng, k = self.cfg, self.engine, int(k)
        n = len(seqs)
        if not 0 <= alpha <= 1:
            raise ValueError(f"alpha must be in [0, 1], got {alpha!r}")
        if not 2 <= k <= CONTRAST_MAX_K:
            raise ValueError(f"k must be in [2, {CONTRAST_MAX_K}], got {k}")
        slots = [[s.kv_slot + c for c in range(k)] for s in seqs]
        if any(sl[-1] >= cfg.max_slots for sl in slots) or len({x for sl in slots for x in sl}) != n * k:
            raise ValueError(f"{n} sequences x {k} candidates need {n * k} distinct KV slots below max_slots={cfg.max_slots}")
        tok, prob = eng.forward_contrast_begin([Seq(list(s.rows), kv_slot=s.kv_slot) for s in seqs], [(i, -1) for i in range(n)], k)
        cand = {i: (tok[i].copy(), prob[i].copy()) for i in range(n)}
        out: List[List[int]] = [[] for _ in range(n)]
        pos = list(lens)
        live = [i for i in range(n) if max_new_tokens > 0 and pos[i] < cfg.max_ctx]
        while live:
            step = [Seq([int(cand[i][0][c])], kv_slot=slots[i][c], past_len=pos[i], prefix_slot=slots[i][0]) for i in live for c in range(k)]
            sel, ntok, nprob = eng.forward_contrast_step(step, np.arange(len(live) + 1, dtype=np.int32) * k,
                                                         np.concatenate([cand[i][1] for i in live]), alpha, k)
            for j, i in enumerate(live):
                out[i].append(int(cand[i][0][int(sel[j])]))
                cand[i] = (ntok[j].copy(), nprob[j].copy())
                pos[i] += 1
            live = [i for i in live if out[i][-1] != self.eos_token_id and len(out[i]) < max_new_tokens and pos[i] < cfg.max_ctx]
        return out

    def _decode(self, seqs: Sequence[Seq], lens: Sequence[int], max_new_tokens: int, choose, rules: Optional[LogitRules] = None,
                histories=None, logprobs=None):
        """The generate() loop over a token chooser choose(step_seqs, want, sequence indices, token index, edits) -> tokens; a
        sequence stops at EOS (the reference's keyword criterion stops on '</s>', the decoded EOS) or when the context is full.
        rules (active) need histories[i], the text ids of sequence i's prompt with the placeholders left out: every step builds
        one plan per wanted row from histories[i] + what i has generated (batch_id = i) and hands the packed edits to `choose`;
        without rules `edits` is None and the engine calls are the plain ones.
        logprobs = n: `choose` returns (tokens, `TokenLogprobs`) and the result is (ids, records), records[i] holding one entry per
        generated token of sequence i."""
        cfg = self.cfg
        logprobs = check_logprobs(logprobs)
        n = len(seqs)
        if rules is not None and not rules.active:
            rules = None
        if rules is not None and (histories is None or len(histories) != n):
            raise ValueError("logits rules need one history (the prompt's text ids) per sequence")
        nxt = choose(seqs, [(i, -1) for i in range(n)], list(range(n)), 0,
                     self._edits(rules, [(histories[i], 0, i) for i in range(n)]) if rules is not None else None)
        if logprobs is not None:
            nxt, rec = nxt
            lps = [[] for _ in range(n)]
            curlp = {i: rec.rows(slice(i, i + 1)) for i in range(n)}
        out: List[List[int]] = [[] for _ in range(n)]
        pos = list(lens)
        live = list(range(n))
        cur = {i: int(nxt[i]) for i in range(n)}
        for _ in range(max_new_tokens):
            still = []
            for i in live:
                out[i].append(cur[i])
                if logprobs is not None:
                    lps[i].append(curlp[i])
                if cur[i] != self.eos_token_id and pos[i] + 1 < cfg.max_ctx:
                    still.append(i)
            live = still
            if not live or len(out[live[0]]) >= max_new_tokens:
                break
            step = [Seq([cur[i]], kv_slot=seqs[i].kv_slot, past_len=pos[i]) for i in live]
            nxt = choose(step, [(j, 0) for j in range(len(live))], live, len(out[live[0]]),
                         self._edits(rules, [(list(histories[i]) + out[i], len(out[i]), i) for i in live]) if rules is not None else None)
            if logprobs is not None:
                nxt, rec = nxt
            for j, i in enumerate(live):
                cur[i] = int(nxt[j])
                pos[i] += 1
                if logprobs is not None:
                    curlp[i] = rec.rows(slice(j, j + 1))
        if logprobs is not None:
            return out, [TokenLogprobs.concat(l, logprobs) for l in lps]
        return out

    # ---- multiple choice (vstar_bench_eval.py:115-165) ----
    def multiple_choices_inference(self, image, question, options, object_crops=None, images_long=None,
                                   objects_long=None) -> int:
        losses = self.option_losses(image, question, options, object_crops, images_long, objects_long)
        return int(torch.stack(losses).argmin().item())

    def option_losses(self, image, question, options, object_crops=None, images_long=None, objects_long=None):
        eng, cfg = self.engine, self.cfg
        if 1 + len(options) > cfg.max_slots:
            raise ValueError("more options than KV slots")
        img_slots, obj_slots = self._encode(image, object_crops, 0)
        q_ids, q_rows = self._question_rows(question, img_slots, obj_slots, images_long, objects_long)
        q_logits, _ = eng.forward([Seq(q_rows, kv_slot=0)], [(0, -1)])
        P = len(q_rows)
        seqs, want, opt_ids = [], [], []
        for j, option in enumerate(options):
            full_ids, _ = self._question_rows(question, img_slots, obj_slots, images_long, objects_long, answer=option)
            ids = full_ids[len(q_ids):]                                    # option_answer_input_ids (:145-146)
            opt_ids.append(ids)
            seqs.append(Seq(ids, kv_slot=1 + j, past_len=P, prefix_slot=0))
            want += [(j, t) for t in range(len(ids) - 1)]
        o_logits, _ = eng.forward(seqs, want) if want else (np.zeros((0, cfg.llm_vocab), np.float16), None)
        losses, k = [], 0
        for ids in opt_ids:
            rows = [torch.from_numpy(q_logits[0:1])]
            if len(ids) > 1:
                rows.append(torch.from_numpy(o_logits[k:k + len(ids) - 1]))
            k += len(ids) - 1
            lg = torch.cat(rows, 0)                                        # cat(question_logits[-1:], option_logits[:-1])
            # CrossEntropyLoss on the fp16 logits (:156-159): fp32 log-softmax internally, fp16 result
            loss = torch.nn.functional.cross_entropy(lg.float(), torch.tensor(ids, dtype=torch.long)).to(torch.float16)
            losses.append(loss)
        return losses

    # ---- batched scoring with the on-device loss tail (csrc/score.hip) ----
    def score_continuations(self, image, question, continuations, object_crops=None, images_long=None,
                            objects_long=None) -> List[np.ndarray]:
        """Per-token negative log-likelihoods (float32 [n_tokens]) of each continuation as the assistant's answer to `question`
        — the tokens `option_losses` scores — computed on the device: no logits cross to the host."""
        return self.score_continuations_batch([dict(image=image, question=question, options=continuations,
                                                    object_crops=object_crops, images_long=images_long,
                                                    objects_long=objects_long)])[0]

    def score_continuations_batch(self, samples: Sequence[dict]) -> List[List[np.ndarray]]:
        """`score_continuations` for many samples (dicts with image, question, options and optionally object_crops, images_long,
        objects_long), two engine calls per chunk of samples: call 1 prefills every question of the chunk in one ragged batch
        and scores its last row once per option against that option's first token; call 2 advances every option as a fork of
        its question's KV slot and scores rows 0 .. len-2 against tokens 1 .. len-1.  Question i of a chunk and its options sit
        in consecutive KV slots.  A chunk is closed before the sample that would exceed max_images (1 + object crops per
        sample), max_slots (1 + options), max_rows (call 1: the questions' rows, padded to the longest when they are
        prefilled together; call 2: the options' rows) — values do not depend on how the samples fall into chunks beyond the
        GEMM kernels the row counts select."""
        cfg, eng = self.cfg, self.engine
        plans = []
        for s in samples:
            crops = s.get("object_crops")
            n_obj = len(crops) if crops is not None else 0
            if 1 + len(s["options"]) > cfg.max_slots:
                raise ValueError("more options than KV slots")
            if 1 + n_obj > cfg.max_images:
                raise ValueError(f"{1 + n_obj} images/object crops exceed the engine's feature table (max_images="
                                 f"{cfg.max_images}); build the engine with a larger VQAConfig.max_images")
            dummy = ([0], list(range(1, 1 + n_obj)), s.get("images_long"), s.get("objects_long"))
            q_ids, q_rows = self._question_rows(s["question"], *dummy)
            opt_ids = [self._question_rows(s["question"], *dummy, answer=o)[0][len(q_ids):] for o in s["options"]]   # (:145-146)
            # (the ids do not depend on the feature slots; the rows do, and are expanded again once the chunk's slots are known.
            # A one-token option is scored by call 1 alone but still rides through call 2 with no wanted row, as in option_losses:
            # call 2 of a batch of one then has exactly option_losses' rows, and with them the GEMM kernels its row count selects)
            plans.append(dict(s=s, n_img=1 + n_obj, n_slots=1 + len(opt_ids), P=len(q_rows), q_ids=q_ids, opt_ids=opt_ids,
                              n_opt_rows=sum(len(i) for i in opt_ids)))

        def call1_rows(ps):        # the engine right-pads fresh sequences of more than 64 rows in all to the longest
            tot = sum(p["P"] for p in ps)
            return len(ps) * max(p["P"] for p in ps) if tot > 64 else tot

        chunks, cur = [], []
        for p in plans:
            t = cur + [p]
            if cur and (sum(x["n_img"] for x in t) > cfg.max_images or sum(x["n_slots"] for x in t) > cfg.max_slots or
                        call1_rows(t) > cfg.max_rows or sum(x["n_opt_rows"] for x in t) > cfg.max_rows):
                chunks.append(cur)
                t = [p]
            cur = t
        if cur:
            chunks.append(cur)
        out: List[List[np.ndarray]] = []
        for ch in chunks:
            out += self._score_chunk(ch)
        return out

    def _score_chunk(self, plans) -> List[List[np.ndarray]]:
        eng = self.engine
        fslot = kslot = 0
        q_seqs, want1, tgt1, o_seqs, want2, tgt2 = [], [], [], [], [], []
        for i, p in enumerate(plans):
            s = p["s"]
            img_slots, obj_slots = self._encode(s["image"], s.get("object_crops"), fslot)
            fslot += p["n_img"]
            q_rows = eng.expand_ids(p["q_ids"], img_slots, obj_slots, s.get("images_long"), s.get("objects_long"))
            q_seqs.append(Seq(q_rows, kv_slot=kslot))
            for j, ids in enumerate(p["opt_ids"]):
                want1.append((i, -1))
                tgt1.append(ids[0])
                want2 += [(len(o_seqs), t) for t in range(len(ids) - 1)]
                tgt2 += ids[1:]
                o_seqs.append(Seq(ids, kv_slot=kslot + 1 + j, past_len=len(q_rows), prefix_slot=kslot))
            kslot += p["n_slots"]
        first = eng.forward_score(q_seqs, want1, tgt1) if want1 else np.zeros(0, np.float32)
        rest = eng.forward_score(o_seqs, want2, tgt2) if want2 else np.zeros(0, np.float32)
        out, a, b = [], 0, 0
        for p in plans:
            per = []
            for ids in p["opt_ids"]:
                per.append(np.concatenate([first[a:a + 1], rest[b:b + len(ids) - 1]]).astype(np.float32))
                a += 1
                b += len(ids) - 1
            out.append(per)
        return out

    @staticmethod
    def nll_loss(nll: np.ndarray) -> torch.Tensor:
        """The loss of one continuation from its per-token values, in token order: fp16(fp32(sum_double(nll) / n)) — what
        CrossEntropyLoss(mean) on the fp16 logits followed by .to(float16) gives, up to fp32 rounding."""
        acc = 0.0
        for v in np.asarray(nll, np.float32):
            acc += float(v)
        return torch.tensor(np.float16(np.float32(acc / len(nll))))

    def option_losses_batch(self, samples: Sequence[dict]) -> List[List[torch.Tensor]]:
        """`option_losses` of every sample (fp16 0-d tensors), through `score_continuations_batch`."""
        return [[self.nll_loss(v) for v in per] for per in self.score_continuations_batch(samples)]

    def multiple_choices_batch(self, samples: Sequence[dict]) -> List[int]:
        """`multiple_choices_inference` of every sample: the arg-min of its fp16 option losses, first index on ties."""
        return [int(torch.stack(losses).argmin().item()) for losses in self.option_losses_batch(samples)]
