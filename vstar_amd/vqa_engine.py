"""Python face of the VQA-LLM HIP engine (include/vstar_vqa.h): weight hand-over, image/object feature encoding into the
device-resident feature table, and the KV-cached forward over ragged rows of many sequences.  All arithmetic happens in
libvstar_hip.so (fp16 instantiation); numpy/torch only hold host buffers."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import IMAGE_TOKEN_INDEX, OBJECT_TOKEN_INDEX, PAD_ROW, VQAConfig
from .weights import vqa_state_dict_spec

_DT = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def _ptr(a: Optional[np.ndarray]):
    return ctypes.c_void_p(a.ctypes.data) if a is not None and a.size else None


class TokenLogprobs(NamedTuple):
    """The log-probability record of a call with `logprobs=n` (csrc/logprob.hip), one entry per wanted row: of the
    token the tail chose its log-probability and rank (0: it is the arg-max), and the n most likely tokens with theirs, sorted by
    (log-probability descending, token id ascending).  A verify row behind the acceptance holds NaN / -1."""
    token_logprob: np.ndarray    # float32 [n_want]
    rank: np.ndarray             # int32 [n_want]
    top_token: np.ndarray        # int32 [n_want, n]
    top_logprob: np.ndarray      # float32 [n_want, n]

    @staticmethod
    def concat(parts: Sequence["TokenLogprobs"], n: int) -> "TokenLogprobs":
        """The records of consecutive steps as one (an empty record of width n for no steps)."""
        if not parts:
            return TokenLogprobs(np.empty(0, np.float32), np.empty(0, np.int32), np.empty((0, n), np.int32), np.empty((0, n), np.float32))
        return TokenLogprobs(*(np.concatenate([p[k] for p in parts]) for k in range(4)))

    def rows(self, idx) -> "TokenLogprobs":
        return TokenLogprobs(*(a[idx] for a in self))


def check_logprobs(n) -> Optional[int]:
    """`logprobs=None | n`: None, or the number of alternatives as an int in [0, 32] (ValueError otherwise)."""
    if n is None:
        return None
    if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= _lib.MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs must be None or an integer in [0, {_lib.MAX_TOP_LOGPROBS}], got {n!r}")
    return int(n)


@dataclass
class Seq:
    """New rows of one sequence for `VqaEngine.forward`."""
    rows: Sequence[int]          # >= 0 vocabulary ids; < 0 feature rows as produced by VqaEngine.feature_rows()
    kv_slot: int                 # cache slot receiving the new rows' K/V
    past_len: int = 0            # cached positions in front of the new rows
    prefix_slot: Optional[int] = None   # slot holding [0, past_len); None = kv_slot


class VqaEngine:
    def __init__(self, cfg: VQAConfig, device: int = 0):
        self.cfg = cfg
        self.lib = _lib.load()
        self.handle = ctypes.c_void_p()
        c = cfg.to_c()
        _lib.check_vqa(self.lib.vstar_vqa_create(ctypes.byref(c), device, ctypes.byref(self.handle)))
        self.device = device
        self.finalized = False

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.vstar_vqa_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- weights (replaces load_pretrained_model, LLaVA/llava/model/builder.py:26-151) ----
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        for k in vqa_state_dict_spec(self.cfg):
            if k.startswith("clip.vision_model.encoder.layers.") and \
                    int(k.split(".")[4]) >= self.cfg.clip_layers + 1 + self.cfg.clip_select_layer:
                continue
            if k.startswith("clip.vision_model.post_layernorm"):
                continue
            if k not in sd:
                raise KeyError(f"checkpoint tensor missing: {k}")
            t = sd[k].detach().cpu().contiguous()
            if t.dtype not in _DT:
                t = t.float()
            shape = (ctypes.c_int64 * max(t.dim(), 1))(*t.shape)
            _lib.check_vqa(self.lib.vstar_vqa_load_tensor(self.handle, k.encode(), ctypes.c_void_p(t.data_ptr()), _DT[t.dtype],
                                                          t.dim(), shape), self.handle)
        _lib.check_vqa(self.lib.vstar_vqa_finalize_weights(self.handle), self.handle)
        self.finalized = True

    # ---- encode_images / project_features (llava_search_arch.py:84-94) ----
    def encode_images(self, pixels, first_slot: int = 0) -> None:
        """pixels [n,3,I,I] (CLIPImageProcessor output); fills feature slots first_slot .. first_slot+n-1."""
        t = torch.as_tensor(pixels).to(torch.float16).contiguous().cpu()
        I = self.cfg.clip_image_size
        assert t.dim() == 4 and tuple(t.shape[1:]) == (3, I, I), t.shape
        _lib.check_vqa(self.lib.vstar_vqa_encode_images(self.handle, t.shape[0], ctypes.c_void_p(t.data_ptr()), first_slot),
                       self.handle)

    def feature_rows(self, slot: int, long: bool) -> List[int]:
        """Row sources that splice the long (P rows) or short (pcv_latents rows) features of a slot."""
        P, L = self.cfg.n_img_tokens, self.cfg.pcv_latents
        base = slot * (P + L)
        idx = range(base, base + P) if long else range(base + P, base + P + L)
        return [-(1 + i) for i in idx]

    def expand_ids(self, ids: Sequence[int], image_slots: Sequence[int], object_slots: Sequence[int],
                   images_long: Optional[Sequence[bool]], objects_long: Optional[Sequence[bool]]) -> List[int]:
        """<image> (-200) / <object> (-300) placeholders -> feature rows, with the long/short selection of
        prepare_inputs_labels_for_multimodal (llava_search_arch.py:136-140,175-179)."""
        out: List[int] = []
        ii = io = 0
        for t in ids:
            if t == IMAGE_TOKEN_INDEX:
                out += self.feature_rows(image_slots[ii], images_long is None or bool(images_long[ii]))
                ii += 1
            elif t == OBJECT_TOKEN_INDEX:
                out += self.feature_rows(object_slots[io], not (objects_long is None or not objects_long[io]))
                io += 1
            else:
                out.append(int(t))
        return out

    # ---- LlavaSearchLlamaForCausalLM.forward over new rows (llava_search_llama.py:56-113) ----
    @staticmethod
    def _rows_args(seqs: Sequence[Seq], want: Sequence[Tuple[int, int]]):
        """The row arguments (nseq, row_off, src, kv_slot, prefix_slot, past_len, n_want, want) of the C-ABI forward calls, and the
        arrays behind them (keep them alive while the call runs)."""
        n = len(seqs)
        row_off = np.zeros(n + 1, np.int32)
        for i, s in enumerate(seqs):
            row_off[i + 1] = row_off[i] + len(s.rows)
        src = np.concatenate([np.asarray(s.rows, np.int64) for s in seqs]).astype(np.int32)
        kv = np.asarray([s.kv_slot for s in seqs], np.int32)
        pre = np.asarray([s.kv_slot if s.prefix_slot is None else s.prefix_slot for s in seqs], np.int32)
        past = np.asarray([s.past_len for s in seqs], np.int32)
        w = np.asarray([row_off[i] + (r if r >= 0 else len(seqs[i].rows) + r) for i, r in want], np.int32)
        return (n, _ptr(row_off), _ptr(src), _ptr(kv), _ptr(pre), _ptr(past), len(w), _ptr(w)), (row_off, src, kv, pre, past, w)

    @staticmethod
    def _per_row(values, dtype, nw: int, what: str) -> np.ndarray:
        """One value per wanted row as a contiguous array (a tail's scores / targets / drafts)."""
        a = np.ascontiguousarray(values, dtype)
        if a.shape != (nw,):
            raise ValueError(f"{a.size} {what} for {nw} wanted rows")
        return a

    @staticmethod
    def _sampling_array(params, nw: int):
        """One `_lib.VqaSampling` for all wanted rows, or a list of one per row -> the ctypes array behind the C pointer."""
        if isinstance(params, _lib.VqaSampling):
            params = [params] * nw
        if len(params) != nw:
            raise ValueError(f"{len(params)} sampling records for {nw} wanted rows")
        return (_lib.VqaSampling * max(nw, 1))(*params)

    @staticmethod
    def _warpers_array(warpers, nw: int):
        """One `_lib.VqaWarpers` for all wanted rows, or a list of one per row -> the ctypes array behind the C pointer."""
        if isinstance(warpers, _lib.VqaWarpers):
            warpers = [warpers] * nw
        if len(warpers) != nw:
            raise ValueError(f"{len(warpers)} warper records for {nw} wanted rows")
        return (_lib.VqaWarpers * max(nw, 1))(*warpers)

    @staticmethod
    def _edits_struct(edits, nw: int):
        """`edits` = the packed arrays (off, tok, penalty) of `LogitRules.pack`, one plan per wanted row -> the
        vstar_vqa_logit_edits record behind the C pointer, and the arrays to keep alive while the call runs."""
        off, tok, pen = edits
        off = np.ascontiguousarray(off, np.int32)
        tok = np.ascontiguousarray(tok, np.int32)
        pen = np.ascontiguousarray(pen, np.float32)
        if off.shape != (3 * nw + 1,) or pen.shape != (nw,):
            raise ValueError(f"logits edits for {(off.size - 1) // 3} rows ({pen.size} penalties) given for {nw} wanted rows")
        if off.size and tok.size < int(off.max(initial=0)):
            raise ValueError(f"logits edits: the offsets reach {int(off.max())} but only {tok.size} token ids are given")
        st = _lib.VqaLogitEdits(off.ctypes.data, tok.ctypes.data if tok.size else None, pen.ctypes.data)
        return st, (off, tok, pen)

    @staticmethod
    def _logprobs_struct(n: int, nw: int):
        """The vstar_vqa_logprobs record of a call that asks for n alternatives on nw wanted rows, and the host arrays behind it."""
        m = max(nw, 1)
        lp, rk = np.empty(m, np.float32), np.empty(m, np.int32)
        tt, tl = np.empty((m, n), np.int32), np.empty((m, n), np.float32)
        st = _lib.VqaLogprobs(n, lp.ctypes.data, rk.ctypes.data, tl.ctypes.data if n else None, tt.ctypes.data if n else None)
        return st, TokenLogprobs(lp[:nw], rk[:nw], tt[:nw], tl[:nw])

    @staticmethod
    def _guidance_struct(guidance, nw: int):
        """`guidance` = (neg, scale, log_beta), one entry per OUTPUT row (the first len(neg) wanted rows; the rest of the nw wanted
        rows are the negative rows neg points at, -1 = unguided) -> the vstar_vqa_guidance record behind the C pointer, the arrays to
        keep alive while the call runs, and n_out."""
        neg, scale, lb = guidance
        neg = np.ascontiguousarray(neg, np.int32)
        n_out = int(neg.size)
        scale = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float32), neg.shape))
        lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lb, np.float32), neg.shape))
        if neg.ndim != 1 or not 1 <= n_out <= nw:
            raise ValueError(f"guidance for {n_out} output rows given for {nw} wanted rows")
        return _lib.VqaGuidance(n_out, neg.ctypes.data, scale.ctypes.data, lb.ctypes.data), (neg, scale, lb), n_out

    def guide_rows(self, dev_logits: torch.Tensor, cond_row, neg_row, scale, log_beta, vocab: Optional[int] = None) -> None:
        """The guidance kernel alone (csrc/guide.hip) on a DEVICE tensor [rows, ld] of float16 / bfloat16: row
        cond_row[p] becomes the guided combination of itself and row neg_row[p], in place, for its first `vocab` (default ld)
        columns; scale[p] = gamma, log_beta[p] <= 0 (-inf: no plausibility cut).  Nothing else is written."""
        if dev_logits.dim() != 2 or not dev_logits.is_contiguous() or dev_logits.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("guide_rows needs a contiguous 2-d float16 / bfloat16 device tensor")
        rows, ld = dev_logits.shape
        c, u = np.ascontiguousarray(cond_row, np.int32), np.ascontiguousarray(neg_row, np.int32)
        sc, lb = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(log_beta, np.float32)
        if not (c.shape == u.shape == sc.shape == lb.shape and c.ndim == 1):
            raise ValueError("guide_rows: cond_row, neg_row, scale and log_beta must be 1-d arrays of one length")
        _lib.check_vqa(self.lib.vstar_vqa_guide_rows(ctypes.c_void_p(dev_logits.data_ptr()), _DT[dev_logits.dtype], rows,
                                                     ld if vocab is None else int(vocab), ld, int(c.size), _ptr(c), _ptr(u), _ptr(sc), _ptr(lb)))

    def logit_edit_capacity(self) -> int:
        """The most token ids (the three lists of all wanted rows together) one call with edits may carry."""
        return int(self.lib.vstar_vqa_logit_edit_capacity(self.handle))

    def forward(self, seqs: Sequence[Seq], want: Sequence[Tuple[int, int]], logits: bool = True, edits=None, logprobs=None, guidance=None):
        """want: (sequence index, row index inside that sequence's new rows; negative counts from the end).
        edits: None, or the packed arrays of `LogitRules.pack` (one plan per wanted row): the logits are edited on the device
        ahead of the arg-max (csrc/edit.hip) and the returned logits are the edited ones (HF's `scores`).
        logprobs: None, or n in [0, 32]: the arg-max's log-probability and rank and the n best alternatives of every wanted row,
        computed on the device from the (edited) row the arg-max was taken from (csrc/logprob.hip).
        guidance: None, or (neg, scale, log_beta) with one entry per OUTPUT row (csrc/guide.hip): the first
        len(neg) wanted rows are the output rows, the rest the negative rows; neg[j] = the index into `want` of output row j's
        negative row (-1: unguided), scale[j] = gamma, log_beta[j] = float32(log beta) <= 0 (-inf: no plausibility cut).  The
        output row's logits become gamma * (log_softmax(row) - log_softmax(negative)) + log_softmax(negative) ahead of the edits;
        edits, logprobs and everything returned then have one entry per OUTPUT row.  None takes the call without it.
        Returns (logits float16 [n_want, vocab] or None, argmax int32 [n_want]), with logprobs one more value, a `TokenLogprobs`."""
        n_lp = check_logprobs(logprobs)
        args, _keep = self._rows_args(seqs, want)
        nw = args[6]
        if guidance is not None:
            gd, _keep3, nw = self._guidance_struct(guidance, nw)
            out_logits = np.empty((nw, self.cfg.llm_vocab), np.float16) if logits else None
            out_arg = np.empty((nw,), np.int32)
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw) if n_lp is not None else (None, None)
            _lib.check_vqa(self.lib.vstar_vqa_forward_guided(self.handle, *args, _ptr(out_logits), _ptr(out_arg), ctypes.byref(gd),
                                                             ctypes.byref(st) if st is not None else None,
                                                             ctypes.byref(lp) if lp is not None else None), self.handle)
            return (out_logits, out_arg, rec) if n_lp is not None else (out_logits, out_arg)
        out_logits = np.empty((nw, self.cfg.llm_vocab), np.float16) if (logits and nw) else None
        out_arg = np.empty((max(nw, 1),), np.int32)
        if n_lp is not None:
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw)
            _lib.check_vqa(self.lib.vstar_vqa_forward_logprobs(self.handle, *args, _ptr(out_logits), _ptr(out_arg),
                                                               ctypes.byref(st) if st is not None else None, ctypes.byref(lp)), self.handle)
            return out_logits, out_arg[:nw], rec
        if edits is None:
            _lib.check_vqa(self.lib.vstar_vqa_forward(self.handle, *args, _ptr(out_logits), _ptr(out_arg)), self.handle)
        else:
            st, _keep2 = self._edits_struct(edits, nw)
            _lib.check_vqa(self.lib.vstar_vqa_forward_edits(self.handle, *args, _ptr(out_logits), _ptr(out_arg), ctypes.byref(st)),
                           self.handle)
        return out_logits, out_arg[:nw]

    def forward_sample(self, seqs: Sequence[Seq], want: Sequence[Tuple[int, int]], params, edits=None, logprobs=None, warpers=None,
                       guidance=None):
        """`forward` with the arg-max replaced by the on-device sampling tail (csrc/sample.hip): `params` holds one
        `_lib.VqaSampling` per wanted row (or one record for all of them); edits as in `forward` (the draw sees the edited
        logits).  logprobs as in `forward`, of the drawn token — under the edited, UN-WARPED, temperature-1 distribution (DESIGN.md
        §8.9).  warpers: None, or one `_lib.VqaWarpers` per wanted row (or one record for all): min-p, typical-p and the epsilon /
        eta cutoffs between top-p and the draw (`vqa.warper_params`); None is the call without them, launch for
        launch.  guidance as in `forward`: the draw is made from the guided (then edited) row, and params, warpers, edits, logprobs and
        the result have one entry per OUTPUT row.
        Returns the drawn tokens, int32 [n_want], with logprobs (tokens, `TokenLogprobs`); the logits never leave the device."""
        n_lp = check_logprobs(logprobs)
        args, _keep = self._rows_args(seqs, want)
        nw = args[6]
        if guidance is not None:
            gd, _keep3, nw = self._guidance_struct(guidance, nw)
            prm = self._sampling_array(params, nw)
            out = np.empty((nw,), np.int32)
            wrp = self._warpers_array(warpers, nw) if warpers is not None else None
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw) if n_lp is not None else (None, None)
            _lib.check_vqa(self.lib.vstar_vqa_forward_sample_guided(self.handle, *args, ctypes.cast(prm, ctypes.c_void_p), _ptr(out),
                                                                    ctypes.cast(wrp, ctypes.c_void_p) if wrp is not None else None,
                                                                    ctypes.byref(gd), ctypes.byref(st) if st is not None else None,
                                                                    ctypes.byref(lp) if lp is not None else None), self.handle)
            return (out, rec) if n_lp is not None else out
        prm = self._sampling_array(params, nw)
        out = np.empty((max(nw, 1),), np.int32)
        if warpers is not None:
            wrp = self._warpers_array(warpers, nw)
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw) if n_lp is not None else (None, None)
            _lib.check_vqa(self.lib.vstar_vqa_forward_sample_warp(self.handle, *args, ctypes.cast(prm, ctypes.c_void_p), _ptr(out),
                                                                  ctypes.cast(wrp, ctypes.c_void_p),
                                                                  ctypes.byref(st) if st is not None else None,
                                                                  ctypes.byref(lp) if lp is not None else None), self.handle)
            return (out[:nw], rec) if n_lp is not None else out[:nw]
        if n_lp is not None:
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw)
            _lib.check_vqa(self.lib.vstar_vqa_forward_sample_logprobs(self.handle, *args, ctypes.cast(prm, ctypes.c_void_p), _ptr(out),
                                                                      ctypes.byref(st) if st is not None else None, ctypes.byref(lp)),
                           self.handle)
            return out[:nw], rec
        if edits is None:
            _lib.check_vqa(self.lib.vstar_vqa_forward_sample(self.handle, *args, ctypes.cast(prm, ctypes.c_void_p), _ptr(out)),
                           self.handle)
        else:
            st, _keep2 = self._edits_struct(edits, nw)
            _lib.check_vqa(self.lib.vstar_vqa_forward_sample_edits(self.handle, *args, ctypes.cast(prm, ctypes.c_void_p), _ptr(out),
                                                                   ctypes.byref(st)), self.handle)
        return out[:nw]

    def forward_beam(self, seqs: Sequence[Seq], want: Sequence[Tuple[int, int]], beam_scores, group_off, n_cand: int,
                     logits: bool = False):
        """`forward` with the arg-max replaced by the on-device beam select (csrc/beam.hip): wanted row j carries
        the fp32 beam score beam_scores[j]; wanted rows group_off[g] .. group_off[g+1]-1 form group g.  Returns (scores float32
        [n_groups, n_cand], tokens int32 [n_groups, n_cand], rows-in-group int32 [n_groups, n_cand], logits float16 [n_want,
        vocab] or None), the candidates of each group sorted by (score descending, row * vocab + token ascending)."""
        args, _keep = self._rows_args(seqs, want)
        nw = args[6]
        sc = self._per_row(beam_scores, np.float32, nw, "beam scores")
        go = np.ascontiguousarray(group_off, np.int32)
        ng = max(len(go) - 1, 0)
        cs = np.empty((max(ng, 1), max(n_cand, 1)), np.float32)
        ct = np.empty_like(cs, dtype=np.int32)
        cr = np.empty_like(cs, dtype=np.int32)
        out_logits = np.empty((nw, self.cfg.llm_vocab), np.float16) if (logits and nw) else None
        _lib.check_vqa(self.lib.vstar_vqa_forward_beam(self.handle, *args, _ptr(sc), ng, _ptr(go), int(n_cand), _ptr(cs), _ptr(ct),
                                                       _ptr(cr), _ptr(out_logits)), self.handle)
        return cs[:ng, :n_cand], ct[:ng, :n_cand], cr[:ng, :n_cand], out_logits

    def forward_score(self, seqs: Sequence[Seq], want: Sequence[Tuple[int, int]], targets, rank: bool = False):
        """`forward` with the arg-max replaced by the on-device scoring tail (csrc/score.hip): wanted row j is
        scored against the token id targets[j].  Returns nll float32 [n_want] — the tokens' negative log-likelihoods — and, with
        rank=True, (nll, target_rank int32 [n_want]) where rank 0 means the arg-max is the target.  A row may be wanted several
        times with different targets; n_want may be as large as max_rows (the engine chunks by 256 rows); the logits never leave
        the device."""
        args, _keep = self._rows_args(seqs, want)
        nw = args[6]
        tg = self._per_row(targets, np.int32, nw, "targets")
        nll = np.empty((max(nw, 1),), np.float32)
        rk = np.empty((max(nw, 1),), np.int32) if rank else None
        _lib.check_vqa(self.lib.vstar_vqa_forward_score(self.handle, *args, _ptr(tg), _ptr(nll), _ptr(rk)), self.handle)
        return (nll[:nw], rk[:nw]) if rank else nll[:nw]

    def forward_verify(self, step: Sequence[Seq], wanted: Sequence[Tuple[int, int]], groups, draft, params=None, edits=None,
                       logprobs=None, warpers=None):
        """`forward` with the arg-max replaced by the on-device verify tail of speculative decoding (csrc/spec.hip, DESIGN.md
        §8.5): wanted rows groups[g] .. groups[g+1]-1 are the rows of one sequence in position order (its current token and the
        drafts fed behind it), draft[j] the token wanted row j's choice is compared with (-1 on a group's last row).  params:
        None = greedy, else one `_lib.VqaSampling` per wanted row (or one record for all).  edits as in `forward`: every row's
        choice sees its edited logits.  Returns (n_accept int32 [n_groups], tokens int32 [n_want]): per group the accepted drafts
        and one more token, -1 behind them.  logprobs as in `forward`, of every row's token (NaN / -1 on the -1 rows): one more
        returned value, a `TokenLogprobs`.  warpers as in `forward_sample` (sampled rows only: a greedy verify ignores them): a draft
        outside the kept set they leave is never accepted."""
        n_lp = check_logprobs(logprobs)
        args, _keep = self._rows_args(step, wanted)
        nw = args[6]
        go = np.ascontiguousarray(groups, np.int32)
        dr = self._per_row(draft, np.int32, nw, "draft entries")
        ng = max(len(go) - 1, 0)
        prm = self._sampling_array(params, nw) if params is not None else None
        acc = np.empty((max(ng, 1),), np.int32)
        tok = np.empty((max(nw, 1),), np.int32)
        tail = (ctypes.cast(prm, ctypes.c_void_p) if prm is not None else None, _ptr(go), ng, _ptr(dr), _ptr(acc), _ptr(tok))
        if warpers is not None:
            wrp = self._warpers_array(warpers, nw)
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw) if n_lp is not None else (None, None)
            _lib.check_vqa(self.lib.vstar_vqa_forward_verify_warp(self.handle, *args, *tail, ctypes.cast(wrp, ctypes.c_void_p),
                                                                  ctypes.byref(st) if st is not None else None,
                                                                  ctypes.byref(lp) if lp is not None else None), self.handle)
            return (acc[:ng], tok[:nw], rec) if n_lp is not None else (acc[:ng], tok[:nw])
        if n_lp is not None:
            st, _keep2 = self._edits_struct(edits, nw) if edits is not None else (None, None)
            lp, rec = self._logprobs_struct(n_lp, nw)
            _lib.check_vqa(self.lib.vstar_vqa_forward_verify_logprobs(self.handle, *args, *tail, ctypes.byref(st) if st is not None else None,
                                                                      ctypes.byref(lp)), self.handle)
            return acc[:ng], tok[:nw], rec
        if edits is None:
            _lib.check_vqa(self.lib.vstar_vqa_forward_verify(self.handle, *args, *tail), self.handle)
        else:
            st, _keep2 = self._edits_struct(edits, nw)
            _lib.check_vqa(self.lib.vstar_vqa_forward_verify_edits(self.handle, *args, *tail, ctypes.byref(st)), self.handle)
        return acc[:ng], tok[:nw]

    def forward_contrast_begin(self, seqs: Sequence[Seq], want: Sequence[Tuple[int, int]], k: int):
        """The prefill of contrastive search (csrc/contrast.hip): `forward` that also writes the final-norm hidden
        row of every new row into its slot's history (prefix_slot == kv_slot; past_len 0, or the slot's history length for a chunked
        prefill).  Returns (next_tok int32 [n_want, k], next_prob float32 [n_want, k]): per wanted row the k most probable tokens,
        sorted by (probability descending, token id ascending)."""
        args, _keep = self._rows_args(seqs, want)
        nw, k = args[6], int(k)
        nt = np.empty((max(nw, 1), max(k, 1)), np.int32)
        npb = np.empty((max(nw, 1), max(k, 1)), np.float32)
        _lib.check_vqa(self.lib.vstar_vqa_forward_contrast_begin(self.handle, *args, k, _ptr(nt), _ptr(npb)), self.handle)
        return nt[:nw, :k], npb[:nw, :k]

    def forward_contrast_step(self, seqs: Sequence[Seq], group_off, cand_prob, alpha: float, k_next: int, penalties: bool = False):
        """One step of contrastive search: every Seq is ONE candidate row (all rows are wanted), rows group_off[g] ..
        group_off[g+1]-1 the candidates of group g — continuations of one owner slot (their prefix_slot) at past_len == the owner's
        history length, each into a kv_slot of its own.  cand_prob[j]: candidate j's probability.  On the device: the degeneration
        penalty against the owner's hidden history, score = (1 - alpha) p - alpha pen, the pick, the winner's hidden row appended,
        its K/V row adopted by the owner slot.  Returns (sel int32 [n_groups] — the winner's row in its group, next_tok int32
        [n_groups, k_next], next_prob float32 [n_groups, k_next]), with penalties=True one more value, pen float32 [n_rows]."""
        args, _keep = self._rows_args(seqs, [(i, 0) for i in range(len(seqs))])
        nw, k = args[6], int(k_next)
        go = np.ascontiguousarray(group_off, np.int32)
        ng = max(len(go) - 1, 0)
        cp = self._per_row(cand_prob, np.float32, nw, "candidate probabilities")
        sel = np.empty((max(ng, 1),), np.int32)
        nt = np.empty((max(ng, 1), max(k, 1)), np.int32)
        npb = np.empty((max(ng, 1), max(k, 1)), np.float32)
        pen = np.empty((max(nw, 1),), np.float32) if penalties else None
        _lib.check_vqa(self.lib.vstar_vqa_forward_contrast_step(self.handle, *args, _ptr(go), ng, _ptr(cp), float(alpha), k, _ptr(sel),
                                                                _ptr(nt), _ptr(npb), _ptr(pen)), self.handle)
        out = (sel[:ng], nt[:ng, :k], npb[:ng, :k])
        return out + (pen[:nw],) if penalties else out

    def contrast_hist(self, slot: int) -> np.ndarray:
        """The hidden history of a slot, float32 [hist_len, hidden] (parity tests)."""
        H = self.cfg.llm_hidden
        return self.debug_read(f"contrast_hist:{int(slot)}", self.cfg.max_ctx * H).reshape(-1, H)

    def contrast_cand(self) -> np.ndarray:
        """The candidate hidden rows of the last contrast step, float32 [rows, hidden] (parity tests)."""
        H = self.cfg.llm_hidden
        return self.debug_read("contrast_cand", 256 * H).reshape(-1, H)

    def kv_reorder(self, dst_slots: Sequence[int], src_slots: Sequence[int], lo: int, hi: int) -> None:
        """Beam reorder without moving K/V: ancestry entries [lo, hi) of dst_slots[i] = those of src_slots[i], all sources read
        before any destination is written (include/vstar_vqa.h)."""
        d = np.ascontiguousarray(dst_slots, np.int32)
        s = np.ascontiguousarray(src_slots, np.int32)
        if d.shape != s.shape:
            raise ValueError("kv_reorder: dst_slots and src_slots differ in length")
        _lib.check_vqa(self.lib.vstar_vqa_kv_reorder(self.handle, int(d.size), _ptr(d), _ptr(s), int(lo), int(hi)), self.handle)

    def kv_copy(self, dst: int, src: int, lo: int, hi: int) -> None:
        """Physical copy of K/V rows [lo, hi) into dst's own rows, read through src's ancestry; dst's ancestry -> identity."""
        _lib.check_vqa(self.lib.vstar_vqa_kv_copy(self.handle, int(dst), int(src), int(lo), int(hi)), self.handle)

    def decode_weight_bits(self) -> int:
        """8 when the int8 weight-only decode mode is active (finalized engine built with decode_weight_bits=8), 4 in the int4
        group-scaled mode (decode_weight_format=1), else 0."""
        return int(self.lib.vstar_vqa_decode_weight_bits(self.handle))

    def kv_cache_format(self) -> int:
        """The active KV-cache format: 0 = fp16, 1 = block-scaled fp8 (config.KVFMT_MXFP8), 2 = the same values emulated in fp16."""
        return int(self.lib.vstar_vqa_kv_cache_format(self.handle))

    def kv_cache_bytes(self) -> int:
        """Bytes of K plus V storage of the finalized engine, scale bytes included: what max_slots and max_ctx cost."""
        return int(self.lib.vstar_vqa_kv_cache_bytes(self.handle))

    def kv_rows(self, layer: int, slot: int) -> np.ndarray:
        """The DECODED K and V cache of one layer and slot, float32 [2, heads, max_ctx, 128], in every format (parity tests)."""
        H, C = self.cfg.llm_heads, self.cfg.max_ctx
        return self.debug_read(f"kv:{int(layer)}:{int(slot)}", 2 * H * C * 128).reshape(2, H, C, 128)

    def last_forward_ms(self) -> float:
        return float(self.lib.vstar_vqa_last_forward_ms(self.handle))

    def debug_read(self, name: str, count: int) -> np.ndarray:
        out = np.empty((count,), np.float32)
        n = self.lib.vstar_vqa_debug_read(self.handle, name.encode(), ctypes.c_void_p(out.ctypes.data), count)
        if n < 0:
            _lib.check_vqa(int(n), self.handle)
        return out[:n]

    def features(self, slot: int) -> Tuple[np.ndarray, np.ndarray]:
        """(long [P,H], short [L,H]) of one feature slot, as float32 (parity tests)."""
        P, L, H = self.cfg.n_img_tokens, self.cfg.pcv_latents, self.cfg.llm_hidden
        all_ = self.debug_read("features", (slot + 1) * (P + L) * H).reshape(slot + 1, P + L, H)
        return all_[slot, :P], all_[slot, P:]
