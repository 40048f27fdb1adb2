/*
 * vstar_vqa.h — C-ABI of the VQA-LLM engine inside libvstar_hip.so (MI355X / gfx950, IEEE fp16 storage, fp32 accumulate):
 * the second model of the V* pipeline, i.e. `LlavaSearchLlamaForCausalLM`
 *   CLIP-ViT-L/14@224 -> { mm_projector ("long", 256 tokens/image) | mm_projector_object = LayerNorm + PerceiverResampler
 *   + Linear ("short", 32 tokens/image) } -> <image>/<object> splice -> LLaMA-7B with a KV cache -> lm_head,
 * as driven by VQA_LLM.free_form_inference / multiple_choices_inference (vstar_bench_eval.py:78-165).
 *
 * The reference has no FFI; the Python call sites each entry point replaces are cited below (paths relative to the
 * reference repo root).  Conventions are those of vstar_hip.h (0 = OK, negative = error, caller owns host buffers, one
 * handle per device, stream-ordered, synchronised before return).  fp16 tensors cross the ABI as uint16_t bits.
 *
 * Design (MI355X-first, not a port of HF generate): the KV cache is a set of `max_slots` fixed slots of `max_ctx`
 * positions ([layer][slot][head][ctx][128], K and V) resident in HBM; a forward call advances any number of sequences by
 * any number of new rows each (prefill, one-token decode steps of many sequences at once, or teacher-forced option
 * continuations), and a sequence may read its first `past_len` positions from ANOTHER slot — the multiple-choice options
 * fork the question's cache without copying it.  Rows are vocabulary ids or rows of the device-resident feature table
 * written by vstar_vqa_encode_images, so image/object features never leave the GPU.
 */
#ifndef VSTAR_VQA_H
#define VSTAR_VQA_H

#include "vstar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSTAR_VQA_ABI_VERSION 1
#define VSTAR_VQA_PAD_ROW INT32_MIN      /* a row source meaning "zero embedding" */

/* Geometry: LlavaSearchConfig(LlamaConfig) + CLIP tower + projector builder
 * (LLaVA/llava/model/language_model/llava_search_llama.py:30-50, multimodal_projector/builder.py:33-68). */
typedef struct vstar_vqa_config {
  int32_t abi_version;        /* VSTAR_VQA_ABI_VERSION */
  int32_t clip_image_size;    /* 224 */
  int32_t clip_patch;         /* 14 */
  int32_t clip_hidden;        /* 1024 */
  int32_t clip_heads;         /* 16 */
  int32_t clip_mlp;           /* 4096 */
  int32_t clip_layers;        /* 24 */
  int32_t clip_select_layer;  /* -2, patch tokens only (mm_vision_select_feature = 'patch') */
  int32_t llm_hidden;         /* 4096 */
  int32_t llm_heads;          /* 32 (head dim 128) */
  int32_t llm_mlp;            /* 11008 */
  int32_t llm_layers;         /* 32 */
  int32_t llm_vocab;          /* len(tokenizer) after builder.py:131-135 */
  float   llm_rms_eps;
  float   llm_rope_theta;
  int32_t projector_type;     /* mm_projector: 0 = linear, 1 = mlp2x_gelu (builder.py:39-49) */
  int32_t pcv_depth;          /* 6   PerceiverResampler(depth, heads, dim_head, num_latents), builder.py:54-66 */
  int32_t pcv_heads;          /* 16 */
  int32_t pcv_dim_head;       /* 96 */
  int32_t pcv_latents;        /* 32 = short tokens per image */
  int32_t pcv_ff_mult;        /* 4 */
  int32_t max_slots;          /* KV-cache slots */
  int32_t max_ctx;            /* positions per slot */
  int32_t max_rows;           /* new rows per forward call (after padding a ragged prefill batch) */
  int32_t max_images;         /* feature-table slots; each holds P long rows then pcv_latents short rows */
  int32_t decode_weight_bits; /* 0 (default) = fp16 weights everywhere; 8 = int8 weight-only decode of the LLaMA block linears
                               * (q|k|v, o_proj, gate|up, down_proj), see vstar_vqa_decode_weight_bits; anything else fails at create */
  int32_t decode_weight_format; /* 0 (default) = decode_weight_bits alone decides; VSTAR_VQA_WFMT_W4G128 (1) = int4 group-scaled
                               * weight-only decode (one fp16 scale per 128 input channels): needs decode_weight_bits
                               * == 0, llm_hidden % 128 == 0 and llm_mlp % 128 == 0; anything else fails at create */
  int32_t kv_cache_format;    /* 0 (default) = fp16 KV cache; VSTAR_VQA_KVFMT_MXFP8 (1) = block-scaled fp8 (MX e4m3, blocks of 32: 132
                               * bytes per cached row instead of 256); VSTAR_VQA_KVFMT_MXFP8_EMULATED (2) = the same values held in the
                               * fp16 cache (yardstick / study tool), see vstar_vqa_kv_cache_format; anything else fails at create.
                               * Independent of decode_weight_bits / decode_weight_format */
  int32_t reserved[5];
} vstar_vqa_config;

#define VSTAR_VQA_WFMT_W4G128 1 /* vstar_vqa_config.decode_weight_format */
#define VSTAR_VQA_KVFMT_MXFP8 1          /* vstar_vqa_config.kv_cache_format */
#define VSTAR_VQA_KVFMT_MXFP8_EMULATED 2

typedef struct vstar_vqa_engine vstar_vqa_handle;

/* Replaces load_pretrained_model(...) (LLaVA/llava/model/builder.py:26-151, called at vstar_bench_eval.py:46). */
int vstar_vqa_create(const vstar_vqa_config* cfg, int device, vstar_vqa_handle** out);
void vstar_vqa_destroy(vstar_vqa_handle* h);
const char* vstar_vqa_last_error(const vstar_vqa_handle* h);
/* HF state-dict keys of LlavaSearchLlamaForCausalLM ("model.layers.N...", "model.mm_projector...",
 * "model.mm_projector_object.{0,1,2}...", "lm_head.weight") plus the separately loaded CLIP tower under "clip.". */
int vstar_vqa_load_tensor(vstar_vqa_handle* h, const char* key, const void* host_ptr, int dtype, int ndim,
                          const int64_t* shape);
int vstar_vqa_finalize_weights(vstar_vqa_handle* h);

/* encode_images / project_features (LLaVA/llava/model/llava_search_arch.py:84-94): CLIP tower, then BOTH projectors, for
 * n images given as fp16 pixels [n,3,I,I] (CLIPImageProcessor output, .half()).  Image i fills feature slot
 * first_slot + i: rows [0,P) = long features, rows [P, P+pcv_latents) = short features; a feature row's global index is
 * slot * (P + pcv_latents) + row, and a forward row source of -(1 + index) splices it
 * (prepare_inputs_labels_for_multimodal, llava_search_arch.py:96-266). */
int vstar_vqa_encode_images(vstar_vqa_handle* h, int n, const uint16_t* pixels_f16, int first_slot);

/* One model forward over new rows of nseq sequences — LlavaSearchLlamaForCausalLM.forward
 * (llava_search_llama.py:56-113) for the prefill (vstar_bench_eval.py:127-133), each generate() step (:90-103) and each
 * option continuation with past_key_values (:148-151).
 *   row_off[nseq+1]  sequence i contributes rows row_off[i] .. row_off[i+1]-1 of src
 *   src[rows]        >= 0: vocabulary id; < 0: feature row -(1+index); VSTAR_VQA_PAD_ROW: zero row
 *   kv_slot[nseq]    slot that receives the new rows' K/V at positions past_len[i], past_len[i]+1, ...
 *   prefix_slot[nseq] slot holding positions [0, past_len[i]) (== kv_slot[i] unless the sequence forks a shared prefix)
 *   past_len[nseq]   number of cached positions in front of the new rows
 *   want[n_want]     indices into src of the rows whose logits are needed (lm_head runs on these rows only)
 *   logits_f16       [n_want, llm_vocab] fp16 logits (may be NULL);  argmax [n_want] (may be NULL) */
int vstar_vqa_forward(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                      const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                      uint16_t* logits_f16, int32_t* argmax);

/* Sampled decoding: HF 4.31 generate(do_sample=True) for one logits row.  Scores s = lp(float(x) / temperature)
 * rounded to the logits' storage type; top-k keeps every score >= the k-th largest (ties included); top-p keeps a token iff
 * the softmax mass of the kept tokens with a strictly greater score is < top_p (the maximal score is always kept); the token
 * is the smallest kept index, in vocabulary order, whose inclusive prefix mass exceeds u * Z (Z = the kept mass), with
 * u = (x0 >> 8) * 2^-24 and x0 the first word of Philox4x32-10 at key (seed lo, seed hi), counter (step, stream lo,
 * stream hi, 0).  Masses are exp(s - max s) in unsigned 64-bit fixed point (2^-40 units), summed exactly: the draw is
 * deterministic and a row's token depends on that row and its record only. */
typedef struct vstar_vqa_sampling {   /* 32 bytes */
  float    temperature;   /* > 0 */
  int32_t  top_k;         /* 0 = off */
  float    top_p;         /* [0,1]; >= 1 = off */
  uint32_t step;          /* Philox counter word 0 */
  uint64_t seed;          /* Philox key */
  uint64_t stream;        /* Philox counter words 1-2 */
} vstar_vqa_sampling;

/* vstar_vqa_forward with the arg-max replaced by the sampling tail: params[n_want], tokens[n_want] (host).  Only the tokens
 * cross to the host (no logits copy). */
int vstar_vqa_forward_sample(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src,
                             const int32_t* kv_slot, const int32_t* prefix_slot, const int32_t* past_len,
                             int n_want, const int32_t* want, const vstar_vqa_sampling* params, int32_t* tokens);

/* Op-level (tests, micro-benchmarks): DEVICE logits [rows, ld] of dtype F16/BF16 (1 <= vocab <= 2^22, rows <= 65535); host
 * params / outputs; u_out[rows] and n_kept[rows] nullable diagnostics (the uniform drawn, the size of the kept set).  Null
 * stream, synchronises. */
int vstar_vqa_op_sample(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld,
                        const vstar_vqa_sampling* params, int32_t* tokens, float* u_out, int32_t* n_kept);

/* Beam search: HF 4.31 generate(num_beams=k).  vstar_vqa_forward with the arg-max replaced by the beam-select
 * tail: wanted row j carries the fp32 beam score beam_scores[j]; rows group_off[g] .. group_off[g+1]-1 of `want` form group g
 * (the k beams of one sample, 1 .. 16 rows).  Per row lp = log_softmax(logits) (log-sum-exp in double, rounded to fp16) and
 * s = beam score + lp (one fp32 add); per group the n_cand (<= 32, <= rows x vocab) largest s, sorted by (s descending,
 * row_in_group * vocab + token ascending), come back as cand_scores / cand_tokens / cand_rows [n_groups, n_cand] (host).
 * logits_f16 (nullable): the raw logits rows as in vstar_vqa_forward. */
int vstar_vqa_forward_beam(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                           const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                           const float* beam_scores, int n_groups, const int32_t* group_off, int n_cand, float* cand_scores,
                           int32_t* cand_tokens, int32_t* cand_rows, uint16_t* logits_f16);
/* Beam reorder without moving K/V: every slot has an ancestry row (position p of its sequence lives in slot anc[slot][p]);
 * entries [lo, hi) of dst_slot[i] become those of src_slot[i] for i < n, as if every source were read before any destination is
 * written (swaps, one source feeding several destinations).  The destinations become "ancestral": their continued sequences
 * (prefix_slot == kv_slot) attend through the table; a fresh sequence (past_len 0) in the slot, or a fork INTO it (prefix_slot
 * another slot, whose [0, past_len) it then reads) makes it an ordinary slot again; forking FROM an ancestral slot is an error
 * (kv_copy it into a slot of its own first).  The rows a
 * forward call writes always land in the sequence's own slot, so a physical row is written once and never overwritten while a
 * descendant can read it — as long as every beam of a search advances by the same positions. */
int vstar_vqa_kv_reorder(vstar_vqa_handle* h, int n, const int32_t* dst_slot, const int32_t* src_slot, int lo, int hi);
/* Physical copy of the K/V rows [lo, hi) of every layer into dst's own rows, read through src's ancestry (dst != src); dst's
 * ancestry becomes the identity.  Detaches a beam; the yardstick of the reorder's bit-identity tests. */
int vstar_vqa_kv_copy(vstar_vqa_handle* h, int dst, int src, int lo, int hi);
/* Op-level beam select (tests, micro-benchmarks): DEVICE logits [rows, ld] of dtype F16/BF16 (1 <= vocab <= 2^22); host
 * beam_scores[rows], group_off[n_groups+1], outputs [n_groups, n_cand]; lp_out (nullable, host, [rows, vocab]) the rounded
 * log-probabilities as float.  Null stream, synchronises. */
int vstar_vqa_op_beam_select(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const float* beam_scores,
                             int n_groups, const int32_t* group_off, int n_cand, float* cand_scores, int32_t* cand_tokens,
                             int32_t* cand_rows, float* lp_out);

/* Scoring: vstar_vqa_forward with the arg-max replaced by the scoring tail: targets[n_want] (host), nll[n_want]
 * fp32 (host), target_rank[n_want] nullable.  Per wanted row j: lse = max + log(sum exp(x_i - max)) in double (fixed summation
 * order), nll[j] = (float)(lse - x[targets[j]]) — the token's negative log-likelihood, one rounding; x[target] = -inf gives
 * +inf, NaN logits give NaN; target_rank[j] = #{i : x_i > x[targets[j]]} (0: the arg-max is the target).  A target outside
 * [0, llm_vocab) is an error.  A row may appear in `want` several times with different targets.  n_want <= max_rows: the
 * wanted rows are processed in consecutive chunks of 256 (the last one shorter), each through norm -> lm_head -> score, so rows
 * [256 c, 256 (c + 1)) see the lm_head of a vstar_vqa_forward call that wants exactly those rows.  No logits cross to the host. */
int vstar_vqa_forward_score(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                            const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                            const int32_t* targets, float* nll, int32_t* target_rank);
/* Op-level (tests, micro-benchmarks): DEVICE logits [rows, ld], F16/BF16 (1 <= vocab <= 2^22, rows <= 65535), host targets /
 * outputs; target_rank and lse_out (double [rows], the log-sum-exp) nullable.  Null stream, synchronises. */
int vstar_vqa_op_score(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* targets, float* nll,
                       int32_t* target_rank, double* lse_out);

/* Speculative decoding: vstar_vqa_forward with the arg-max replaced by the verify tail.  A sequence is fed its
 * current token plus d draft tokens as one multi-row continuation, all d + 1 rows wanted; rows group_off[g] .. group_off[g+1]-1 of
 * `want` form group g — rows of ONE sequence in position order, 1 .. 16 of them — and draft[j] is the token wanted row j's choice
 * is compared with, i.e. the token fed as the next row (-1 = not compared: always so on a group's last row).  Per group, with rows
 * r0 .. r0+m:  n_accept_out[g] = a, the number of leading rows whose choice accepted its draft;  tokens_out[r0 .. r0+a] = the
 * chosen tokens (the a accepted drafts and one more token), tokens_out behind them = -1.  The sequence's cache is then valid up to
 * past_len + a + 1 positions; the rows behind are overwritten by its next call.
 *   params == NULL (greedy): a row's choice is vstar_vqa_forward's arg-max of that row, bit for bit; it accepts iff it equals
 *     the draft.
 *   params[n_want] (sampled): the kept set and fixed-point masses m_i, Z = sum m_i, of vstar_vqa_forward_sample.  A row without
 *     draft is that call's draw.  With draft x: accept iff x is kept and floor(u_a * Z) < m_x, u_a the uniform of Philox counter
 *     (step, stream + 1); otherwise the token is drawn from the kept set without x (Z' = Z - m_x, or Z): the smallest kept index
 *     != x whose inclusive prefix mass, skipping x, exceeds floor(u * Z'), u the uniform of (step, stream), and the group ends.
 *     Either way P(token = y) = m_y / Z.
 * Errors (VSTAR_ERR_INVALID, before any launch): a draft outside [0, llm_vocab) other than -1, a last row with a draft, a group of
 * more than 16 rows, groups that do not cover the wanted rows, wanted rows of a group that are not rows of one sequence in
 * position order.  Only n_accept_out and tokens_out cross to the host. */
int vstar_vqa_forward_verify(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                             const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                             const vstar_vqa_sampling* params, const int32_t* group_off, int n_groups, const int32_t* draft,
                             int32_t* n_accept_out, int32_t* tokens_out);
/* Op-level (tests, micro-benchmarks): DEVICE logits [rows, ld], F16/BF16 (1 <= vocab <= 2^22, rows <= 65535); host group_off /
 * draft / params (nullable: greedy) / outputs.  Null stream, synchronises. */
int vstar_vqa_op_verify(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                        const int32_t* draft, const vstar_vqa_sampling* params, int32_t* n_accept_out, int32_t* tokens_out);

/* Logits edits: HF generate's logits processors — repetition_penalty, no_repeat_ngram_size, bad_words_ids,
 * min_new_tokens, suppress_tokens, prefix_allowed_tokens_fn — reduced by the caller to three token lists per wanted row and applied
 * on the device to that row's logits x (storage type T) between lm_head and the tail that picks a token:
 *   1. penalised t:  x[t] = T(f32(x[t]) < 0 ? f32(x[t]) * theta : f32(x[t]) / theta), IEEE fp32 multiply / divide, then one
 *      round-to-nearest-even to T (NaN stays NaN, -0 takes the divide): transformers' RepetitionPenaltyLogitsProcessor, bit for bit
 *   2. banned t:     x[t] = -inf
 *   3. a non-empty allowed list:  x[t] = -inf for every t in [0, llm_vocab) not in it
 * in this order: a ban wins over a penalty, a token both allowed and banned is -inf.  All arrays HOST, one CSR array for the lists:
 *   off[3 * n_want + 1]  non-decreasing, off[0] == 0; wanted row j's penalised ids are tok[off[3j] .. off[3j+1]), its banned ids
 *                        tok[off[3j+1] .. off[3j+2]), its allowed ids tok[off[3j+2] .. off[3j+3])
 *   tok[off[3 n_want]]   every list strictly increasing, ids in [0, llm_vocab)
 *   penalty[n_want]      theta per row, finite and > 0; read only where the row's penalised list is non-empty
 * A row whose three lists are empty keeps its logits untouched. */
typedef struct vstar_vqa_logit_edits {
  const int32_t* off;
  const int32_t* tok;
  const float*   penalty;
} vstar_vqa_logit_edits;

/* vstar_vqa_forward / _forward_sample / _forward_verify with the edits applied to the wanted rows' logits ahead of the arg-max /
 * draw / verify choice; edits == NULL is the plain call, bit for bit.  logits_f16 of the first returns the EDITED logits (HF's
 * `scores`).  Errors (VSTAR_ERR_INVALID, before any device work, the engine stays usable): lists that break the rules above, or more
 * than vstar_vqa_logit_edit_capacity ids in one call.  The device arrays for the lists are allocated by the first call that
 * carries edits (a failed allocation is VSTAR_ERR_NOMEM and leaves the engine usable); an engine that never sees edits allocates and
 * launches nothing for them.  The beam and scoring tails take no edits: HF applies the processors to the log-softmax output in beam
 * search, with the log-sum-exp of the unedited row, which an edit ahead of the beam select would not reproduce (open follow-up);
 * a target's likelihood under edited logits has no reference meaning. */
int vstar_vqa_forward_edits(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                            const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                            uint16_t* logits_f16, int32_t* argmax, const vstar_vqa_logit_edits* edits);
int vstar_vqa_forward_sample_edits(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src,
                                   const int32_t* kv_slot, const int32_t* prefix_slot, const int32_t* past_len,
                                   int n_want, const int32_t* want, const vstar_vqa_sampling* params, int32_t* tokens,
                                   const vstar_vqa_logit_edits* edits);
int vstar_vqa_forward_verify_edits(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                                   const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                                   const vstar_vqa_sampling* params, const int32_t* group_off, int n_groups, const int32_t* draft,
                                   int32_t* n_accept_out, int32_t* tokens_out, const vstar_vqa_logit_edits* edits);
/* The most token ids (the three lists of all wanted rows together) one call with edits may carry: 256 * (max_ctx + 2048). */
int64_t vstar_vqa_logit_edit_capacity(const vstar_vqa_handle* h);
/* Op-level (tests, micro-benchmarks): DEVICE logits [rows, ld] of dtype F16/BF16 (1 <= vocab <= 2^22, rows <= 65535, any ld >=
 * vocab), edited in place — columns [vocab, ld) are never written; host off / tok / penalty as above with n_want = rows, checked
 * before any device work.  Null stream, synchronises. */
int vstar_vqa_op_edit(void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok,
                      const float* penalty);

/* Per-token log-probabilities and top-n alternatives: HF generate's output_scores / compute_transition_scores
 * without a vocabulary row crossing to the host.  Behind the arg-max, the draw or the verify choice, on the logits row x that tail
 * just read and the token t it just chose, per wanted row j:
 *   lse              = max + log(sum exp(x_i - max)) in double, fixed summation order: vstar_vqa_forward_score's, bit for bit
 *   token_logprob[j] = (float)(x[t] - lse), one rounding: the sign-flipped nll of vstar_vqa_forward_score for target t.  x[t] = -inf
 *                      gives -inf, NaN logits give NaN, a row whose maximum is +inf gives NaN
 *   token_rank[j]    = #{i : x_i > x[t]} (nullable; 0: t is the arg-max)
 *   top_token / top_logprob [j, 0 .. n), n = min(n_top, llm_vocab): the n largest elements under (value descending, index
 *                      ascending), in that order, compared by VALUE (-0 and +0 tie, the lower index first; a NaN sorts as -inf),
 *                      top_logprob = (float)(x[i] - lse); entries [n, n_top) are -1 / NaN
 *   a verify row behind the acceptance (tokens_out[j] = -1) is not read: token_logprob NaN, token_rank -1, top_token -1, top_logprob NaN
 * With edits the row is the EDITED row: the log-probabilities are of the distribution the pick was made from.  Under sampling the
 * row is the edited, UN-WARPED, temperature-1 row (HF's `scores` under sampling are the warped ones: a stated deviation). */
#define VSTAR_VQA_MAX_TOP_LOGPROBS 32
typedef struct vstar_vqa_logprobs {   /* all HOST arrays */
  int32_t  n_top;          /* 0 .. 32 */
  float*   token_logprob;  /* [n_want] */
  int32_t* token_rank;     /* [n_want], nullable */
  float*   top_logprob;    /* [n_want, n_top], null iff n_top == 0 */
  int32_t* top_token;      /* [n_want, n_top], null iff n_top == 0 */
} vstar_vqa_logprobs;

/* vstar_vqa_forward_edits / _forward_sample_edits / _forward_verify_edits with the log-probability outputs; edits stays nullable,
 * lp == NULL is the _edits call bit for bit.  Errors (VSTAR_ERR_INVALID, before any device work, the engine stays usable): n_top
 * outside [0, 32], a missing token_logprob, top arrays that do not match n_top.  The device arrays for the outputs are allocated by
 * the first call that asks (a failed allocation is VSTAR_ERR_NOMEM and leaves the engine usable); an engine that never asks allocates,
 * launches and copies nothing for them.  The beam and scoring tails have no such entry: beam candidates carry their scores, the
 * scoring tail returns the target's nll and rank. */
int vstar_vqa_forward_logprobs(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                               const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                               uint16_t* logits_f16, int32_t* argmax, const vstar_vqa_logit_edits* edits,
                               const vstar_vqa_logprobs* lp);
int vstar_vqa_forward_sample_logprobs(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src,
                                      const int32_t* kv_slot, const int32_t* prefix_slot, const int32_t* past_len,
                                      int n_want, const int32_t* want, const vstar_vqa_sampling* params, int32_t* tokens,
                                      const vstar_vqa_logit_edits* edits, const vstar_vqa_logprobs* lp);
int vstar_vqa_forward_verify_logprobs(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                                      const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                                      const vstar_vqa_sampling* params, const int32_t* group_off, int n_groups, const int32_t* draft,
                                      int32_t* n_accept_out, int32_t* tokens_out, const vstar_vqa_logit_edits* edits,
                                      const vstar_vqa_logprobs* lp);
/* Further warpers of the sampled decode: the rest of HF 4.31 generate's warper list, on the device, behind
 * top-k / top-p and ahead of the draw, in HF's order min-p -> typical-p -> epsilon -> eta.  Each stage sees the kept set K the
 * stage before it left and p_i = m_i / Z_K, with m_i the fixed-point masses of vstar_vqa_sampling (exp(s_i - s_max) in 2^-40 units,
 * relative to the row's maximum whether or not it is still kept; a token whose mass rounds to 0 takes part in nothing) and
 * l_i = s_i - s_max in fp32:
 *   min_p           keep iff p_i >= min_p * max_K p
 *   typical_p       H = -sum_K p_i ln p_i, d_i = |-ln p_i - H| = |l_i - E_p[l]| (fp32); keep iff the mass of the tokens of K with a
 *                   strictly smaller d is < typical_p * Z_K: every tie in d is kept, the token of smallest d always stays.  The kept
 *                   set becomes a band of scores, which may exclude the arg-max
 *   epsilon_cutoff  keep iff p_i >= epsilon_cutoff
 *   eta_cutoff      eta = min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)), H the entropy over the current K; keep iff p_i >= eta
 * The largest score of K always stays (min_tokens_to_keep = 1).  Entropies and softmaxes are exact where HF rounds them to fp16;
 * E_p[l] is summed in double in a fixed order, every other sum is an exact integer, so a row's result depends on that row and its
 * records only.  The log-probabilities of vstar_vqa_logprobs stay those of the un-warped row. */
typedef struct vstar_vqa_warpers {    /* 16 bytes */
  float min_p;            /* [0, 1]; 0 = off */
  float typical_p;        /* > 0; >= 1 = off */
  float epsilon_cutoff;   /* [0, 1); 0 = off */
  float eta_cutoff;       /* [0, 1); 0 = off */
} vstar_vqa_warpers;

/* vstar_vqa_forward_sample_logprobs / _forward_verify_logprobs with one vstar_vqa_warpers record per wanted row (host, parallel to
 * params); edits and lp stay nullable.  warpers == NULL is the _logprobs call, bit for bit and launch for launch; records that are
 * all off give its bits too.  A greedy verify (params == NULL) checks the records and ignores them, as it has no top-k / top-p.
 * Errors (VSTAR_ERR_INVALID, before any device work, the engine stays usable): a NaN or negative value, min_p > 1, typical_p <= 0,
 * a cutoff >= 1; the message names the field.  The device array for the records is allocated by the first call that carries them
 * (a failed allocation is VSTAR_ERR_NOMEM and leaves the engine usable); a call without them allocates and copies nothing. */
int vstar_vqa_forward_sample_warp(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src,
                                  const int32_t* kv_slot, const int32_t* prefix_slot, const int32_t* past_len,
                                  int n_want, const int32_t* want, const vstar_vqa_sampling* params, int32_t* tokens,
                                  const vstar_vqa_warpers* warpers, const vstar_vqa_logit_edits* edits, const vstar_vqa_logprobs* lp);
int vstar_vqa_forward_verify_warp(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                                  const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                                  const vstar_vqa_sampling* params, const int32_t* group_off, int n_groups, const int32_t* draft,
                                  int32_t* n_accept_out, int32_t* tokens_out, const vstar_vqa_warpers* warpers,
                                  const vstar_vqa_logit_edits* edits, const vstar_vqa_logprobs* lp);
/* Op-level (tests, micro-benchmarks): vstar_vqa_op_sample / vstar_vqa_op_verify with host warpers[rows] (nullable: the plain op).
 * kept_mask (nullable diagnostic, host, uint8 [rows, vocab]): 1 where the token is in the kept set the draw was made from. */
int vstar_vqa_op_sample_warp(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* params,
                             const vstar_vqa_warpers* warpers, int32_t* tokens, float* u_out, int32_t* n_kept, uint8_t* kept_mask);
int vstar_vqa_op_verify_warp(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* group_off,
                             int n_groups, const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers,
                             int32_t* n_accept_out, int32_t* tokens_out);

/* Op-level (tests, micro-benchmarks): DEVICE logits [rows, ld] of dtype F16/BF16 (1 <= vocab <= 2^22, rows <= 65535, any ld >=
 * vocab); host tokens[rows] (a negative token: the row is not read) and outputs as above with n_want = rows; token_rank nullable,
 * top_logprob / top_token null iff n_top == 0.  n_top outside [0, 32] or a token >= vocab is VSTAR_ERR_INVALID with a message, before
 * any device work.  Null stream, synchronises. */
int vstar_vqa_op_logprobs(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* tokens, int n_top,
                          float* token_logprob, int32_t* token_rank, float* top_logprob, int32_t* top_token);

/* Contrastive search: HF 4.31 generate(penalty_alpha = alpha, top_k = k) — contrastive_search + _ranking_fast — with
 * the degeneration penalty, the pick, the next candidates and the carry-over of the winner on the device.  Per sequence the engine
 * keeps the hidden history Hs[0 .. L): the final-norm output (LlamaModel.norm, HF's hidden_states[-1]) of every position so far,
 * spliced image / object rows included, fp16, with the fp32 reciprocal norm of every row; hist_len[slot] = L (host).  T tokens cost
 * one begin call plus T step calls.  The history ([max_slots][max_ctx][llm_hidden] fp16 + [max_slots][max_ctx] fp32 =
 * max_slots * max_ctx * (2 * llm_hidden + 4) bytes) and the step's buffers are allocated by the first contrast call (a failed
 * allocation is VSTAR_ERR_NOMEM and leaves the engine usable); an engine that never asks allocates and launches nothing.  Once the
 * history exists every other call that writes K/V rows of a slot at position p lowers hist_len[slot] to min(hist_len, p) (host
 * arithmetic): stale history is never read.
 * The arithmetic (csrc/contrast.hpp states it in full): hidden rows h(w * h(x * rstd)), one routine for prefill and candidate rows;
 * cos = dot * rnorm_c * rnorm_j with the dot and the squared norms in fp32 in one fixed order (a result depends on its own inputs
 * only and repeats bit for bit), a zero-norm row gives cosine 0 (HF: NaN — a stated deviation); pen_c = max_{j < L} cos(h_c, Hs[j]);
 * score_c = (1 - alpha) * p_c - alpha * pen_c in double from the fp32 p and pen and the fp32 alpha, every operation rounded on its
 * own, so the pick — the largest score, the lowest c on a tie — is reproducible exactly from the returned p and pen; the top k of a
 * logits row in vstar_vqa_logprobs' top-n order with p = (float)exp((double)x - lse), lse the scoring tail's double log-sum-exp.
 * Probabilities and cosines are exact where HF rounds them to fp16.
 *
 * begin: a vstar_vqa_forward prefill (the eight row arguments) that writes the hidden row of EVERY new row into the history of its
 * kv_slot and returns, per wanted row, the k (2 .. 32, <= llm_vocab) best tokens and their probabilities, next_tok / next_prob
 * [n_want, k] (host).  Rules: prefix_slot == kv_slot; past_len == 0 (a fresh sequence: the history starts again) or == hist_len[kv_slot]
 * (a chunked prefill continues it); the kv_slots pairwise distinct.  Afterwards hist_len[kv_slot] = past_len + rows. */
int vstar_vqa_forward_contrast_begin(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                                     const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want, int k,
                                     int32_t* next_tok, float* next_prob);
/* step: the k candidates of each sequence as one-row continuations.  Every sequence of the call has exactly one row and wanted row j
 * is row j (n_want == nseq); rows group_off[g] .. group_off[g+1]-1 (1 .. 32 of them) are group g: they share prefix_slot (the owner)
 * and past_len == hist_len[owner] (>= 1), their kv_slots are pairwise distinct over the whole call (one of a group's may be its owner;
 * none may be another group's owner); cand_prob[n_want] finite and in [0, 1]; alpha in [0, 1]; k_next in [2, 32], <= llm_vocab.  Per
 * group g: sel_out[g] = the winner (row in group), next_tok / next_prob [n_groups, k_next] = the top k_next of the winner's logits row,
 * penalty_out[n_want] (nullable) = pen of every candidate; the winner's hidden row becomes Hs[L] and its K/V row becomes row L of the
 * owner slot in every layer (copied on the device unless its kv_slot is the owner: 128 code bytes + 4 scale bytes per row in
 * kv_cache_format 1, else the fp16 row).  Afterwards hist_len[owner] = L + 1, and the history of every other candidate slot is empty.
 * A violation is VSTAR_ERR_INVALID with a message that names the field, before any launch; the engine stays usable.  Logits edits and
 * log-probabilities are not available with these two entries (open follow-ups). */
int vstar_vqa_forward_contrast_step(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                                    const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                                    const int32_t* group_off, int n_groups, const float* cand_prob, float alpha, int k_next,
                                    int32_t* sel_out, int32_t* next_tok, float* next_prob, float* penalty_out);
/* Op-level (tests, micro-benchmarks): the step behind lm_head.  DEVICE: logits [rows, ld] and candidate hidden rows [rows, hidden] of
 * dtype F16/BF16 (both), the history dev_hist [n_groups, cap, hidden] of that dtype and dev_hist_rnorm [n_groups, cap] fp32, group g's
 * first hist_len[g] rows valid; the winner's row and reciprocal norm are appended IN PLACE at row hist_len[g].  HOST: hist_len
 * [n_groups], group_off [n_groups + 1], cand_prob [rows] and the outputs of the step (penalty_out nullable).  Checked before any device
 * work (VSTAR_ERR_INVALID, the message names the field): a NULL pointer, hidden % 8 != 0, hist_len outside [1, cap), and the step's
 * rules.  Null stream, synchronises. */
int vstar_vqa_op_contrast(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const void* dev_cand_hidden, int hidden,
                          void* dev_hist, float* dev_hist_rnorm, int n_groups, int cap, const int32_t* hist_len, const int32_t* group_off,
                          const float* cand_prob, float alpha, int k_next, int32_t* sel_out, int32_t* next_tok, float* next_prob,
                          float* penalty_out);

/* Guided decoding against a negative sequence: HF generate(guidance_scale = gamma, negative_prompt_ids = ...) —
 * UnbatchedClassifierFreeGuidanceLogitsProcessor, "visual contrastive decoding" when the negative sequence is the same question without
 * (or with a degraded) image — with the combination of the two logits rows on the device, ahead of the logits edits (HF puts the
 * guidance processor first in its list): lm_head -> guide -> edits -> tail -> log-probabilities.  The wanted rows of a guided call are
 * the n_out OUTPUT rows want[0 .. n_out) followed by the NEGATIVE rows want[n_out .. n_want); every array of the tail, the edits and the
 * log-probabilities (params, warpers, tokens, argmax, logits_f16, off / penalty, token_logprob ...) has n_out entries and describes the
 * output rows.  All arrays HOST, n_out entries:
 *   neg[j]       index into `want` (>= n_out) of output row j's negative row, each negative row belonging to exactly one output row;
 *                -1: row j is unguided (its logits pass through untouched)
 *   scale[j]     gamma, finite and >= 0 (1 gives log_softmax of the row itself, 0 that of the negative row); read where neg[j] >= 0
 *   log_beta[j]  <= 0: the adaptive plausibility cut of Li et al. — token i stays iff x_c[i] - max x_c >= log_beta (an exact fp32
 *                difference of fp16 values), every other token becomes -inf; -inf = off; the caller passes float32(log(beta))
 * With x_c / x_u the two logits rows: lse = max + log(sum exp(x_i - max)) in double in vstar_vqa_forward_score's fixed order, c_i =
 * x_c[i] - lse_c, u_i = x_u[i] - lse_u, g_i = gamma * (c_i - u_i) + u_i in double (every operation rounded on its own), rounded ONCE to
 * fp16; a finite g_i beyond the fp16 range becomes +-65504.  x_c[i] = -inf or NaN gives -inf; x_u[i] non-finite with x_c[i] finite gives
 * c_i rounded once; a non-finite lse_c or lse_u gives a row of -inf.  The guided row replaces the output row's logits: the edits, the
 * tail and the log-probabilities see it, and logits_f16 returns it (HF's `scores`).  HF computes both log_softmax in the scores' dtype
 * and rounds after every operation; here the value is exact and rounded once (a stated deviation).  Negative rows only write their K/V. */
typedef struct vstar_vqa_guidance {   /* all HOST arrays */
  int32_t        n_out;       /* output rows: the first n_out wanted rows */
  const int32_t* neg;         /* [n_out] */
  const float*   scale;       /* [n_out] */
  const float*   log_beta;    /* [n_out] */
} vstar_vqa_guidance;

/* vstar_vqa_forward_logprobs / vstar_vqa_forward_sample_warp with the guidance stage; warpers, edits and lp stay nullable, guidance ==
 * NULL is that call, bit for bit and launch for launch.  Errors (VSTAR_ERR_INVALID, before any device work, the engine stays usable):
 * n_out outside [1, n_want], a neg entry that is neither -1 nor in [n_out, n_want), a negative row with no or with two output rows, a
 * scale or log_beta out of range.  The device arrays for the records are allocated by the first call that carries guidance (a failed
 * allocation is VSTAR_ERR_NOMEM and leaves the engine usable); an engine that never sees guidance allocates, launches and copies nothing
 * for it.  The beam, scoring, verify and contrast tails have no such entry. */
int vstar_vqa_forward_guided(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src, const int32_t* kv_slot,
                             const int32_t* prefix_slot, const int32_t* past_len, int n_want, const int32_t* want,
                             uint16_t* logits_f16, int32_t* argmax, const vstar_vqa_guidance* guidance,
                             const vstar_vqa_logit_edits* edits, const vstar_vqa_logprobs* lp);
int vstar_vqa_forward_sample_guided(vstar_vqa_handle* h, int nseq, const int32_t* row_off, const int32_t* src,
                                    const int32_t* kv_slot, const int32_t* prefix_slot, const int32_t* past_len,
                                    int n_want, const int32_t* want, const vstar_vqa_sampling* params, int32_t* tokens,
                                    const vstar_vqa_warpers* warpers, const vstar_vqa_guidance* guidance,
                                    const vstar_vqa_logit_edits* edits, const vstar_vqa_logprobs* lp);
/* Kernel-level door (tests, micro-benchmarks): DEVICE logits [rows, ld] of dtype F16/BF16 (1 <= vocab <= 2^22, any ld >= vocab); host
 * records of n_pairs (<= 65535) pairs: cond_row / neg_row (two different rows in [0, rows), no row in two records), scale (finite, >= 0),
 * log_beta (<= 0, -inf = off), checked before any device work.  Row cond_row[p] is overwritten in place, columns [0, vocab) only; no other
 * element is written.  Null stream, synchronises. */
int vstar_vqa_guide_rows(void* dev_logits, int dtype, int rows, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row,
                         const int32_t* neg_row, const float* scale, const float* log_beta);

/* Op-level entry for tests and micro-benchmarks, fp16, all pointers DEVICE pointers: C[M,N] = epilogue(A[M,K] · W[N,K]^T
 * + bias) (+ residual), epilogue codes and operand rules as vstar_op_gemm (W rows padded to a multiple of 256, K % 64 == 0).
 * kernel: 0 = the engine's dispatch (weight-streaming kernel for M <= 64, MFMA tile kernels otherwise), 1 = force the
 * weight-streaming kernel (M <= 64; for M <= 8 that is its LDS-ring variant), 2 = force the tile kernels, 3 = the weight-streaming
 * kernel with the weights through registers even where the LDS-ring variant would run (bit-identity tests), 4 = the 4-wave / AGPR
 * 256x256 tile kernel (gemm4w, round 6; error outside its domain), 5 = the 8-wave 256x256 kernel.  dev_norm_w (nullable, weight-streaming kernel only):
 * LlamaRMSNorm gains [K]; the rows of A are RMS-normalised (eps = norm_eps) while they are loaded, as the decode path
 * does for input_layernorm -> q/k/v and post_attention_layernorm -> gate/up.  Runs on the null stream and synchronises. */
int vstar_vqa_op_gemm(const void* dev_A, const void* dev_W, const void* dev_bias, const void* dev_residual, void* dev_C,
                      int M, int N, int K, int epilogue, int kernel, const void* dev_norm_w, float norm_eps);

/* int8 weight-only decode (W8A16), opt-in through vstar_vqa_config.decode_weight_bits = 8.  finalize_weights then
 * quantises the LLaMA block linears once, on the device, per output row n of W[N, K]: a = max_k |W[n,k]|, s = float(a) / 127.0f
 * (one correctly rounded fp32 divide; s = 1 when a == 0), q[n,k] = clamp(rint(float(W[n,k]) / s), -127, 127) as int8 (-128 never
 * occurs).  Calls of up to 64 rows (decode steps) stream the int8 weights through the weight-streaming kernels — every MFMA sees
 * fp16(q), exact, and the reduced fp32 accumulator is multiplied once by s — while the fp16 weights are REPLACED by
 * fp16(float(q) * s), so prefill and larger calls run the same quantised model on the tile kernels.  lm_head, the embedding, the
 * CLIP tower, the projectors and the Perceiver stay fp16.  A failed allocation fails finalize_weights (no fp16 fallback).
 * Returns 8 when the mode is active on a finalized engine, 4 in the int4 group-scaled mode (below), else 0. */
int vstar_vqa_decode_weight_bits(const vstar_vqa_handle* h);
/* Op-level quantiser (tests): DEVICE W [rows, K] fp16 (K % 8 == 0) -> q int8 [rows, K], scale fp32 [rows], and (nullable, may
 * alias W) What fp16 [rows, K] = fp16(float(q) * s).  Null stream, synchronises. */
int vstar_vqa_op_quantize_w8(const void* dev_W_f16, int rows, int K, void* dev_q_i8, float* dev_scale_f32, void* dev_What_f16);
/* Op-level W8A16 GEMV (tests, micro-benchmarks): vstar_vqa_op_gemm with the weight given as int8 rows dev_Wq [ceil(N/256)*256, K]
 * and fp32 scales dev_scale [ceil(N/256)*256]: C = epilogue((A · fp16(q)^T) * s + bias) (+ residual), operand rules as
 * vstar_vqa_op_gemm.  kernel: 1 = dispatch (the LDS-ring variant where eligible), 3 = force the register-streaming kernel.
 * layout: 0 = the ring reads the row-major int8, 1 = the op packs a temporary tile-major image and the ring reads that (needs
 * N % 16 == 0, SiLU-mul N % 32 == 0).  Outside the weight-streaming domain (M > 64) it is an error. */
int vstar_vqa_op_gemm_w8(const void* dev_A, const void* dev_Wq, const float* dev_scale, const void* dev_bias,
                         const void* dev_residual, void* dev_C, int M, int N, int K, int epilogue, int kernel,
                         const void* dev_norm_w, float norm_eps, int layout);

/* int4 group-scaled weight-only decode (W4A16, groups of 128), opt-in through
 * vstar_vqa_config.decode_weight_format = VSTAR_VQA_WFMT_W4G128 (decode_weight_bits stays 0: the value 4 there keeps failing at
 * create).  finalize_weights quantises the LLaMA block linears once, on the device, per row n of W[N, K] and group j = k / 128
 * (fp32 unless said otherwise): a = max |W[n, 128 j .. 128 j + 127]|, s = fp16(float(a) / 7.0f) (one correctly rounded divide,
 * one round-to-nearest-even conversion), s = min(s, 9352) (7 * 9352 is finite in fp16), s = 1 if s == 0,
 * q = clamp(rint(float(W) / float(s)), -7, 7) (-8 is never produced), What = fp16(q) * s as ONE fp16 multiply (subnormals kept).
 * Storage: u = q + 8 in 1..15 (0 decodes to -8); eight elements per little-endian 32-bit word, element e in nibble
 * (e >> 1) + 4 (e & 1); row-major image uint32 [Npad, K / 8], scales fp16 [Npad, K / 128], Npad = ceil(N / 256) * 256, padding
 * rows q = 0 (u = 8), s = 1.  Calls of up to 64 rows stream the words through the W4 form of the register weight-streaming kernel,
 * which applies the group scale to the weights in registers: every MFMA sees exactly What, so the call is BIT-IDENTICAL to the fp16
 * kernel on What — and the fp16 weights are REPLACED by What, so prefill and larger calls run the same quantised model.  There is no
 * LDS-ring form: decode steps of up to 8 sequences take the register kernel too, which reads a tile-major image of the words and
 * scales (one coalesced 1-KiB load per wave and pair of its double steps) unless VSTAR_DECODE_TILED=0.  lm_head, the embedding, the CLIP tower, the
 * projectors and the Perceiver stay fp16.  vstar_vqa_decode_weight_bits returns 4 on a finalized engine in this mode. */
/* Op-level quantiser (tests): DEVICE W [rows, K] fp16 (K % 128 == 0) -> q uint32 [rows, K / 8], scale fp16 [rows, K / 128], and
 * (nullable, may alias W) What fp16 [rows, K].  Null stream, synchronises. */
int vstar_vqa_op_quantize_w4(const void* dev_W_f16, int rows, int K, void* dev_q_u32, void* dev_scale_f16, void* dev_What_f16);
/* Op-level W4A16 GEMV (tests, micro-benchmarks): vstar_vqa_op_gemm_w8's parameter list and meanings with the weight given as words
 * dev_Wq [ceil(N/256)*256, K / 8] and fp16 scales dev_scale [ceil(N/256)*256, K / 128] (K % 128 == 0):
 * C = epilogue(A · (fp16(q) * s)^T + bias) (+ residual).  kernel: 1 = dispatch, 3 = force the register-streaming kernel (both run
 * it: there is no W4 ring).  layout: 0 = the kernel reads the row-major words and scales, 1 = the op packs a temporary tile-major
 * image and the kernel reads that (needs N % 16 == 0, SiLU-mul N % 32 == 0).  M > 64 is an error. */
int vstar_vqa_op_gemm_w4(const void* dev_A, const void* dev_Wq, const void* dev_scale, const void* dev_bias,
                         const void* dev_residual, void* dev_C, int M, int N, int K, int epilogue, int kernel,
                         const void* dev_norm_w, float norm_eps, int layout);

/* Block-scaled fp8 KV cache, opt-in through vstar_vqa_config.kv_cache_format.  Every cached row — the 128 values of
 * one (layer, slot, head, position) of K (after RoPE) and likewise of V — is cut into 4 blocks of 32 consecutive head-dim elements;
 * a block stores one E8M0 byte e, 2^(e - 127) being the smallest power of two that brings the block's largest magnitude to <= 448
 * (integer arithmetic on the fp32 bits of amax = 1.f x 2^E: e = E + 127 - 8, one more when 1.f > 1.75; 0 for an all-zero block), and
 * the OCP e4m3 codes rne_e4m3(x * 2^(127 - e)).  The row's value is code * 2^(e - 127) from then on, for every reader: the prefill
 * attends to the round-tripped K and V too, and a decode step attends to its own row's round-tripped values.
 *   VSTAR_VQA_KVFMT_MXFP8 (1): codes u8 [layer][slot][head][ctx][128] and scale bytes u8 [layer][slot][head][ctx][4], for K and for V;
 *     the attention kernels decode in registers (one exact fp32 multiply per element) and are otherwise the fp16 kernels: same lane
 *     geometry, same accumulation order.
 *   VSTAR_VQA_KVFMT_MXFP8_EMULATED (2): the fp16 cache and the fp16 readers; the writers store fp16(code * 2^(e - 127)).
 * For fp16 inputs with |x| < 63488 the decoded value is exactly representable in fp16, so an engine in mode 1 is BIT-IDENTICAL to one in
 * mode 2 in every call.  Rows holding |x| >= 63488 (the top grid point decodes to 65536, +inf in fp16) or non-finite values are outside
 * that claim; they do not fault.  fp16 engine only.  Returns the active format (the config's value). */
int vstar_vqa_kv_cache_format(const vstar_vqa_handle* h);
/* Bytes of K plus V storage of a finalized engine, scale bytes included: 2 * layers * max_slots * heads * max_ctx * 128 * 2 in formats 0
 * and 2, 2 * layers * max_slots * heads * max_ctx * 132 in format 1 (0 before finalize_weights). */
int64_t vstar_vqa_kv_cache_bytes(const vstar_vqa_handle* h);
/* Op-level quantiser (tests): DEVICE x [rows, 128] fp16 -> codes u8 [rows, 128], scale bytes u8 [rows, 4] and (nullable, may alias x)
 * xhat fp16 [rows, 128] = the decoded row, through the device function every mode-1 / mode-2 writer quantises with.  Null stream,
 * synchronises. */
int vstar_vqa_op_kv_quantize(const void* dev_x_f16, int rows, void* dev_codes_u8, void* dev_scales_u8, void* dev_xhat_f16);

/* Op-level doors of the decode-side kernels (decode.hip; tests/test_decode_ops_gpu.py).  fp16 only, null stream, synchronise.  Data
 * tensors are DEVICE pointers; every index array is a HOST pointer that the door checks against the extents given here and uploads
 * itself, so no input can make a kernel index outside an allocation.  A violated rule is VSTAR_ERR_INVALID with a message, before
 * anything is launched or allocated.
 * vstar_vqa_kv_view / vstar_vqa_kv_rows — one layer of a KV cache and the host index arrays of one call — are declared, with their
 * rules, in vstar_hip.h (which this header includes): the bf16 doors vstar_op_rope_kv_append / vstar_op_cached_attention take the same
 * structs.  Here fmt is 0, 1 or 2 (vstar_vqa_kv_cache_format above). */
/* rope_kv_append on dev_qkv [R, 3 * heads * 128] (q | k | v) with the table dev_cos_sin [table_rows, 128] (cos[64] | sin[64]). */
int vstar_vqa_op_rope_kv_append(void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                                const vstar_vqa_kv_rows* rows);
/* cached_attention -> dev_out [R, heads * 128].  path 0: the rows are already rotated and appended (the un-fused kernel; dev_cos_sin
 * is not read); path 1: fused, unsplit (no workspace is passed); path 2: fused split-KV, on a workspace the door allocates for R rows
 * and zero-fills once.  The op is launched `repeat` (>= 1) times back to back on that workspace (the fused writers are idempotent).
 * *path_ran = what the dispatcher launched.  Further rules: row_pos + 1 <= max_keys <= ctx; paths 1 and 2: no padding rows, exactly
 * one row per sequence, pairwise distinct seq_kv, row_slot[r] == seq_kv[row_seq[r]]; paths 0 and 1: (128 + max_keys) * 4 <= 40 KiB;
 * path 2 where the dispatcher would not split (R * heads > 128, max_keys < 256, VSTAR_DECODE_SPLIT_KV=0) is an error, never a
 * silent fall-back. */
int vstar_vqa_op_cached_attention(void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                                  const vstar_vqa_kv_rows* rows, int max_keys, int path, int repeat, void* dev_out, int* path_ran);
/* perceiver_attention: dev_q [n * L, H * DH], dev_kv [n * NK, 2 * H * DH] (k | v) -> dev_out [n * L, H * DH]; DH in {32, 64, 96},
 * 1 <= NK <= 512. */
int vstar_vqa_op_perceiver_attention(const void* dev_q, const void* dev_kv, void* dev_out, int n, int L, int NK, int H, int DH);
/* embed_rows: dev_x [R, C] = host_src[r] >= 0 ? dev_table[src] (zero when src >= vocab) : src == INT32_MIN ? 0 :
 * dev_feats[-(src + 1)] (zero when that is >= n_feat_rows; dev_feats nullable when n_feat_rows == 0); C % 8 == 0. */
int vstar_vqa_op_embed_rows(const int32_t* host_src, int R, const void* dev_table, int vocab, const void* dev_feats,
                            int64_t n_feat_rows, void* dev_x, int C);
/* argmax_rows_lp on dev_x [rows, ld] (ld >= cols) -> host_out [rows]. */
int vstar_vqa_op_argmax_rows(const void* dev_x, int rows, int cols, int64_t ld, int32_t* host_out);

/* Op-level doors of the fp16 PREFILL kernels — the -DVSTAR_LP_F16 build of attention.hip, norm.hip and elementwise.hip that every VQA
 * prefill, the fp16 CLIP tower and the Perceiver run (tests/test_f16_prefill_gpu.py).  fp16 only, null stream, one launch, synchronise.
 * Data tensors are DEVICE pointers and every buffer comes with its extent in rows; a violated rule is VSTAR_ERR_INVALID with a message,
 * before anything is allocated or launched.  The doors do no arithmetic of their own.
 * attention: attn_forward alone (no RoPE, no grouped sequences) on dev_qkv [qkv_rows >= B * S, 3 * H * D] (q | k | v) -> dev_out
 * [out_rows >= B * S, H * D], scale 1 / sqrtf(D); D in {64, 128}, causal 0 or 1, 1 <= H <= 256, B * S <= 2^24, S * 3 * H * D * 2 < 2^31. */
int vstar_vqa_op_attention(const void* dev_qkv, int64_t qkv_rows, void* dev_out, int64_t out_rows, int B, int S, int H, int D, int causal);
/* layernorm_lp: dev_y [rows, cols] = LN(dev_x[host_row_index ? host_row_index[r] : r]) * dev_gamma [cols] + dev_beta [cols] (nullable);
 * act 1: exact-erf GELU of the fp16-rounded affine result.  dev_x [x_rows, cols]; host_row_index (nullable, HOST, [rows]) is checked
 * against x_rows and uploaded by the door; without it x_rows >= rows.  cols % 8 == 0, 8 <= cols <= 4096, 1 <= rows <= 2^20. */
int vstar_vqa_op_layernorm(const void* dev_x, int64_t x_rows, const void* dev_gamma, const void* dev_beta, void* dev_y, int rows, int cols,
                           float eps, const int32_t* host_row_index, int act);
/* rmsnorm_lp (LlamaRMSNorm: gamma * fp16(x * rstd)); arguments and rules as vstar_vqa_op_layernorm. */
int vstar_vqa_op_rmsnorm(const void* dev_x, int64_t x_rows, const void* dev_gamma, void* dev_y, int rows, int cols, float eps,
                         const int32_t* host_row_index);
/* add_bcast: dev_out [rows, cols] = dev_a [rows, cols] + dev_b [b_rows, cols][r % b_rows], one fp32 add rounded once; cols % 8 == 0,
 * 1 <= b_rows <= rows <= 2^24. */
int vstar_vqa_op_add_bcast(const void* dev_a, const void* dev_b, void* dev_out, int64_t rows, int cols, int64_t b_rows);
/* vit_assemble_tokens: dev_tokens [B * (P + 1), C] = cat([dev_cls [C], dev_patch [B, P, C]]) + dev_pos [P + 1, C]; C % 8 == 0. */
int vstar_vqa_op_vit_assemble_tokens(const void* dev_patch, const void* dev_cls, const void* dev_pos, void* dev_tokens, int B, int P, int C);

/* Diagnostics for the parity tests: "features" = the whole feature table, fp16 -> float; "kv:<layer>:<slot>" = the DECODED K then V
 * cache of that layer and slot as floats [2][llm_heads][max_ctx][128], in every kv_cache_format (an index out of range is an error);
 * "contrast_hist:<slot>" = the hidden history of that slot [hist_len, llm_hidden], "contrast_cand" = the candidate hidden rows of the
 * last contrast step [rows, llm_hidden] (both VSTAR_ERR_STATE on an engine that ran no contrast call).
 * Returns elements written. */
int64_t vstar_vqa_debug_read(vstar_vqa_handle* h, const char* name, float* out, int64_t capacity);
/* Timing of the last forward call in milliseconds (HIP events on the engine stream). */
double vstar_vqa_last_forward_ms(const vstar_vqa_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* VSTAR_VQA_H */
