// llm_cached.hpp — the KV-cached LLaMA runner shared by the two engines (dtype-generic, VS_NS): the VQA-LLM's forward
// (LLaVA/llava/model/language_model/llava_search_llama.py:56-113) and the VSM's free-text decode for the contextual-cue
// branch (VSMForCausalLM.inference mode='vqa', VisualSearch/model/VSM.py:438-462 / visual_search.py:427-443).
// It owns the KV cache, the activations and the row metadata; the weights belong to the engine that built them.
//
// One forward call advances nseq sequences by any number of new rows each, in one of two regimes:
//   * prefill  (every past_len == 0 and more than 64 new rows): sequences right-padded to a common length, the MFMA tile
//     GEMMs and the flash-attention kernel; K/V rows are stored into the cache on the way.
//   * cached   (decode steps, option continuations): flat ragged rows, weight-streaming skinny GEMMs (M <= 64), attention
//     straight out of the KV cache with an optional shared prefix slot.
#pragma once
#include "engine_base.hpp"
#include <array>
#include "tails_lp.hpp"

namespace VS_NS {

// The new rows of one forward() call: the eight row arguments of vstar_vqa_forward, documented there (include/vstar_vqa.h);
// host arrays.
struct LlmRows {
  int nseq = 0;
  const int32_t *row_off = nullptr, *src = nullptr, *kv_slot = nullptr, *prefix_slot = nullptr, *past_len = nullptr;
  int n_want = 0;
  const int32_t* want = nullptr;
};

// The beam-search tail of forward() (beam.hip): host arrays.  The wanted rows carry scores[n_want] and form
// n_groups groups (rows goff[g] .. goff[g+1]-1 of `want`); each group's n_cand best (score, token, row in group) come back.
struct LlmBeamArgs {
  const float* scores = nullptr;
  int n_groups = 0;
  const int32_t* goff = nullptr;
  int n_cand = 0;
  float* cand_s = nullptr;
  int32_t* cand_tok = nullptr;
  int32_t* cand_row = nullptr;
};

// The scoring tail of forward() (score.hip): host arrays.  Wanted row j is scored against targets[j]; nll[j]
// (and rank[j], nullable) come back.  A row may be wanted several times with different targets.
// CHUNKING RULE (part of the contract — lm_head's row count selects its GEMM kernel): this tail alone accepts n_want up to
// max_rows; the wanted rows are processed in consecutive chunks of max_want (256) rows, the last one shorter, each chunk
// gather -> final norm -> lm_head -> score through the one [max_want, vpad] logits buffer.  So wanted rows [256 c, 256 (c + 1))
// see the lm_head a plain forward() with exactly those wanted rows runs.
struct LlmScoreArgs {
  const int32_t* targets = nullptr;
  float* nll = nullptr;
  int32_t* rank = nullptr;
};

// The verify tail of forward() (spec.hip): host arrays.  The wanted rows form n_groups groups (rows goff[g] ..
// goff[g+1]-1 of `want`: consecutive-or-later rows of ONE sequence in position order); wanted row j's choice is compared with
// draft[j] (-1: not compared; always -1 on a group's last row).  n_accept[n_groups] and tokens[n_want] come back.  Greedy unless
// the tail also carries sampling records (one per wanted row).
struct LlmVerifyArgs {
  int n_groups = 0;
  const int32_t* goff = nullptr;
  const int32_t* draft = nullptr;
  int32_t* n_accept = nullptr;
  int32_t* tokens = nullptr;
};

// The logits edits of forward() (edit.hip): host arrays, one triple of sorted token lists per wanted row in one CSR
// array — row j's penalised ids tok[off[3j] .. off[3j+1]), banned ids tok[off[3j+1] .. off[3j+2]), allowed ids tok[off[3j+2] ..
// off[3j+3]) — and penalty[n_want], read where the penalised list is non-empty.  Applied to the wanted rows' logits between
// lm_head and the tail, which then sees the edited rows; ARGMAX, SAMPLE and VERIFY tails only.
struct LlmEdits {
  const int32_t* off = nullptr;
  const int32_t* tok = nullptr;
  const float* penalty = nullptr;
};

// The log-probability stage of forward() (logprob.hip): host arrays.  Behind an ARGMAX, SAMPLE or VERIFY tail, on
// the logits rows that tail just read (the EDITED rows when the call carries edits) and the tokens it just chose: per wanted row j
// the chosen token's log-probability lp_out[j] and rank rank_out[j] (nullable), and the n_top (0 .. 32) best alternatives
// top_tok_out / top_lp_out [n_want, n_top] (null iff n_top == 0).  A verify row behind the acceptance (token -1) gives NaN / -1.
struct LlmLogprobArgs {
  int n_top = 0;
  float* lp_out = nullptr;
  int32_t* rank_out = nullptr;
  float* top_lp_out = nullptr;
  int32_t* top_tok_out = nullptr;
};

// The guidance stage of forward() (guide.hip): host arrays of n_out entries.  The first n_out wanted rows of the
// call are its OUTPUT rows, wanted rows [n_out, n_want) its NEGATIVE rows; neg[j] = the wanted-row index (>= n_out) of output row j's
// negative row (every negative row belongs to exactly one output row) or -1 (row j is unguided), scale[j] = gamma, log_beta[j] <= 0
// (-inf: no plausibility cut).  Between lm_head and the edits the logits of output row j become the guided row; the tail, the edits,
// the log-probabilities and all their arrays then have n_out entries and run on rows [0, n_out) of the logits buffer.  ARGMAX and
// SAMPLE tails only.
struct LlmGuide {
  int n_out = 0;
  const int32_t* neg = nullptr;
  const float* scale = nullptr;
  const float* log_beta = nullptr;
};

// The contrastive-search tail of forward() (contrast.hip): host arrays.  goff == null: the BEGIN call — a prefill
// (prefix_slot == kv_slot, past_len == the slot's history length or 0) whose new rows' final-norm hidden rows fill the history of
// their slot, and per wanted row the k best tokens and their probabilities come back, next_tok / next_prob [n_want, k].  goff given:
// a STEP — every sequence one row, wanted row j = row j; rows goff[g] .. goff[g+1]-1 are the candidates of group g, continuations of
// one owner (their common prefix_slot) at past_len == the owner's history length, each into a kv_slot of its own (one may be the
// owner); cand_prob[n_want] their probabilities.  sel[n_groups], next_tok / next_prob [n_groups, k] and (nullable) pen_out[n_want]
// come back; the winner's hidden row joins the owner's history and its K/V row becomes the owner's.
struct LlmContrastArgs {
  int k = 0;
  int32_t* next_tok = nullptr;
  float* next_prob = nullptr;
  int n_groups = 0;
  const int32_t* goff = nullptr;
  const float* cand_prob = nullptr;
  float alpha = 0.f;
  int32_t* sel = nullptr;
  float* pen_out = nullptr;
};

struct LlmCached;

// What forward() does with the wanted rows' logits: exactly one of the six tails, built by the function of its name — so a call
// cannot ask for two tails, or for a tail together with an output that tail does not have.
struct LlmTail {
  enum Kind { ARGMAX, SAMPLE, BEAM, SCORE, VERIFY, CONTRAST };
  static LlmTail argmax(uint16_t* logits_out, int32_t* argmax_out) { LlmTail t; t.logits_out = logits_out; t.tokens_out = argmax_out; return t; }
  static LlmTail sample(const vstar_vqa_sampling* params, int32_t* tokens, const vstar_vqa_warpers* warpers = nullptr) { LlmTail t; t.kind = SAMPLE; t.params = params; t.tokens_out = tokens; t.warpers = warpers; return t; }
  static LlmTail beam_select(const LlmBeamArgs& b, uint16_t* logits_out) { LlmTail t; t.kind = BEAM; t.beam = b; t.logits_out = logits_out; return t; }
  static LlmTail score_rows(const LlmScoreArgs& sc) { LlmTail t; t.kind = SCORE; t.score = sc; return t; }
  static LlmTail verify_rows(const LlmVerifyArgs& v, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers = nullptr) { LlmTail t; t.kind = VERIFY; t.verify = v; t.params = params; t.warpers = warpers; return t; }
  static LlmTail contrast(const LlmContrastArgs& c) { LlmTail t; t.kind = CONTRAST; t.con = c; return t; }
  // the tail with the log-probability stage behind it (null: the tail as it is); refused on BEAM and SCORE by tail_check
  LlmTail with_logprobs(const LlmLogprobArgs* lp) const { LlmTail t = *this; t.has_lp = lp != nullptr; if (lp) t.lp = *lp; return t; }

 private:      // only the functions above fill these, only LlmCached reads them
  friend struct LlmCached;
  LlmTail() = default;
  Kind kind = ARGMAX;
  uint16_t* logits_out = nullptr;                // ARGMAX, BEAM (nullable): the wanted rows' logits [n_want, vocab]
  int32_t* tokens_out = nullptr;                 // ARGMAX (nullable): the arg-max; SAMPLE: the drawn tokens (sample.hip)
  const vstar_vqa_sampling* params = nullptr;    // SAMPLE; VERIFY (nullable: greedy): one record per wanted row
  const vstar_vqa_warpers* warpers = nullptr;    // SAMPLE, VERIFY (nullable): the §8.10 stages behind top-p, one record per wanted row
  LlmBeamArgs beam; LlmScoreArgs score; LlmVerifyArgs verify; LlmContrastArgs con;      // the kind's own host arrays
  bool has_lp = false;                           // ARGMAX, SAMPLE, VERIFY: the log-probability stage runs behind the tail
  LlmLogprobArgs lp;
};

struct LlmCachedCfg {
  int hidden = 0, heads = 0, mlp = 0, layers = 0, vocab = 0;
  float rms_eps = 1e-6f, rope_theta = 10000.f;
  int max_slots = 1, max_ctx = 1024, max_rows = 1024;
  int weight_bits = 0;      // 8: int8 weight-only decode of the block linears (fp16 build only);
                            // 4: int4 with one fp16 scale per group of 128 (fp16 build only)
  int kv_format = KV_FMT_F16;   // KV_FMT_MXFP8 / KV_FMT_MXFP8_EMU: block-scaled fp8 KV cache (fp16 build only)
  // Decode attention of a runner whose steps must not depend on their row count (the batched cue decode through decode_greedy):
  // split_rows > 0 sizes the split-KV workspace for that many rows instead of SPLIT_ROWS, attn_decide_rows > 0 makes every step take
  // the split / unsplit decision of a step of that many rows (kernels.hpp: cached_attention's decide_rows).
  int split_rows = 0, attn_decide_rows = 0;
};

// What the decode GEMV streams for one layer's four block linears (SkinnyWeights, kernels.hpp).  fp16 (cfg.weight_bits == 0):
// only the tile-major copies of q|k|v, gate|up and down, where built.  int8 / int4: the row-major q + scales
// of all four and the tile-major images the format's rules allow (LlmCached::build_quantised); null where there is none.
struct DecodeLayerW { SkinnyWeights qkv, o, gate_up, down; };

// The KV cache of a runner: K and V as [layers][slots][heads][ctx][128] cells in one format (KvLayer, kernels.hpp), layer i
// `layer_stride` cells behind layer 0 (KV_FMT_MXFP8: its scale bytes layer_stride / 32 bytes behind layer 0's).
struct KvCache {
  KvLayer l0;                  // layer 0's view
  int layers = 0;
  int64_t layer_stride = 0;
  int64_t bytes = 0;           // K + V storage, scale bytes included
  int alloc(EngineBase* e, int fmt, int layers_, int slots, int heads, int ctx);
  KvLayer layer(int i) const {
    KvLayer l = l0;
    const int64_t off = (int64_t)i * layer_stride;
    if (l0.fmt == KV_FMT_MXFP8) { l.k = (uint8_t*)l0.k + off; l.v = (uint8_t*)l0.v + off; l.ks = l0.ks + off / 32; l.vs = l0.vs + off / 32; }
    else { l.k = (lp_t*)l0.k + off; l.v = (lp_t*)l0.v + off; }
    return l;
  }
  // the decoded K then V of one slot of one layer, [2][heads][ctx][128] floats, cut at cap; waits for `s` first.  Returns the
  // count, or -1 after a HIP failure.
  int64_t read(int layer_i, int slot, float* out, int64_t cap, hipStream_t s) const;
};

inline int KvCache::alloc(EngineBase* e, int fmt, int layers_, int slots, int heads, int ctx) {
  if (fmt != KV_FMT_F16 && fmt != KV_FMT_MXFP8 && fmt != KV_FMT_MXFP8_EMU) {
    e->set_error("kv_cache_format must be 0 (fp16), 1 (MX fp8) or 2 (MX fp8 emulated in fp16)");
    return VSTAR_ERR_INVALID;
  }
#ifndef VSTAR_LP_F16
  if (fmt != KV_FMT_F16) { e->set_error("kv_cache_format: the block-scaled fp8 KV cache needs the fp16 engine"); return VSTAR_ERR_INVALID; }
#endif
  l0 = KvLayer{};
  l0.fmt = fmt; l0.H = heads; l0.ctx = ctx;
  l0.slot_stride = (int64_t)heads * ctx * 128;
  layers = layers_;
  layer_stride = l0.slot_stride * slots;
  const size_t n = (size_t)layer_stride * layers;
  if (fmt == KV_FMT_MXFP8) {
    uint8_t *k = nullptr, *v = nullptr;
    RC(e->dalloc(&k, n));
    RC(e->dalloc(&v, n));
    RC(e->dalloc(&l0.ks, n / 32));
    RC(e->dalloc(&l0.vs, n / 32));
    l0.k = k; l0.v = v;
    bytes = (int64_t)(2 * (n + n / 32));
  } else {
    lp_t *k = nullptr, *v = nullptr;
    RC(e->dalloc(&k, n));
    RC(e->dalloc(&v, n));
    l0.k = k; l0.v = v;
    bytes = (int64_t)n * 2 * 2;
  }
  return 0;
}

inline int64_t KvCache::read(int layer_i, int slot, float* out, int64_t cap, hipStream_t s) const {
  const int64_t per = l0.slot_stride;                      // cells of one slot of K (or V)
  const int64_t cnt = std::min<int64_t>(2 * per, cap);
  if (hipStreamSynchronize(s) != hipSuccess) return -1;
  const KvLayer l = layer(layer_i);
  const int64_t off = (int64_t)slot * per;
  for (int which = 0; which < 2; ++which) {
    const int64_t lo = which * per, m = std::min(per, cnt - lo);
    if (m <= 0) break;
    if (l.fmt == KV_FMT_MXFP8) {
      std::vector<uint8_t> codes((size_t)per), sc((size_t)per / 32);
      if (hipMemcpy(codes.data(), (const uint8_t*)(which ? l.v : l.k) + off, codes.size(), hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(sc.data(), (which ? l.vs : l.ks) + off / 32, sc.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
      for (int64_t i = 0; i < m; ++i) {                    // OCP e4m3: 1-4-3, bias 7, subnormals, 0x7f / 0xff = NaN
        const uint8_t c = codes[(size_t)i];
        const int ex = (c >> 3) & 15, mant = c & 7;
        float v = ex == 15 && mant == 7 ? NAN : (ex ? ldexpf((float)(8 + mant), ex - 10) : ldexpf((float)mant, -9));
        v = ldexpf(v, (int)sc[(size_t)(i >> 5)] - 127);
        out[lo + i] = (c & 0x80) ? -v : v;
      }
    } else {
      std::vector<lp_t> tmp((size_t)m);
      if (hipMemcpy(tmp.data(), (const lp_t*)(which ? l.v : l.k) + off, (size_t)m * 2, hipMemcpyDeviceToHost) != hipSuccess) return -1;
      for (int64_t i = 0; i < m; ++i) out[lo + i] = lp2f(tmp[(size_t)i]);
    }
  }
  return cnt;
}

struct LlmCached {
  EngineBase* e = nullptr;
  LlmCachedCfg cfg;
  bool ready = false;
  // weights (not owned)
  const lp_t* embed = nullptr;
  const std::vector<LlmBlock>* blocks = nullptr;
  const lp_t* final_norm = nullptr;
  const Lin* lm_head = nullptr;
  // rows < 0 of `src` index this table (device, [n_feat_rows, hidden]); set by the owner before forward()
  const lp_t* feats = nullptr;
  int64_t n_feat_rows = 0;
  // owned
  lp_t* rope = nullptr;                          // [max_ctx, 128] cos | sin
  KvCache kv;
  lp_t *lx = nullptr, *lh = nullptr, *lqkv = nullptr, *latt = nullptr, *lact = nullptr;
  lp_t *wsel = nullptr, *wnorm = nullptr, *logits = nullptr;
  int32_t *d_src = nullptr, *d_row_pos = nullptr, *d_row_slot = nullptr, *d_row_seq = nullptr, *d_want = nullptr, *d_argmax = nullptr;
  // the per-sequence metadata [3][seq_cap()] = own slot | prefix slot | past length, uploaded as one block, and the row view over it
  // and the three row arrays above (anc null: a call that attends through the ancestry table sets it in its copy)
  int seq_cap() const { return cfg.max_slots * 4; }
  int32_t* d_seq = nullptr;
  // d_seq and its host images are [3][seq_cap()]: k = 0 own slot, 1 prefix slot, 2 past length
  size_t seq_index(int k, int i) const { return (size_t)k * seq_cap() + i; }
  int32_t* seq_array(int k) const { return d_seq + seq_index(k, 0); }
  KvRows kv_rows;
  void seq_set(std::vector<int32_t>& image, int i, int slot, int prefix, int past) const {
    image[seq_index(0, i)] = slot; image[seq_index(1, i)] = prefix; image[seq_index(2, i)] = past;
  }
  vstar_vqa_sampling* d_sparams = nullptr;      // [max_want] per-row sampling records of the SAMPLE and sampled VERIFY tails
  vstar_vqa_warpers* d_swarp = nullptr;         // [max_want] their §8.10 records: allocated by the first call that carries them
  int max_want = 256;                            // wanted rows of one lm_head call (the scoring tail chunks by it, up to max_rows)
  int32_t *d_starget = nullptr, *d_srank = nullptr;   // [max_rows] the scoring tail's targets / ranks
  float* d_nll = nullptr;                        // [max_rows]
  int32_t *d_vdraft = nullptr, *d_vflag = nullptr, *d_vtok = nullptr, *d_vacc = nullptr;   // [max_want] the verify tail's drafts / flags / outputs
  // ---- logits edits: allocated by the first forward() that carries edits, never by an engine that sees none ----
  int32_t *d_eoff = nullptr, *d_etok = nullptr;  // [3 max_want + 1] offsets, [edit_capacity()] ids
  float* d_epen = nullptr;                       // [max_want]
  int64_t edit_capacity() const { return (int64_t)max_want * (cfg.max_ctx + 2048); }     // ids of one call, the three lists of all rows together
  // ---- log-probabilities: allocated by the first forward() that asks for them, never by an engine that does not ----
  float *d_lp = nullptr, *d_lp_top = nullptr;    // [max_want], [max_want, 32] (row stride: the call's n_top)
  int32_t *d_lp_rank = nullptr, *d_lp_tok = nullptr;
  // ---- guidance: allocated by the first forward() that carries guidance, never by an engine that sees none ----
  // one device block [4][max_want] = cond row | neg row | scale | log_beta of the call's pairs, and its host image (guide_check fills it)
  int32_t* d_guide = nullptr;
  std::vector<int32_t> g_host;
  int g_pairs = 0;
  // ---- contrastive search: allocated by the first forward() with the contrast tail, never by an engine without one ----
  // The hidden history [max_slots][max_ctx][hidden] and its fp32 reciprocal norms [max_slots][max_ctx]; hist_len[slot] (host) = the
  // rows of the slot's history that describe the slot's K/V rows.  Once the history exists every other forward() (and whatever else
  // rewrites K/V rows of a slot) lowers hist_len to the first position it writes: stale history can never be read.
  lp_t* c_hist = nullptr;
  float* c_hist_rn = nullptr;
  std::vector<int32_t> hist_len;
  lp_t* c_cand = nullptr;                        // [max_want, hidden] the last step's candidate rows
  float *c_cand_rn = nullptr, *c_prob = nullptr, *c_pen = nullptr, *c_nprob = nullptr;      // [max_want] x 3, [max_want, 32]
  int32_t *c_sel = nullptr, *c_ntok = nullptr;   // [max_want], [max_want, 32]
  // the call's metadata, one device block and its host image: int64 dst[max_rows] (fill: history / candidate row of physical row r,
  // -1: padding) | int64 hbase[max_want] | int32 goff[max_want + 1] | hlen | owner | pos | rowslot [max_want] each
  char* c_meta = nullptr;
  std::vector<char> c_meta_host;
  int c_cand_rows = 0, c_max_group = 0, c_max_len = 0, c_fill_rows = 0;
  size_t c_meta_bytes() const { return ((size_t)cfg.max_rows + max_want) * 8 + ((size_t)5 * max_want + 1) * 4; }
  template <typename T> T* c_meta_at(char* base, int which) const {      // which: 0 dst, 1 hbase, 2 goff, 3 hlen, 4 owner, 5 pos, 6 rowslot
    const size_t W = (size_t)max_want, o8 = ((size_t)cfg.max_rows + W) * 8;
    const size_t off[7] = {0, (size_t)cfg.max_rows * 8, o8, o8 + (W + 1) * 4, o8 + (2 * W + 1) * 4, o8 + (3 * W + 1) * 4, o8 + (4 * W + 1) * 4};
    return (T*)(base + off[which]);
  }
  int contrast_alloc();
  int contrast_check(const LlmRows& r, const LlmContrastArgs& a);
  void hist_lower(int slot, int pos) { if (c_hist && hist_len[(size_t)slot] > pos) hist_len[(size_t)slot] = pos; }
  static constexpr int SPLIT_ROWS = 4;           // decode steps of up to this many sequences take the split-KV attention
  int split_rows() const { return cfg.split_rows > 0 ? cfg.split_rows : SPLIT_ROWS; }      // rows the workspace holds
  char* split_ws = nullptr;
  // ---- beam search ----
  // KV ancestry table [max_slots, max_ctx]: position p of the sequence in slot s lives in slot d_anc[s * max_ctx + p].  A slot is
  // "ancestral" (anc_flag) once kv_reorder has written its entries; its continued sequences then attend through the table (the
  // ANC attention kernels).  A fresh sequence (past_len 0) in the slot resets it to identity, and so does a fork into it (prefix
  // another slot) — unless the same call runs ANC, where the fork's entries are written as [0, past) -> prefix instead.  Forking
  // FROM an ancestral slot is an error.
  int32_t *d_anc = nullptr, *d_anc_tmp = nullptr, *d_reo = nullptr;
  std::vector<char> anc_flag;
  float *d_bscore = nullptr, *d_cand_s = nullptr;
  int32_t *d_goff = nullptr, *d_cand_t = nullptr, *d_cand_r = nullptr;
  char* beam_ws = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double last_ms = 0;
  // ---- greedy decode of n sequences, rows 0 .. n - 1, as one replayed hipGraph per n (decode_greedy) ----
  // A decode step is ~165 launches of 10-55 us (5 per layer); their arguments never change from token to token — token ids,
  // positions and past lengths live in DEVICE arrays, and so does what differs per call (eos id, per-row caps) — so the step of n
  // rows is captured once and replayed: a graph depends on n alone.  A last kernel of the step feeds every unfinished row's arg-max
  // back as its next input, advances its position and logs the tokens to coherent host memory, which the host polls with steps
  // queued ahead instead of synchronising the stream.  A runner decodes up to dec_rows_max() sequences at once (a one-slot runner: one).
  static constexpr int DEC_BATCH_MAX = 16;
  int dec_rows_max() const { return std::min(DEC_BATCH_MAX, cfg.max_slots); }
  hipGraphExec_t dec_graph[DEC_BATCH_MAX + 1] = {};
  int dec_attn_path = -1;                        // cached_attention path of the step the graphs hold / the last step launched by hand
  // device: [0] = eos id, [1 + r] = cap of row r (tokens, the prefill's included), [17 + r] = tokens row r has emitted,
  // [33 + r] = row r finished
  int32_t* d_dec_ctl = nullptr;
  int32_t* h_dec_log = nullptr;                  // coherent HOST memory: [0] = steps done, [1] = unfinished rows, [2 + step * n + r] = tokens
  int dec_log_steps = 0;                         // steps the log holds (of dec_rows_max() rows each)
  // ---- the decode GEMV's weight descriptors: empty (row-major fp16 weights only), or one record per layer ----
  // Tile-major copies of the big decode weights (round 5; SKINNY_W_F16): the weight-streaming GEMV gives a workgroup 16 (gate|up: 32)
  // ROWS of the row-major matrix, i.e. 16 - 32 sequential streams 2 K bytes apart and 4096 - 22016 of them over the chip; laid out
  // tile-major the same bytes stream at 6.5 - 7.0 TB/s instead of 5.4 - 6.5 (profiles/r05_stream_layout_probe.txt).  HBM has the room
  // for a second copy (q|k|v, gate|up, down: 11.8 GB at 7B); built when the runner is initialised, VSTAR_DECODE_TILED=0 keeps the
  // row-major streams (A/B, tests: bit-identical).
  // Weight-only decode (cfg.weight_bits == 8 / 4): per layer the int8 / int4 copies of q|k|v, o, gate|up and
  // down; the fp16 masters then hold the DEQUANTISED weights (prefill and every call of more than 64 rows run the same quantised
  // model on the tile kernels) and the fp16 tile-major copies are not built.
  std::vector<DecodeLayerW> dec_w;
  const DecodeLayerW& dec(int i) const { static const DecodeLayerW none{}; return dec_w.empty() ? none : dec_w[(size_t)i]; }
  bool tiled_fallback = false;      // the fp16 tile-major copies were wanted but did not fit / pack: decode runs on the row-major weights
  int build_quantised(int fmt);

  void set_error(const std::string& m) { e->set_error(m); }
  int init(EngineBase* owner, const LlmCachedCfg& c, const lp_t* embed_, const std::vector<LlmBlock>* blocks_,
           const lp_t* final_norm_, const Lin* lm_head_);
  void release() {
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
    for (hipGraphExec_t& g : dec_graph) { if (g) hipGraphExecDestroy(g); g = nullptr; }
    if (h_dec_log) hipHostFree(h_dec_log);
    h_dec_log = nullptr;
  }
  int decode_step_body(int n, int keys_bound);
  int decode_state(int n, const int32_t* first, const int32_t* past, const int32_t* caps, int eos_id);
  int decode_greedy(int n, const int32_t* first, const int32_t* past, const int32_t* caps, int eos_id, int32_t* out_ids, int64_t out_ld,
                    int32_t* n_out);
  // the fp16 tile-major decode weights of another runner over the same blocks (set before init: this runner then builds none)
  const std::vector<DecodeLayerW>* borrow_dec_w = nullptr;
  int lin_auto(const lp_t* A, int64_t lda, const Lin& L, void* C, int64_t ldc, int M, int epi = VSTAR_EPI_NONE,
               const lp_t* res = nullptr, int64_t ldr = 0, const SkinnyWeights* dw = nullptr);
  int lin_norm(const lp_t* x, const lp_t* norm_w, lp_t* scratch, const Lin& L, void* C, int64_t ldc, int M, int epi,
               const SkinnyWeights* dw = nullptr);
  int lin_skinny(GemmParams& p, int epi, const SkinnyWeights* dw);
  int llm_layers_prefill(int nseq, int S);
  int llm_layers_cached(int R, int max_keys, bool single_rows, const int32_t* anc = nullptr);
  // ---- forward(): the head and the tail's stages (one switch over the six tails each) ----
  struct TailCopy { void* dev = nullptr; const void* in = nullptr; void* out = nullptr; size_t bytes = 0; };
  size_t vpad() const { return (size_t)(cfg.vocab + 255) / 256 * 256; }      // row stride of the logits buffer
  int forward(const LlmRows& rw, const LlmTail& tail, const LlmEdits* edits = nullptr, const LlmGuide* guide = nullptr);
  int head(int w0, int m);
  int tail_check(const LlmRows& r, const LlmTail& t);
  int guide_check(const LlmRows& r, const LlmTail& t, const LlmGuide& g);
  int edits_check(const LlmRows& r, const LlmTail& t, const LlmEdits& ed);
  int logprobs_check(const LlmRows& r, const LlmTail& t);
  std::array<TailCopy, 6> tail_copies(const LlmTail& t, int n_want);
  void contrast_meta(const LlmRows& r, const LlmTail& t, const std::vector<int32_t>& h_pos, const std::vector<int32_t>& h_slot, int rows);
  int tail_launch(const LlmTail& t, int w0, int m);
  int kv_reorder(int n, const int32_t* dst, const int32_t* src, int lo, int hi);
  int kv_copy(int dst, int src, int lo, int hi);
};

inline int LlmCached::init(EngineBase* owner, const LlmCachedCfg& c, const lp_t* embed_, const std::vector<LlmBlock>* blocks_,
                           const lp_t* final_norm_, const Lin* lm_head_) {
  e = owner; cfg = c; embed = embed_; blocks = blocks_; final_norm = final_norm_; lm_head = lm_head_;
  const int H = c.hidden;
  if (H != c.heads * 128) { set_error("LLaMA head dim must be 128"); return VSTAR_ERR_INVALID; }
  {  // HF LlamaRotaryEmbedding: fp32 cos/sin cast to the activation dtype before use
    std::vector<lp_t> tab((size_t)c.max_ctx * 128);
    for (int s = 0; s < c.max_ctx; ++s)
      for (int i = 0; i < 64; ++i) {
        const float inv = 1.0f / powf(c.rope_theta, (float)(2 * i) / 128.0f);
        const float f = (float)s * inv;
        tab[(size_t)s * 128 + i] = f2lp(cosf(f));
        tab[(size_t)s * 128 + 64 + i] = f2lp(sinf(f));
      }
    RC(e->dalloc(&rope, tab.size()));
    if (hipMemcpy(rope, tab.data(), tab.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { set_error("rope table upload failed"); return VSTAR_ERR_HIP; }
  }
  RC(kv.alloc(e, c.kv_format, c.layers, c.max_slots, c.heads, c.max_ctx));
  const size_t R = (size_t)c.max_rows;
  RC(e->dalloc(&lx, R * H));
  RC(e->dalloc(&lh, R * H));
  RC(e->dalloc(&lqkv, R * 3 * H));
  RC(e->dalloc(&latt, R * H));
  RC(e->dalloc(&lact, R * c.mlp));
  RC(e->dalloc(&wsel, (size_t)max_want * H));
  RC(e->dalloc(&wnorm, (size_t)max_want * H));
  RC(e->dalloc(&logits, (size_t)max_want * vpad()));
  RC(e->dalloc(&d_src, R));
  RC(e->dalloc(&d_row_pos, R));
  RC(e->dalloc(&d_row_slot, R));
  RC(e->dalloc(&d_row_seq, R));
  RC(e->dalloc(&d_seq, (size_t)3 * seq_cap()));
  kv_rows = KvRows{d_row_seq, d_row_pos, d_row_slot, seq_array(0), seq_array(1), seq_array(2), nullptr};
  RC(e->dalloc(&d_want, std::max(R, (size_t)max_want)));     // (the scoring tail wants up to max_rows rows)
  RC(e->dalloc(&d_starget, R));
  RC(e->dalloc(&d_srank, R));
  RC(e->dalloc(&d_nll, R));
  RC(e->dalloc(&d_argmax, (size_t)max_want));
  RC(e->dalloc(&d_sparams, (size_t)max_want));
  RC(e->dalloc(&d_vdraft, (size_t)max_want));
  RC(e->dalloc(&d_vflag, (size_t)max_want));
  RC(e->dalloc(&d_vtok, (size_t)max_want));
  RC(e->dalloc(&d_vacc, (size_t)max_want));
  {  // split-KV decode attention (decode.hip): scores / partials / tickets for steps of up to SPLIT_ROWS sequences, zeroed once
    const size_t wb = cached_attention_split_ws_bytes(split_rows(), c.heads, c.max_ctx);
    RC(e->dalloc(&split_ws, wb));
    if (hipMemset(split_ws, 0, wb) != hipSuccess) { set_error("split-KV workspace memset failed"); return VSTAR_ERR_HIP; }
  }
  {  // beam search: the ancestry table (identity), its reorder scratch, the select tail's buffers
    const size_t na = (size_t)c.max_slots * c.max_ctx;
    RC(e->dalloc(&d_anc, na));
    RC(e->dalloc(&d_anc_tmp, na));
    RC(e->dalloc(&d_reo, (size_t)2 * c.max_slots));
    std::vector<int32_t> ident(na);
    for (size_t i = 0; i < na; ++i) ident[i] = (int32_t)(i / c.max_ctx);
    if (hipMemcpy(d_anc, ident.data(), na * 4, hipMemcpyHostToDevice) != hipSuccess) { set_error("ancestry table upload failed"); return VSTAR_ERR_HIP; }
    anc_flag.assign((size_t)c.max_slots, 0);
    RC(e->dalloc(&d_bscore, (size_t)max_want));
    RC(e->dalloc(&d_goff, (size_t)max_want + 1));
    RC(e->dalloc(&d_cand_s, (size_t)max_want * VSTAR_BEAM_MAX_CAND));
    RC(e->dalloc(&d_cand_t, (size_t)max_want * VSTAR_BEAM_MAX_CAND));
    RC(e->dalloc(&d_cand_r, (size_t)max_want * VSTAR_BEAM_MAX_CAND));
    RC(e->dalloc(&beam_ws, vstar_beam_ws_bytes(max_want, VSTAR_BEAM_MAX_CAND)));
  }
  if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) { set_error("hipEventCreate failed"); return VSTAR_ERR_HIP; }
  {  // tile-major copies of q|k|v, gate|up and down for the decode GEMV (o_proj's 33 MB live in the Infinity Cache either way).
     // OPTIONAL: the row-major weights serve the same GEMV (dw.tiled == nullptr), so a failed allocation or pack — ~11.8 GB more at
     // 7B — drops the copies, clears the error and continues row-major instead of failing generate().
    const char* env = getenv("VSTAR_DECODE_TILED");
    const bool on = !(env && atoi(env) == 0) && c.weight_bits == 0;      // (the quantised modes build their own images: build_quantised)
    dec_w.clear();                                            // a retried init starts from an empty list: dec_w[i] is layer i or nothing
    std::vector<void*> mine;                                  // this block's allocations, freed together if any step fails
    bool ok = true;
    auto tile = [&](const Lin& L, int nt, SkinnyWeights& out) {
      const int rows = (L.N + 16 * nt - 1) / (16 * nt) * (16 * nt);     // (the packed W is padded to 256 rows)
      if (L.N % (16 * nt) || L.K % 64) return;
      void* t = nullptr;
      if (hipMalloc(&t, (size_t)rows * L.K * sizeof(lp_t)) != hipSuccess) { (void)hipGetLastError(); ok = false; return; }
      mine.push_back(t);
      if (skinny_pack_tiles(L.W, (lp_t*)t, rows, L.K, nt, e->stream) != hipSuccess) { (void)hipGetLastError(); ok = false; return; }
      out.tiled = t;
    };
    if (borrow_dec_w) {
      dec_w = *borrow_dec_w;                                  // (empty when the lender runs row-major: so does this runner)
    } else if (on && c.hidden >= 512) {
      size_t need = 0, free_b = 0, total_b = 0;
      for (int i = 0; i < c.layers; ++i) {
        const LlmBlock& b = (*blocks)[i];
        need += ((size_t)b.qkv.N * b.qkv.K + (size_t)b.gate_up.N * b.gate_up.K + (size_t)b.down.N * b.down.K) * sizeof(lp_t);
      }
      // keep 1 GiB of headroom for the caller's later allocations (KV growth happens above; this is the last big block of init)
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)1 << 30)) { (void)hipGetLastError(); ok = false; }
      dec_w.assign((size_t)c.layers, DecodeLayerW{});
      for (int i = 0; ok && i < c.layers; ++i) {
        const LlmBlock& b = (*blocks)[i];
        tile(b.qkv, 1, dec_w[i].qkv);
        if (ok) tile(b.gate_up, 2, dec_w[i].gate_up);
        if (ok) tile(b.down, 1, dec_w[i].down);
      }
      if (hipStreamSynchronize(e->stream) != hipSuccess) { (void)hipGetLastError(); ok = false; }
      if (ok) {
        for (void* q : mine) e->allocs.push_back(q);            // owned by the engine from here on
      } else {
        for (void* q : mine) hipFree(q);
        dec_w.clear();                                          // row-major decode
        tiled_fallback = true;
      }
    }
  }
  if (c.weight_bits == 8 || c.weight_bits == 4) RC(build_quantised(c.weight_bits));
  else if (c.weight_bits != 0) { set_error("decode_weight_bits must be 0 or 8"); return VSTAR_ERR_INVALID; }
  ready = true;
  return 0;
}

#ifdef VSTAR_LP_F16
// What differs between the quantised decode formats; everything else of build_quantised is shared.
struct DecodeFmt {
  int fmt;                     // SkinnyWeights::fmt = cfg.weight_bits
  const char* what;            // message prefix
  int k_mult;                  // K of every block linear must be a multiple of it
  size_t (*q_bytes)(int K);    // bytes of q / of the scales per row of the packed (256-padded) matrix
  size_t (*scale_bytes)(int K);
  hipError_t (*quantise)(const lp_t* W, int rows, int K, void* q, void* scale, lp_t* What, hipStream_t s);
  size_t (*tile_bytes)(int N, int K, int nt);
  hipError_t (*pack)(const void* q, const void* scale, void* Wt, int N, int K, int nt, hipStream_t s);
  // Which linears get a tile-major image (VSTAR_DECODE_TILED=0: none; always whole 16 NT-row tiles only).  The two formats differ on
  // purpose: the int8 image feeds the LDS-ring kernel, which runs from K = 512 on and gains nothing for o_proj (its 33 MB at 7B live
  // in the Infinity Cache either way) — the fp16 path's rules; the int4 image is read by the register kernel, which serves every
  // width and every linear, and replaces four 16-byte row loads per lane by one coalesced load wherever it exists.
  bool tiles_need_hidden_512;
  bool tiles_for_o;
};
inline const DecodeFmt* decode_fmt(int fmt) {
  static const DecodeFmt table[] = {
      {SKINNY_W_INT8, "int8 decode weights", 64,
       [](int K) { return (size_t)K; }, [](int) { return sizeof(float); },
       [](const lp_t* W, int rows, int K, void* q, void* sc, lp_t* What, hipStream_t s) { return quantize_rows_w8(W, rows, K, (int8_t*)q, (float*)sc, What, s); },
       [](int N, int K, int) { return (size_t)N * K; },
       [](const void* q, const void*, void* Wt, int N, int K, int nt, hipStream_t s) { return skinny_pack_tiles_w8((const int8_t*)q, (int8_t*)Wt, N, K, nt, s); },
       true, false},
      {SKINNY_W_INT4G128, "int4 decode weights (decode_weight_format = 1)", 128,
       [](int K) { return (size_t)(K / 8) * sizeof(uint32_t); }, [](int K) { return (size_t)(K / 128) * sizeof(lp_t); },
       [](const lp_t* W, int rows, int K, void* q, void* sc, lp_t* What, hipStream_t s) { return quantize_groups_w4(W, rows, K, (uint32_t*)q, (lp_t*)sc, What, s); },
       [](int N, int K, int nt) { return skinny_tiles_w4_bytes(N, K, nt); },
       [](const void* q, const void* sc, void* Wt, int N, int K, int nt, hipStream_t s) { return skinny_pack_tiles_w4((const uint32_t*)q, (const lp_t*)sc, Wt, N, K, nt, s); },
       false, true},
  };
  for (const DecodeFmt& f : table)
    if (f.fmt == fmt) return &f;
  return nullptr;
}
#endif

// The weight-only decode modes, once, on the device, from the packed fp16 weights: every quantised
// buffer is allocated and filled FIRST (a failed allocation or launch is an error with the fp16 masters untouched: there is no fp16
// fallback behind the caller's back), then the masters are overwritten with the dequantised weights.  A launch or the synchronise
// failing DURING that overwrite leaves some masters dequantised and others not: the error is returned, `ready` stays false, every
// forward of the engine then fails with VSTAR_ERR_STATE, and the weights have to be loaded again.  Scales belong to rows of the
// packed matrices, whose gate|up interleave and q|k|v concatenation only permute rows of the original ones.
inline int LlmCached::build_quantised(int fmt) {
#ifdef VSTAR_LP_F16
  const LlmCachedCfg& c = cfg;
  const DecodeFmt& f = *decode_fmt(fmt);
  const std::string what = f.what;
  const char* env = getenv("VSTAR_DECODE_TILED");
  const bool tiled_on = !(env && atoi(env) == 0) && (!f.tiles_need_hidden_512 || c.hidden >= 512);
  std::vector<void*> mine;
  auto fail = [&](const std::string& m, int rc) {
    for (void* q : mine) hipFree(q);
    (void)hipGetLastError();
    dec_w.clear();
    set_error(m);
    return rc;
  };
  auto take = [&](size_t bytes) -> void* {
    void* t = nullptr;
    if (hipMalloc(&t, bytes) != hipSuccess) return nullptr;
    mine.push_back(t);
    return t;
  };
  auto quant = [&](const Lin& L, int nt, bool want_tiles, SkinnyWeights* out) -> int {
    const int npad = (L.N + 255) / 256 * 256;
    if (L.K % f.k_mult) return VSTAR_ERR_INVALID;
    void* q = take((size_t)npad * f.q_bytes(L.K));
    void* sc = take((size_t)npad * f.scale_bytes(L.K));
    if (!q || !sc) return VSTAR_ERR_NOMEM;
    *out = SkinnyWeights{f.fmt, q, sc, nullptr};
    if (f.quantise(L.W, npad, L.K, q, sc, nullptr, e->stream) != hipSuccess) return VSTAR_ERR_HIP;
    if (want_tiles && L.N % (16 * nt) == 0) {
      void* t = take(f.tile_bytes(L.N, L.K, nt));
      if (!t) return VSTAR_ERR_NOMEM;
      out->tiled = t;
      if (f.pack(q, sc, t, L.N, L.K, nt, e->stream) != hipSuccess) return VSTAR_ERR_HIP;
    }
    return 0;
  };
  dec_w.assign((size_t)c.layers, DecodeLayerW{});
  for (int i = 0; i < c.layers; ++i) {
    const LlmBlock& b = (*blocks)[i];
    int rc = quant(b.qkv, 1, tiled_on, &dec_w[i].qkv);
    if (!rc) rc = quant(b.o, 1, tiled_on && f.tiles_for_o, &dec_w[i].o);
    if (!rc) rc = quant(b.gate_up, 2, tiled_on, &dec_w[i].gate_up);
    if (!rc) rc = quant(b.down, 1, tiled_on, &dec_w[i].down);
    if (rc) return fail(what + ": allocation or quantiser launch failed (layer " + std::to_string(i) + ")", rc);
  }
  if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(what + ": quantiser failed", VSTAR_ERR_HIP);
  // every quantised buffer exists: now the masters become the dequantised weights (same q, same scales: deterministic)
  for (int i = 0; i < c.layers; ++i) {
    const LlmBlock& b = (*blocks)[i];
    const Lin* ls[4] = {&b.qkv, &b.o, &b.gate_up, &b.down};
    const SkinnyWeights* qs[4] = {&dec_w[i].qkv, &dec_w[i].o, &dec_w[i].gate_up, &dec_w[i].down};
    for (int j = 0; j < 4; ++j) {
      const int npad = (ls[j]->N + 255) / 256 * 256;
      if (f.quantise(ls[j]->W, npad, ls[j]->K, (void*)qs[j]->q, (void*)qs[j]->scale, ls[j]->W, e->stream) != hipSuccess)
        return fail(what + ": dequantising the fp16 masters failed", VSTAR_ERR_HIP);
    }
  }
  if (hipStreamSynchronize(e->stream) != hipSuccess) return fail(what + ": dequantising the fp16 masters failed", VSTAR_ERR_HIP);
  for (void* q : mine) e->allocs.push_back(q);
  return 0;
#else
  set_error(fmt == 8 ? "decode_weight_bits = 8 needs the fp16 engine" : "decode_weight_format = 1 needs the fp16 engine");
  return VSTAR_ERR_INVALID;
#endif
}

#define LCHK(expr)                                                                           \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                          \
      return VSTAR_ERR_HIP;                                                                  \
    }                                                                                        \
  } while (0)

// the weight-streaming GEMV on the weights `dw` describes (null: L's row-major fp16 / bf16 weights)
inline int LlmCached::lin_skinny(GemmParams& p, int epi, const SkinnyWeights* dw) {
  if (dw) p.dw = *dw;
  const hipError_t he = gemm_skinny_lp(p, epi, false, e->stream);
  if (he != hipSuccess) { set_error(std::string("skinny gemm launch: ") + hipGetErrorString(he)); return VSTAR_ERR_HIP; }
  return 0;
}

// GEMM dispatch for the language model: weight-streaming kernel for decode-sized M, MFMA tile kernels otherwise
inline int LlmCached::lin_auto(const lp_t* A, int64_t lda, const Lin& L, void* C, int64_t ldc, int M, int epi, const lp_t* res,
                               int64_t ldr, const SkinnyWeights* dw) {
  GemmParams p{};
  p.A = A; p.lda = lda; p.W = L.W; p.bias = L.b; p.res = res; p.ldr = ldr; p.C = C; p.ldc = ldc; p.M = M; p.N = L.N; p.K = L.K;
  if (gemm_skinny_eligible(p)) return lin_skinny(p, epi, dw);
  return e->gemm(p, epi, false);
}

// RMSNorm + Linear: for decode-sized M the norm is fused into the weight-streaming GEMM's operand load (bit-identical to
// the two-kernel form), otherwise norm kernel into `scratch`, then the GEMM
inline int LlmCached::lin_norm(const lp_t* x, const lp_t* norm_w, lp_t* scratch, const Lin& L, void* C, int64_t ldc, int M,
                               int epi, const SkinnyWeights* dw) {
  const int H = cfg.hidden;
  GemmParams p{};
  p.A = x; p.lda = H; p.W = L.W; p.bias = L.b; p.C = C; p.ldc = ldc; p.M = M; p.N = L.N; p.K = L.K;
  if (M <= 16 && L.K == H && gemm_skinny_eligible(p)) {
    p.norm_w = norm_w; p.norm_eps = cfg.rms_eps;
    return lin_skinny(p, epi, dw);
  }
  LCHK(rmsnorm_lp(x, norm_w, scratch, M, H, cfg.rms_eps, nullptr, e->stream));
  return lin_auto(scratch, H, L, C, ldc, M, epi, nullptr, 0, dw);
}

inline int LlmCached::llm_layers_prefill(int nseq, int S) {
  const LlmCachedCfg& c = cfg;
  const int H = c.hidden, rows = nseq * S;
  const float att_scale = 1.0f / sqrtf(128.0f);
  for (int i = 0; i < c.layers; ++i) {
    const LlmBlock& b = (*blocks)[i];
    LCHK(rmsnorm_lp(lx, b.in_norm, lh, rows, H, c.rms_eps, nullptr, e->stream));
    RC(e->lin(lh, H, b.qkv, lqkv, 3 * H, rows));
    LCHK(rope_kv_append(lqkv, rope, kv.layer(i), kv_rows, rows, e->stream));
    LCHK(attn_forward(lqkv, latt, nseq, S, c.heads, 128, 1, att_scale, e->stream));
    RC(e->lin(latt, H, b.o, lx, H, rows, VSTAR_EPI_NONE, lx, H));
    LCHK(rmsnorm_lp(lx, b.post_norm, lh, rows, H, c.rms_eps, nullptr, e->stream));
    RC(e->lin(lh, H, b.gate_up, lact, c.mlp, rows, VSTAR_EPI_SILU_MUL));
    RC(e->lin(lact, c.mlp, b.down, lx, H, rows, VSTAR_EPI_NONE, lx, H));
  }
  return 0;
}

inline int LlmCached::llm_layers_cached(int R, int max_keys, bool single_rows, const int32_t* anc) {
  const LlmCachedCfg& c = cfg;
  const int H = c.hidden;
  KvRows rw = kv_rows;
  rw.anc = anc;
  for (int i = 0; i < c.layers; ++i) {
    const LlmBlock& b = (*blocks)[i];
    const KvLayer kl = kv.layer(i);
    const DecodeLayerW& dw = dec(i);
    RC(lin_norm(lx, b.in_norm, lh, b.qkv, lqkv, 3 * H, R, VSTAR_EPI_NONE, &dw.qkv));
    // decode steps (one new row per sequence): RoPE + cache append happen inside the attention kernel
    if (!single_rows) LCHK(rope_kv_append(lqkv, rope, kl, rw, R, e->stream));
    LCHK(cached_attention(lqkv, kl, rw, single_rows ? rope : nullptr, latt, R, max_keys, e->stream, split_ws, split_rows(),
                          c.attn_decide_rows));
    RC(lin_auto(latt, H, b.o, lx, H, R, VSTAR_EPI_NONE, lx, H, &dw.o));
    RC(lin_norm(lx, b.post_norm, lh, b.gate_up, lact, c.mlp, R, VSTAR_EPI_SILU_MUL, &dw.gate_up));
    RC(lin_auto(lact, c.mlp, b.down, lx, H, R, VSTAR_EPI_NONE, lx, H, &dw.down));
  }
  return 0;
}

// model.norm + lm_head (llava_search_llama.py:92-93) on wanted rows [w0, w0 + m), m <= max_want, into rows [0, m) of the one
// [max_want, vpad] logits buffer; lm_head sees m rows (its row count selects the GEMM kernel)
inline int LlmCached::head(int w0, int m) {
  LCHK(gather_rows(lx, d_want + w0, wsel, m, cfg.hidden, e->stream));
  return lin_norm(wsel, final_norm, wnorm, *lm_head, logits, (int64_t)vpad(), m, VSTAR_EPI_NONE);
}

// ---- the six tails, one switch per stage: checks, host <-> device copies, launch ----
// (forward() validates the rows first, then the tail: of two simultaneous faults the row fault is the one reported)
inline int LlmCached::tail_check(const LlmRows& r, const LlmTail& t) {
  const int n_want = r.n_want, V = cfg.vocab;
  if (t.params && !vstar_sample_params_valid(t.params, n_want)) {
    e->set_error("sampling parameters: temperature must be > 0 and finite, top_k >= 0, top_p >= 0");
    return VSTAR_ERR_INVALID;
  }
  const char* m = nullptr;
  if (t.warpers) {             // SAMPLE, VERIFY; the device records are allocated here, by the first call that carries them
    if ((m = vstar_warpers_check(t.warpers, n_want))) { e->set_error(m); return VSTAR_ERR_INVALID; }
    if (!d_swarp) {
      const int rc = e->dalloc(&d_swarp, (size_t)max_want);
      if (rc) { (void)hipGetLastError(); d_swarp = nullptr; return rc; }
    }
  }
  switch (t.kind) {
    default: break;            // ARGMAX, SAMPLE: nothing of their own
    case LlmTail::BEAM:
      if (n_want < 1 || !t.beam.cand_s || !t.beam.cand_tok || !t.beam.cand_row) { e->set_error("forward_beam: no wanted rows / outputs"); return VSTAR_ERR_INVALID; }
      if ((m = vstar_beam_check(n_want, V, t.beam.scores, t.beam.n_groups, t.beam.goff, t.beam.n_cand))) { e->set_error(std::string("forward_beam: ") + m); return VSTAR_ERR_INVALID; }
      break;
    case LlmTail::SCORE:       // this tail chunks its wanted rows (CHUNKING RULE): its limit is max_rows, not max_want
      if (n_want < 1 || !t.score.targets || !t.score.nll) { e->set_error("forward_score: no wanted rows / targets / outputs"); return VSTAR_ERR_INVALID; }
      if (n_want > cfg.max_rows) { e->set_error("forward_score: more wanted rows than max_rows"); return VSTAR_ERR_INVALID; }
      if ((m = vstar_score_check(n_want, V, t.score.targets))) { e->set_error(std::string("forward_score: ") + m); return VSTAR_ERR_INVALID; }
      break;
    case LlmTail::VERIFY: {
      const LlmVerifyArgs& v = t.verify;
      if (n_want < 1 || !v.goff || !v.draft || !v.n_accept || !v.tokens) { e->set_error("forward_verify: no wanted rows / groups / drafts / outputs"); return VSTAR_ERR_INVALID; }
      if ((m = vstar_verify_check(n_want, V, v.n_groups, v.goff, v.draft))) { e->set_error(std::string("forward_verify: ") + m); return VSTAR_ERR_INVALID; }
      // a group is one sequence's rows in position order: the prefix rule compares row j's choice with the token fed as a LATER row
      for (int g = 0; g < v.n_groups; ++g) {
        int seq = 0;
        while (r.row_off[seq + 1] <= r.want[v.goff[g]]) ++seq;
        for (int j = v.goff[g]; j < v.goff[g + 1]; ++j)
          if (r.want[j] >= r.row_off[seq + 1] || (j > v.goff[g] && r.want[j] <= r.want[j - 1])) {
            e->set_error("forward_verify: the wanted rows of a group must be rows of one sequence in position order");
            return VSTAR_ERR_INVALID;
          }
      }
      break;
    }
    case LlmTail::CONTRAST: RC(contrast_check(r, t.con)); break;
  }
  return 0;
}

// The history and the scratch of the contrast tail, by the first call that carries it: two allocations, the second one's failure
// frees the first, so a failed allocation leaves nothing behind and the engine as it was.
inline int LlmCached::contrast_alloc() {
  if (c_hist) return 0;
  const size_t S = (size_t)cfg.max_slots * cfg.max_ctx, H = (size_t)cfg.hidden, W = (size_t)max_want;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t b_hist = up(S * H * 2), b_rn = up(S * 4);
  const size_t b_cand = up(W * H * 2), b_w4 = up(W * 4), b_top = up(W * VSTAR_CONTRAST_MAX_K * 4), b_meta = up(c_meta_bytes());
  char *hist = nullptr, *blk = nullptr;
  if (hipMalloc(&hist, b_hist + b_rn) != hipSuccess) { (void)hipGetLastError(); set_error("contrastive search: no memory for the hidden history (max_slots * max_ctx * (2 * hidden + 4) bytes)"); return VSTAR_ERR_NOMEM; }
  if (hipMalloc(&blk, b_cand + 4 * b_w4 + 2 * b_top + b_meta) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(hist);
    set_error("contrastive search: no memory for the candidate buffers");
    return VSTAR_ERR_NOMEM;
  }
  e->allocs.push_back(hist);
  e->allocs.push_back(blk);
  c_hist_rn = (float*)(hist + b_hist);
  char* q = blk;
  c_cand = (lp_t*)q; q += b_cand;
  c_cand_rn = (float*)q; q += b_w4;
  c_prob = (float*)q; q += b_w4;
  c_pen = (float*)q; q += b_w4;
  c_sel = (int32_t*)q; q += b_w4;
  c_ntok = (int32_t*)q; q += b_top;
  c_nprob = (float*)q; q += b_top;
  c_meta = q;
  c_meta_host.assign(c_meta_bytes(), 0);
  hist_len.assign((size_t)cfg.max_slots, 0);
  c_hist = (lp_t*)hist;                          // (last: c_hist != null means all of the above exists)
  return 0;
}

// The contrast tail's rules (include/vstar_vqa.h), before any device work; the messages name the field.
inline int LlmCached::contrast_check(const LlmRows& r, const LlmContrastArgs& a) {
  auto bad = [&](const std::string& m) { e->set_error(m); return VSTAR_ERR_INVALID; };
  const bool step = a.goff != nullptr;
  const char* fn = step ? "forward_contrast_step: " : "forward_contrast_begin: ";
  if (r.n_want < 1 || !a.next_tok || !a.next_prob) return bad(std::string(fn) + "no wanted rows / next_tok / next_prob");
  if (a.k < 2 || a.k > VSTAR_CONTRAST_MAX_K || a.k > cfg.vocab) return bad(std::string(fn) + (step ? "k_next" : "k") + " must be in [2, 32] and <= llm_vocab");
  if (step) {
    if (!a.sel) return bad(std::string(fn) + "no sel_out");
    if (r.n_want != r.nseq) return bad(std::string(fn) + "n_want: every sequence has exactly one row and all rows are wanted");
    for (int i = 0; i < r.nseq; ++i) {
      if (r.row_off[i + 1] - r.row_off[i] != 1) return bad(std::string(fn) + "row_off: every sequence has exactly one row");
      if (r.want[i] != i) return bad(std::string(fn) + "want: wanted row j must be row j");
    }
    if (const char* m = vstar_contrast_check(r.n_want, cfg.vocab, a.n_groups, a.goff, a.cand_prob, a.alpha, a.k)) return bad(std::string(fn) + m);
  }
  RC(contrast_alloc());
  std::vector<char> used((size_t)cfg.max_slots, 0);      // 1: some row's kv_slot, 2: an owner that no row writes (yet)
  for (int i = 0; i < r.nseq; ++i) {
    if (used[r.kv_slot[i]] == 1) return bad(std::string(fn) + "kv_slot: the slots of a call must be pairwise distinct");
    used[r.kv_slot[i]] = 1;
  }
  if (!step) {
    for (int i = 0; i < r.nseq; ++i) {
      if (r.prefix_slot[i] != r.kv_slot[i]) return bad(std::string(fn) + "prefix_slot must equal kv_slot");
      if (r.past_len[i] != 0 && r.past_len[i] != hist_len[r.kv_slot[i]])
        return bad(std::string(fn) + "past_len must be 0 (a fresh sequence) or the slot's history length " + std::to_string(hist_len[r.kv_slot[i]]));
      if (r.past_len[i] != 0 && anc_flag[r.kv_slot[i]]) return bad(std::string(fn) + "kv_slot: a beam-reordered slot has no history");
    }
    return 0;
  }
  for (int g = 0; g < a.n_groups; ++g) {
    const int own = r.prefix_slot[a.goff[g]], L = r.past_len[a.goff[g]];
    for (int j = a.goff[g]; j < a.goff[g + 1]; ++j) {
      if (r.prefix_slot[j] != own) return bad(std::string(fn) + "prefix_slot: the rows of a group share one owner slot");
      if (r.past_len[j] != L) return bad(std::string(fn) + "past_len: the rows of a group share one past_len");
    }
    if (L < 1 || L != hist_len[own])
      return bad(std::string(fn) + "past_len must equal the owner's history length " + std::to_string(hist_len[own]) +
                 " (a forward() that rewound the slot invalidated the history behind it; begin again)");
    if (anc_flag[own]) return bad(std::string(fn) + "prefix_slot: a beam-reordered slot has no history");
    bool mine = false;
    for (int j = a.goff[g]; j < a.goff[g + 1]; ++j) mine = mine || r.kv_slot[j] == own;
    if (!mine) {              // (an owner one of its own rows writes is covered by the distinct kv_slots)
      if (used[own]) return bad(std::string(fn) + "prefix_slot: an owner slot is another group's owner or candidate slot");
      used[own] = 2;
    }
  }
  return 0;
}

// The contrast tail's device metadata (c_meta_host; forward() uploads it with the row metadata), from the physical rows of the call.
inline void LlmCached::contrast_meta(const LlmRows& r, const LlmTail& t, const std::vector<int32_t>& h_pos, const std::vector<int32_t>& h_slot, int rows) {
  const LlmContrastArgs& a = t.con;
  char* hb = c_meta_host.data();
  int64_t* dst = c_meta_at<int64_t>(hb, 0);
  if (!a.goff) {
    for (int q = 0; q < rows; ++q) dst[q] = h_pos[q] >= 0 ? (int64_t)h_slot[q] * cfg.max_ctx + h_pos[q] : -1;
    return;
  }
  int64_t* hbase = c_meta_at<int64_t>(hb, 1);
  int32_t *goff = c_meta_at<int32_t>(hb, 2), *hlen = c_meta_at<int32_t>(hb, 3), *owner = c_meta_at<int32_t>(hb, 4), *pos = c_meta_at<int32_t>(hb, 5),
          *rowslot = c_meta_at<int32_t>(hb, 6);
  for (int j = 0; j < r.n_want; ++j) { dst[j] = j; rowslot[j] = r.kv_slot[j]; }
  c_max_group = 0; c_max_len = 0;
  for (int g = 0; g < a.n_groups; ++g) {
    const int own = r.prefix_slot[a.goff[g]], L = r.past_len[a.goff[g]];
    goff[g] = a.goff[g]; hbase[g] = (int64_t)own * cfg.max_ctx; hlen[g] = L; owner[g] = own; pos[g] = L;
    c_max_group = std::max(c_max_group, a.goff[g + 1] - a.goff[g]);
    c_max_len = std::max(c_max_len, L);
  }
  goff[a.n_groups] = a.goff[a.n_groups];
}

// The guidance of a call, validated ahead of its tail (r: ALL wanted rows of the call) and before any device work; the pairs are
// compacted into g_host (an unguided output row has no record) and the device block is allocated here, by the first call that
// carries guidance.
inline int LlmCached::guide_check(const LlmRows& r, const LlmTail& t, const LlmGuide& g) {
  auto bad = [&](const std::string& m) { e->set_error(m); return VSTAR_ERR_INVALID; };
  if (t.kind != LlmTail::ARGMAX && t.kind != LlmTail::SAMPLE) {
    static const char* const names[] = {"arg-max", "sampling", "beam", "scoring", "verify", "contrast"};
    return bad(std::string("guidance with the ") + names[t.kind] + " tail is not supported (the arg-max and sampling tails take it)");
  }
  const int n_want = r.n_want, n_out = g.n_out;
  if (n_out < 1 || n_out > n_want || !g.neg || !g.scale || !g.log_beta)
    return bad("guidance: n_out must be in [1, n_want] and neg, scale and log_beta are required");
  const size_t W = (size_t)max_want;
  g_host.assign(4 * W, 0);
  int32_t *cond = g_host.data(), *neg = cond + W;
  float *scale = (float*)(cond + 2 * W), *beta = (float*)(cond + 3 * W);
  std::vector<char> owned((size_t)n_want, 0);
  g_pairs = 0;
  for (int j = 0; j < n_out; ++j) {
    if (g.neg[j] == -1) continue;
    if (g.neg[j] < n_out || g.neg[j] >= n_want) return bad("guidance: neg must be -1 (unguided) or an index into want in [n_out, n_want)");
    if (owned[(size_t)g.neg[j]]++) return bad("guidance: a negative row belongs to two output rows");
    cond[g_pairs] = j; neg[g_pairs] = g.neg[j]; scale[g_pairs] = g.scale[j]; beta[g_pairs] = g.log_beta[j];
    ++g_pairs;
  }
  for (int k = n_out; k < n_want; ++k)
    if (!owned[(size_t)k]) return bad("guidance: a negative row (want[n_out ..]) belongs to no output row");
  if (g_pairs)
    if (const char* m = vstar_guide_check(n_want, cfg.vocab, g_pairs, cond, neg, scale, beta)) return bad(std::string("guidance: ") + m);
  if (!d_guide) {     // one block: a failed allocation leaves nothing behind and the engine as it was
    int32_t* blk = nullptr;
    const int rc = e->dalloc(&blk, 4 * W);
    if (rc) { (void)hipGetLastError(); return rc; }
    d_guide = blk;
  }
  return 0;
}

// The edits of a call, validated next to its tail (after the rows: the row fault is the one reported) and before any device work;
// the device arrays for the lists are allocated here, by the first call that carries edits.
inline int LlmCached::edits_check(const LlmRows& r, const LlmTail& t, const LlmEdits& ed) {
  if (t.kind == LlmTail::BEAM) {
    e->set_error("logits edits with the beam tail are not supported: HF applies the processors to the log-softmax output, whose "
                 "log-sum-exp is that of the UNEDITED row; editing the logits ahead of the beam select would compute something else");
    return VSTAR_ERR_INVALID;
  }
  if (t.kind == LlmTail::CONTRAST) { e->set_error("logits edits with the contrast tail are not supported (open follow-up)"); return VSTAR_ERR_INVALID; }
  if (t.kind == LlmTail::SCORE) {
    e->set_error("logits edits with the scoring tail are not supported: a target's likelihood under edited logits has no reference meaning");
    return VSTAR_ERR_INVALID;
  }
  if (r.n_want < 1) { e->set_error("logits edits: no wanted rows"); return VSTAR_ERR_INVALID; }
  // (the size first: a call above the capacity is refused for its size, without walking lists that long)
  if (ed.off && (int64_t)ed.off[3 * r.n_want] > edit_capacity()) {
    e->set_error("logits edits: " + std::to_string(ed.off[3 * r.n_want]) + " token ids in one call exceed the capacity of " +
                 std::to_string(edit_capacity()) + " (max_want * (max_ctx + 2048))");
    return VSTAR_ERR_INVALID;
  }
  if (const char* m = vstar_edit_check(r.n_want, cfg.vocab, ed.off, ed.tok, ed.penalty)) { e->set_error(std::string("logits edits: ") + m); return VSTAR_ERR_INVALID; }
  if (!d_eoff) {      // one block: a failed allocation leaves nothing behind and the engine as it was
    const size_t n_off = (size_t)3 * max_want + 1, n_words = n_off + (size_t)max_want + (size_t)edit_capacity();
    int32_t* blk = nullptr;
    const int rc = e->dalloc(&blk, n_words);
    if (rc) { (void)hipGetLastError(); return rc; }
    d_eoff = blk;
    d_epen = (float*)(blk + n_off);
    d_etok = blk + n_off + max_want;
  }
  return 0;
}

// The log-probability stage of a call, validated behind its tail and edits and before any device work; its device arrays are
// allocated here, by the first call that asks.
inline int LlmCached::logprobs_check(const LlmRows& r, const LlmTail& t) {
  if (t.kind == LlmTail::BEAM) {
    e->set_error("log-probabilities with the beam tail are not supported: the beam candidates already carry their scores");
    return VSTAR_ERR_INVALID;
  }
  if (t.kind == LlmTail::CONTRAST) { e->set_error("log-probabilities with the contrast tail are not supported (open follow-up)"); return VSTAR_ERR_INVALID; }
  if (t.kind == LlmTail::SCORE) {
    e->set_error("log-probabilities with the scoring tail are not supported: it already returns the target's nll and rank");
    return VSTAR_ERR_INVALID;
  }
  const LlmLogprobArgs& a = t.lp;
  if (r.n_want < 1 || !a.lp_out) { e->set_error("logprobs: no wanted rows / token_logprob output"); return VSTAR_ERR_INVALID; }
  if (const char* m = vstar_logprob_check(r.n_want, cfg.vocab, nullptr, a.n_top)) { e->set_error(m); return VSTAR_ERR_INVALID; }
  if ((a.n_top > 0) != (a.top_lp_out && a.top_tok_out) || (a.n_top == 0 && (a.top_lp_out || a.top_tok_out))) {
    e->set_error("logprobs: top_logprob and top_token are required with n_top > 0 and must be null with n_top == 0");
    return VSTAR_ERR_INVALID;
  }
  if (!d_lp) {        // one block: a failed allocation leaves nothing behind and the engine as it was
    const size_t W = (size_t)max_want, n_words = 2 * W + 2 * W * VSTAR_LOGPROB_MAX_TOP;
    int32_t* blk = nullptr;
    const int rc = e->dalloc(&blk, n_words);
    if (rc) { (void)hipGetLastError(); return rc; }
    d_lp = (float*)blk;
    d_lp_rank = blk + W;
    d_lp_top = (float*)(blk + 2 * W);
    d_lp_tok = blk + 2 * W + W * VSTAR_LOGPROB_MAX_TOP;
  }
  return 0;
}

// A tail's copies, in stream order: uploads (`in`, host -> dev) go out with the row metadata before the layers, downloads (dev ->
// `out`, host) behind the tail.  An entry whose host pointer is null (an output the caller did not ask for, greedy verify's
// params, the unused entries of the array) or that has zero bytes is no copy.
inline std::array<LlmCached::TailCopy, 6> LlmCached::tail_copies(const LlmTail& t, int n_want) {
  const size_t nw4 = (size_t)n_want * 4, np = (size_t)n_want * sizeof(vstar_vqa_sampling), nwp = (size_t)n_want * sizeof(vstar_vqa_warpers);
  const LlmBeamArgs& b = t.beam;
  const LlmVerifyArgs& v = t.verify;
  const size_t nc4 = (size_t)b.n_groups * b.n_cand * 4;
  switch (t.kind) {
    case LlmTail::ARGMAX: return {{{d_argmax, nullptr, t.tokens_out, nw4}}};
    case LlmTail::SAMPLE: return {{{d_sparams, t.params, nullptr, np}, {d_swarp, t.warpers, nullptr, nwp}, {d_argmax, nullptr, t.tokens_out, nw4}}};
    case LlmTail::BEAM:
      return {{{d_bscore, b.scores, nullptr, nw4}, {d_goff, b.goff, nullptr, (size_t)(b.n_groups + 1) * 4},
               {d_cand_s, nullptr, b.cand_s, nc4}, {d_cand_t, nullptr, b.cand_tok, nc4}, {d_cand_r, nullptr, b.cand_row, nc4}}};
    case LlmTail::SCORE: return {{{d_starget, t.score.targets, nullptr, nw4}, {d_nll, nullptr, t.score.nll, nw4}, {d_srank, nullptr, t.score.rank, nw4}}};
    case LlmTail::VERIFY:
      return {{{d_sparams, t.params, nullptr, np}, {d_goff, v.goff, nullptr, (size_t)(v.n_groups + 1) * 4}, {d_vdraft, v.draft, nullptr, nw4},
               {d_vacc, nullptr, v.n_accept, (size_t)v.n_groups * 4}, {d_vtok, nullptr, v.tokens, nw4}, {d_swarp, t.warpers, nullptr, nwp}}};
    case LlmTail::CONTRAST: {    // (the metadata block goes out with the row metadata: contrast_meta)
      const LlmContrastArgs& c = t.con;
      const size_t ng = c.goff ? (size_t)c.n_groups : (size_t)n_want, nk4 = ng * c.k * 4;
      return {{{c_prob, c.cand_prob, nullptr, nw4}, {c_sel, nullptr, c.sel, ng * 4}, {c_ntok, nullptr, c.next_tok, nk4},
               {c_nprob, nullptr, c.next_prob, nk4}, {c_pen, nullptr, c.pen_out, nw4}}};
    }
  }
  return {};
}

// the tail's kernel(s) on rows [0, m) of the logits buffer = wanted rows [w0, w0 + m) (w0 > 0: the scoring tail's later chunks)
inline int LlmCached::tail_launch(const LlmTail& t, int w0, int m) {
  const int V = cfg.vocab;
  const int64_t ld = (int64_t)vpad();
  switch (t.kind) {
    case LlmTail::ARGMAX: LCHK(argmax_rows_lp(logits, m, V, ld, d_argmax, e->stream)); break;
    case LlmTail::SAMPLE:      // d_argmax receives the drawn tokens
      LCHK(vstar_sample_rows_lp(logits, m, V, ld, d_sparams, t.warpers ? d_swarp : nullptr, d_argmax, nullptr, nullptr, e->stream));
      break;
    case LlmTail::BEAM:        // each group's n_cand best candidates
      LCHK(vstar_beam_select_lp(logits, m, V, ld, d_bscore, t.beam.n_groups, d_goff, t.beam.n_cand, beam_ws, d_cand_s, d_cand_t, d_cand_r,
                                nullptr, e->stream));
      break;
    case LlmTail::SCORE:       // only nll / rank leave
      LCHK(vstar_score_rows_lp(logits, m, V, ld, d_starget + w0, d_nll + w0, t.score.rank ? d_srank + w0 : nullptr, nullptr, e->stream));
      break;
    case LlmTail::VERIFY:      // per group the accepted count, per row the token; d_argmax / d_vflag are its scratch
      LCHK(vstar_verify_rows_lp(logits, m, V, ld, d_goff, t.verify.n_groups, d_vdraft, t.params ? d_sparams : nullptr,
                                t.warpers ? d_swarp : nullptr, d_argmax, d_vflag, d_vacc, d_vtok, e->stream));
      break;
    case LlmTail::CONTRAST: {
      const LlmContrastArgs& c = t.con;
      const int H = cfg.hidden;
      const int64_t* dst = c_meta_at<int64_t>(c_meta, 0);
      if (!c.goff) {           // begin: every new row's final-norm row into its slot's history; the wanted rows' next candidates
        LCHK(vstar_contrast_fill_lp(lx, nullptr, final_norm, cfg.rms_eps, c_fill_rows, H, dst, c_hist, c_hist_rn, e->stream));
        LCHK(vstar_contrast_topk_lp(logits, m, V, ld, c.k, c_ntok, c_nprob, e->stream));
        break;
      }
      const vstar_contrast_groups gr{c.n_groups, c_max_group, c_max_len, c_meta_at<int32_t>(c_meta, 2), c_meta_at<int64_t>(c_meta, 1),
                                     c_meta_at<int32_t>(c_meta, 3)};
      LCHK(vstar_contrast_fill_lp(lx, d_want, final_norm, cfg.rms_eps, m, H, dst, c_cand, c_cand_rn, e->stream));
      c_cand_rows = m;
      LCHK(vstar_contrast_penalty_lp(c_cand, c_cand_rn, m, H, c_hist, c_hist_rn, gr, c_pen, e->stream));
      LCHK(vstar_contrast_select_lp(logits, m, V, ld, c_cand, c_cand_rn, H, c_prob, c_pen, c.alpha, c.k, c_hist, c_hist_rn, gr, c_sel, c_ntok,
                                    c_nprob, e->stream));
      vstar_contrast_kv ck{kv.l0.k, kv.l0.v, kv.l0.ks, kv.l0.vs, kv.l0.fmt == KV_FMT_MXFP8 ? 1 : 2, kv.layers, cfg.heads, cfg.max_ctx,
                           kv.layer_stride, kv.l0.slot_stride};
      LCHK(vstar_contrast_adopt(ck, c.n_groups, gr.goff, c_sel, c_meta_at<int32_t>(c_meta, 6), c_meta_at<int32_t>(c_meta, 4),
                                c_meta_at<int32_t>(c_meta, 5), e->stream));
      break;
    }
  }
  return 0;
}

inline int LlmCached::forward(const LlmRows& rw, const LlmTail& tail, const LlmEdits* edits, const LlmGuide* guide) {
  if (!ready) { e->set_error("language-model runner not initialised"); return VSTAR_ERR_STATE; }
  const LlmCachedCfg& c = cfg;
  const int nseq = rw.nseq, n_want = rw.n_want;
  const int32_t *row_off = rw.row_off, *src = rw.src, *kv_slot = rw.kv_slot, *prefix_slot = rw.prefix_slot, *past_len = rw.past_len, *want = rw.want;
  if (nseq <= 0 || nseq > seq_cap() || !row_off || !src || !kv_slot || !prefix_slot || !past_len || n_want < 0 ||
      (tail.kind != LlmTail::SCORE && n_want > max_want) || (n_want && !want)) {
    e->set_error("llm forward: bad argument");
    return VSTAR_ERR_INVALID;
  }
  LCHK(hipSetDevice(e->device));
  const int R = row_off[nseq];
  int maxT = 0, max_keys = 0;
  bool all_fresh = true;
  for (int i = 0; i < nseq; ++i) {
    const int T = row_off[i + 1] - row_off[i];
    if (T <= 0 || past_len[i] < 0 || past_len[i] + T > c.max_ctx) { e->set_error("sequence length exceeds max_ctx (or is empty)"); return VSTAR_ERR_INVALID; }
    if (kv_slot[i] < 0 || kv_slot[i] >= c.max_slots || prefix_slot[i] < 0 || prefix_slot[i] >= c.max_slots) {
      e->set_error("KV slot out of range");
      return VSTAR_ERR_INVALID;
    }
    if (past_len[i] == 0 && prefix_slot[i] != kv_slot[i]) { e->set_error("prefix slot without a prefix"); return VSTAR_ERR_INVALID; }
    maxT = T > maxT ? T : maxT;
    max_keys = past_len[i] + T > max_keys ? past_len[i] + T : max_keys;
    all_fresh = all_fresh && past_len[i] == 0;
  }
  for (int j = 0; j < n_want; ++j)
    if (want[j] < 0 || want[j] >= R) { e->set_error("want row out of range"); return VSTAR_ERR_INVALID; }
  // with guidance the tail, the edits and the log-probabilities describe the OUTPUT rows, the first n_out wanted rows (LlmGuide)
  if (guide) RC(guide_check(rw, tail, *guide));
  const int n_out = guide ? guide->n_out : n_want;
  LlmRows rt = rw;
  rt.n_want = n_out;
  RC(tail_check(rt, tail));
  if (edits) RC(edits_check(rt, tail, *edits));
  if (tail.has_lp) RC(logprobs_check(rt, tail));
  // ---- KV ancestry: a continued sequence in an ancestral slot attends through the table ----
  bool use_anc = false;
  for (int i = 0; i < nseq; ++i) {
    const bool fork = past_len[i] > 0 && prefix_slot[i] != kv_slot[i];
    if (fork && anc_flag[prefix_slot[i]]) {      // its [0, past) is scattered over other slots: not one prefix slot
      e->set_error("forking from a beam-reordered KV slot is not supported (kv_copy it into a slot of its own first)");
      return VSTAR_ERR_INVALID;
    }
    use_anc = use_anc || (!fork && past_len[i] > 0 && anc_flag[kv_slot[i]]);
  }
  const bool prefill = all_fresh && R > 64;
  const int rows = prefill ? nseq * maxT : R;
  if (rows > c.max_rows) { e->set_error("too many rows for one forward call (max_rows)"); return VSTAR_ERR_INVALID; }
  for (int i = 0; i < nseq; ++i) {
    const int s = kv_slot[i];
    if (past_len[i] > 0 && prefix_slot[i] != s) {
      // a fork into slot s: its [0, past) lives in the (non-ancestral) prefix slot, the rest in s itself.  In an ANC call the
      // table must say so (s becomes ancestral); otherwise the plain kernels read the prefix and s goes back to identity.
      if (use_anc) {
        LCHK(kv_anc_fill(d_anc, s, prefix_slot[i], 0, past_len[i], c.max_ctx, e->stream));
        LCHK(kv_anc_fill(d_anc, s, s, past_len[i], c.max_ctx, c.max_ctx, e->stream));
        anc_flag[s] = 1;
      } else if (anc_flag[s]) {
        LCHK(kv_anc_fill(d_anc, s, s, 0, c.max_ctx, c.max_ctx, e->stream));
        anc_flag[s] = 0;
      }
    } else if (past_len[i] == 0 && anc_flag[s]) {      // a fresh sequence in a reordered slot: the slot owns its rows again
      LCHK(kv_anc_fill(d_anc, s, s, 0, c.max_ctx, c.max_ctx, e->stream));
      anc_flag[s] = 0;
    }
  }
  // ---- row metadata ----
  std::vector<int32_t> h_src((size_t)rows, INT32_MIN), h_pos((size_t)rows, -1), h_slot((size_t)rows, 0), h_seq((size_t)rows, 0);
  std::vector<int32_t> h_want((size_t)(n_want ? n_want : 1), 0), remap((size_t)R);
  for (int i = 0; i < nseq; ++i) {
    const int T = row_off[i + 1] - row_off[i];
    for (int t = 0; t < T; ++t) {
      const int r = prefill ? i * maxT + t : row_off[i] + t;
      h_src[r] = src[row_off[i] + t];
      h_pos[r] = past_len[i] + t;
      h_slot[r] = kv_slot[i];
      h_seq[r] = i;
      remap[row_off[i] + t] = r;
    }
  }
  for (int j = 0; j < n_want; ++j) h_want[j] = remap[want[j]];
  std::vector<int32_t> h_seqmeta((size_t)3 * seq_cap(), 0);
  for (int i = 0; i < nseq; ++i) seq_set(h_seqmeta, i, kv_slot[i], prefix_slot[i], past_len[i]);
  LCHK(hipMemcpyAsync(d_src, h_src.data(), (size_t)rows * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_row_pos, h_pos.data(), (size_t)rows * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_row_slot, h_slot.data(), (size_t)rows * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_row_seq, h_seq.data(), (size_t)rows * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_seq, h_seqmeta.data(), h_seqmeta.size() * 4, hipMemcpyHostToDevice, e->stream));
  if (n_want) LCHK(hipMemcpyAsync(d_want, h_want.data(), (size_t)n_want * 4, hipMemcpyHostToDevice, e->stream));
  if (tail.kind == LlmTail::CONTRAST) {
    contrast_meta(rw, tail, h_pos, h_slot, rows);
    c_fill_rows = rows;
    LCHK(hipMemcpyAsync(c_meta, c_meta_host.data(), c_meta_host.size(), hipMemcpyHostToDevice, e->stream));
  } else if (c_hist) {         // host arithmetic only: the history of a slot ends where this call starts writing its K/V rows
    for (int i = 0; i < nseq; ++i) hist_lower(kv_slot[i], past_len[i]);
  }
  const std::array<TailCopy, 6> copies = tail_copies(tail, n_out);
  for (const TailCopy& x : copies)
    if (x.in && x.bytes) LCHK(hipMemcpyAsync(x.dev, x.in, x.bytes, hipMemcpyHostToDevice, e->stream));
  if (edits) {
    const size_t n_tok = (size_t)edits->off[3 * n_out];
    LCHK(hipMemcpyAsync(d_eoff, edits->off, ((size_t)3 * n_out + 1) * 4, hipMemcpyHostToDevice, e->stream));
    if (n_tok) LCHK(hipMemcpyAsync(d_etok, edits->tok, n_tok * 4, hipMemcpyHostToDevice, e->stream));
    if (edits->penalty) LCHK(hipMemcpyAsync(d_epen, edits->penalty, (size_t)n_out * 4, hipMemcpyHostToDevice, e->stream));
  }
  if (guide && g_pairs) LCHK(hipMemcpyAsync(d_guide, g_host.data(), g_host.size() * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipStreamSynchronize(e->stream));       // the host vectors above go out of scope at return; keep it simple
  LCHK(hipEventRecord(ev0, e->stream));
  // ---- inputs_embeds (prepare_inputs_labels_for_multimodal, llava_search_arch.py:96-266) ----
  LCHK(embed_rows(d_src, embed, c.vocab, feats, n_feat_rows, lx, rows, c.hidden, e->stream));
  if (use_anc) LCHK(kv_anc_mark(d_row_slot, d_row_pos, rows, d_anc, c.max_ctx, e->stream));   // the new rows live in their own slot
  if (prefill) RC(llm_layers_prefill(nseq, maxT));
  else RC(llm_layers_cached(rows, max_keys, maxT == 1, use_anc ? d_anc : nullptr));
  // ---- head + tail, max_want wanted rows at a time: one pass, except for the scoring tail (CHUNKING RULE, LlmScoreArgs) ----
  for (int w0 = 0; w0 < n_want; w0 += max_want) {
    int m = n_want - w0 < max_want ? n_want - w0 : max_want;
    RC(head(w0, m));
    if (guide) {          // (one chunk: w0 == 0) output row j <- guided(row j, its negative row); the stages behind see rows [0, n_out)
      if (g_pairs)
        LCHK(vstar_guide_rows_lp(logits, c.vocab, (int64_t)vpad(), g_pairs, d_guide, d_guide + max_want, (const float*)(d_guide + 2 * max_want),
                                 (const float*)(d_guide + 3 * max_want), e->stream));
      m = n_out;
    }
    if (edits) LCHK(vstar_edit_rows_lp(logits, m, c.vocab, (int64_t)vpad(), d_eoff + 3 * w0, d_etok, d_epen + w0, e->stream));
    RC(tail_launch(tail, w0, m));
    if (tail.has_lp)      // (one chunk: w0 == 0) the row the tail just read, the token it just chose
      LCHK(vstar_logprob_rows_lp(logits, m, c.vocab, (int64_t)vpad(), tail.kind == LlmTail::VERIFY ? d_vtok : d_argmax, tail.lp.n_top, d_lp,
                                 tail.lp.rank_out ? d_lp_rank : nullptr, d_lp_top, d_lp_tok, e->stream));
  }
  LCHK(hipEventRecord(ev1, e->stream));
  if (n_out && tail.logits_out)
    LCHK(hipMemcpy2DAsync(tail.logits_out, (size_t)c.vocab * 2, logits, vpad() * 2, (size_t)c.vocab * 2, n_out,
                            hipMemcpyDeviceToHost, e->stream));
  for (const TailCopy& x : copies)
    if (x.out && x.bytes) LCHK(hipMemcpyAsync(x.out, x.dev, x.bytes, hipMemcpyDeviceToHost, e->stream));
  if (tail.has_lp) {
    const LlmLogprobArgs& a = tail.lp;
    const size_t nt4 = (size_t)n_out * a.n_top * 4;
    LCHK(hipMemcpyAsync(a.lp_out, d_lp, (size_t)n_out * 4, hipMemcpyDeviceToHost, e->stream));
    if (a.rank_out) LCHK(hipMemcpyAsync(a.rank_out, d_lp_rank, (size_t)n_out * 4, hipMemcpyDeviceToHost, e->stream));
    if (nt4) {
      LCHK(hipMemcpyAsync(a.top_lp_out, d_lp_top, nt4, hipMemcpyDeviceToHost, e->stream));
      LCHK(hipMemcpyAsync(a.top_tok_out, d_lp_tok, nt4, hipMemcpyDeviceToHost, e->stream));
    }
  }
  LCHK(hipStreamSynchronize(e->stream));
  if (tail.kind == LlmTail::CONTRAST) {          // the histories now describe: begin — the slot up to its new rows; step — the owner up to
    const LlmContrastArgs& a = tail.con;         // the winner's row, and nothing of a candidate slot that is not its group's owner
    for (int i = 0; i < nseq; ++i) hist_len[kv_slot[i]] = a.goff ? 0 : past_len[i] + (row_off[i + 1] - row_off[i]);
    for (int g = 0; a.goff && g < a.n_groups; ++g) hist_len[prefix_slot[a.goff[g]]] = past_len[a.goff[g]] + 1;
  }
  float ms = 0;
  if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) last_ms = ms;
  e->collect_profile();
  return 0;
}

// Beam reorder without moving K/V: entries [lo, hi) of dst[i]'s ancestry = those of src[i], all sources read first (swaps and
// repeated sources are fine); the destinations become ancestral slots.
inline int LlmCached::kv_reorder(int n, const int32_t* dst, const int32_t* src, int lo, int hi) {
  if (!ready) { e->set_error("language-model runner not initialised"); return VSTAR_ERR_STATE; }
  const LlmCachedCfg& c = cfg;
  if (n <= 0 || n > c.max_slots || !dst || !src || lo < 0 || hi < lo || hi > c.max_ctx) {
    e->set_error("kv_reorder: bad argument (1 <= n <= max_slots, 0 <= lo <= hi <= max_ctx)");
    return VSTAR_ERR_INVALID;
  }
  std::vector<char> seen((size_t)c.max_slots, 0);
  for (int i = 0; i < n; ++i) {
    if (dst[i] < 0 || dst[i] >= c.max_slots || src[i] < 0 || src[i] >= c.max_slots) { e->set_error("kv_reorder: KV slot out of range"); return VSTAR_ERR_INVALID; }
    if (seen[dst[i]]) { e->set_error("kv_reorder: a destination slot appears twice"); return VSTAR_ERR_INVALID; }
    seen[dst[i]] = 1;
  }
  if (hi == lo) return 0;
  LCHK(hipSetDevice(e->device));
  std::vector<int32_t> ds((size_t)2 * n);
  for (int i = 0; i < n; ++i) { ds[i] = dst[i]; ds[(size_t)n + i] = src[i]; }
  LCHK(hipMemcpyAsync(d_reo, ds.data(), ds.size() * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(kv_anc_reorder(d_anc, d_anc_tmp, d_reo, d_reo + n, n, lo, hi, c.max_ctx, e->stream));
  LCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; ++i) { anc_flag[dst[i]] = 1; hist_lower(dst[i], lo); }
  return 0;
}

// Physical copy of K/V rows [lo, hi) of every layer into dst's own rows, read through src's ancestry; dst's ancestry becomes the
// identity (dst is no longer ancestral).
inline int LlmCached::kv_copy(int dst, int src, int lo, int hi) {
  if (!ready) { e->set_error("language-model runner not initialised"); return VSTAR_ERR_STATE; }
  const LlmCachedCfg& c = cfg;
  if (dst < 0 || dst >= c.max_slots || src < 0 || src >= c.max_slots || dst == src || lo < 0 || hi < lo || hi > c.max_ctx) {
    e->set_error("kv_copy: bad argument (distinct slots in range, 0 <= lo <= hi <= max_ctx)");
    return VSTAR_ERR_INVALID;
  }
  LCHK(hipSetDevice(e->device));
  LCHK(kv_copy_rows(kv.l0, kv.layers, kv.layer_stride, d_anc, dst, src, lo, hi, e->stream));
  LCHK(kv_anc_fill(d_anc, dst, dst, 0, c.max_ctx, c.max_ctx, e->stream));
  LCHK(hipStreamSynchronize(e->stream));
  anc_flag[dst] = 0;
  hist_lower(dst, lo);
  return 0;
}

namespace {
// Last node of a decode step of rows 0 .. n - 1 (one workgroup, thread r = row r).  ctl: see LlmCached::d_dec_ctl.  An unfinished
// row takes its arg-max as the next input and advances; it finishes when it emitted the eos id or reached its cap.  A FINISHED row
// is left where it is: the steps it still rides along recompute the same position of its own KV slot, so it can never leave the
// context however long its companions run, and it touches nobody else's keys.  Every row's token is logged step-major (the host
// drops what a finished row emits); then, once per step, the number of unfinished rows and — last, with a system-scope release —
// the step counter are published.  `log` is coherent HOST memory (hipHostMallocCoherent): the host polls log[0] instead of
// synchronising the stream, so the next step is already queued while it looks at this step's tokens.
__global__ void decode_advance_kernel(const int32_t* __restrict__ argmax, int32_t* src, int32_t* row_pos, int32_t* seq_past,
                                      int32_t* ctl, int32_t* log, int n, int cap_steps) {
  __shared__ int alive;
  const int r = threadIdx.x;
  if (r == 0) alive = 0;
  __syncthreads();
  const int32_t step = log[0];
  if (r < n) {
    const int32_t t = argmax[r];
    bool fin = ctl[33 + r] != 0;
    if (!fin) {
      src[r] = t;
      row_pos[r] += 1;
      seq_past[r] += 1;
      const int32_t cnt = ctl[17 + r] + 1;
      ctl[17 + r] = cnt;
      if (t == ctl[0] || cnt >= ctl[1 + r]) { fin = true; ctl[33 + r] = 1; }
    }
    if (step < cap_steps) log[2 + (int64_t)step * n + r] = t;
    if (!fin) atomicAdd(&alive, 1);
    __threadfence_system();
  }
  __syncthreads();
  if (r == 0) {
    log[1] = alive;
    __threadfence_system();
    __hip_atomic_store(&log[0], step + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
}  // namespace

// one decode step of rows 0 .. n - 1 (one row per sequence), every per-step value read from device memory: what the graph of n captures
inline int LlmCached::decode_step_body(int n, int keys_bound) {
  const LlmCachedCfg& c = cfg;
  LCHK(embed_rows(d_src, embed, c.vocab, feats, n_feat_rows, lx, n, c.hidden, e->stream));
  RC(llm_layers_cached(n, keys_bound, true));
  dec_attn_path = cached_attention_last_path();
  RC(head(0, n));
  LCHK(argmax_rows_lp(logits, n, c.vocab, (int64_t)vpad(), d_argmax, e->stream));
  hipLaunchKernelGGL(decode_advance_kernel, dim3(1), dim3(64), 0, e->stream, d_argmax, d_src, d_row_pos, seq_array(2), d_dec_ctl,
                     h_dec_log, n, dec_log_steps);
  LCHK(hipGetLastError());
  return 0;
}

// the per-call state of decode_greedy: sequence i is row i and lives in KV slot i with `past[i]` positions cached
inline int LlmCached::decode_state(int n, const int32_t* first, const int32_t* past, const int32_t* caps, int eos_id) {
  std::vector<int32_t> seqmeta((size_t)3 * seq_cap(), 0), iota((size_t)n), ctl(1 + 3 * DEC_BATCH_MAX, 0);
  int alive = 0;
  ctl[0] = eos_id;
  for (int i = 0; i < n; ++i) {
    seq_set(seqmeta, i, i, i, past[i]);
    iota[i] = i;
    const bool fin = first[i] == eos_id || caps[i] <= 1;
    ctl[1 + i] = caps[i]; ctl[17 + i] = 1; ctl[33 + i] = fin;
    alive += !fin;
  }
  LCHK(hipMemcpyAsync(d_src, first, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_row_pos, past, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_row_slot, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_row_seq, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_seq, seqmeta.data(), seqmeta.size() * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_want, iota.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipMemcpyAsync(d_dec_ctl, ctl.data(), ctl.size() * 4, hipMemcpyHostToDevice, e->stream));
  LCHK(hipStreamSynchronize(e->stream));
  h_dec_log[0] = 0;
  h_dec_log[1] = alive;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  return 0;
}

// Greedy continuation of n sequences at once: sequence i sits in KV slot i with past[i] positions cached, first[i] is its prefill's
// arg-max, caps[i] >= 1 the tokens it may emit in all.  Row i of out_ids (row stride out_ld) receives its tokens, n_out[i] their
// count; it stops at its cap or at eos_id (stored).  One graph per n; VSTAR_DECODE_GRAPH=0, event profiling, a refused capture or a
// failed warm-up step run the same n-row step launch by launch, with the same keys_bound — so the same attention path and partition
// span, the same bits.  Nothing is launched when no row has a step to take.  A beam-reordered (ancestral) slot is refused: the
// step's attention reads no ancestry.
inline int LlmCached::decode_greedy(int n, const int32_t* first, const int32_t* past, const int32_t* caps, int eos_id, int32_t* out_ids,
                                    int64_t out_ld, int32_t* n_out) {
  const LlmCachedCfg& c = cfg;
  if (!ready) { e->set_error("language-model runner not initialised"); return VSTAR_ERR_STATE; }
  if (n < 1 || n > dec_rows_max()) { e->set_error("greedy decode: row count out of range"); return VSTAR_ERR_INVALID; }
  static const bool disabled = [] { const char* v = getenv("VSTAR_DECODE_GRAPH"); return v && atoi(v) == 0; }();
  std::vector<char> fin((size_t)n, 0);
  int alive = 0, max_steps = 0;
  for (int i = 0; i < n; ++i) {
    if (caps[i] < 1 || past[i] < 1 || past[i] + caps[i] - 1 > c.max_ctx || anc_flag[i]) {
      e->set_error("greedy decode: a sequence's cap or cached length is out of range");
      return VSTAR_ERR_INVALID;
    }
    out_ids[(int64_t)i * out_ld] = first[i];
    n_out[i] = 1;
    fin[i] = first[i] == eos_id || caps[i] <= 1;
    if (!fin[i]) { ++alive; max_steps = std::max(max_steps, caps[i] - 1); }
  }
  if (alive == 0) return 0;                             // every answer is its prefill's arg-max alone: no decode step at all
  for (int i = 0; i < n; ++i) hist_lower(i, past[i]);
  LCHK(hipSetDevice(e->device));
  if (!d_dec_ctl) RC(e->dalloc(&d_dec_ctl, (size_t)1 + 3 * DEC_BATCH_MAX));
  if (!h_dec_log) {
    dec_log_steps = c.max_ctx;
    void* hp = nullptr;
    if (hipHostMalloc(&hp, ((size_t)dec_log_steps * dec_rows_max() + 2) * 4, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
      (void)hipGetLastError();
      e->set_error("greedy decode: no pinned host memory for the token log");
      return VSTAR_ERR_NOMEM;
    }
    h_dec_log = (int32_t*)hp;
  }
  const int keys_bound = c.max_ctx;       // sizes the attention launch (LDS: 4 B per key, split / partition span): fixed for the graphs' lifetime
  RC(decode_state(n, first, past, caps, eos_id));
  int launched = 0;
  if (!disabled && !e->profile && !dec_graph[n]) {
    // the first step runs UNCAPTURED: it is a real decode step (its tokens are consumed below) and it takes every one-time
    // hipFuncSetAttribute of the launch helpers out of the capture
    if (decode_step_body(n, keys_bound) != 0 || hipStreamSynchronize(e->stream) != hipSuccess) {
      (void)hipGetLastError();
      e->set_error("");
      RC(decode_state(n, first, past, caps, eos_id));      // start again, launch by launch (a step rewrites the same K/V rows)
    } else {
      launched = 1;
      dec_graph[n] = e->capture_exec(e->stream, [&] { return decode_step_body(n, keys_bound); });    // refused: launch by launch
    }
  }
  const hipGraphExec_t exec = (disabled || e->profile) ? nullptr : dec_graph[n];
  const int DEPTH = 2;                                  // decode steps queued ahead of the step the host is waiting for
  int done_steps = 0;
  LCHK(hipEventRecord(ev0, e->stream));
  const int launched0 = launched;
  while (alive > 0 && done_steps < max_steps) {
    // step k (1-based) produces token k of every row; keep steps done_steps + 1 .. done_steps + DEPTH queued while the device still
    // reports an unfinished row
    while (launched < std::min(max_steps, done_steps + DEPTH) && __atomic_load_n(&h_dec_log[1], __ATOMIC_ACQUIRE) > 0) {
      if (exec) LCHK(hipGraphLaunch(exec, e->stream));
      else RC(decode_step_body(n, keys_bound));
      ++launched;
    }
    if (launched <= done_steps) { set_error("greedy decode: the device reports no unfinished row, the host has one"); return VSTAR_ERR_HIP; }
    unsigned spins = 0;
    while (__atomic_load_n(&h_dec_log[0], __ATOMIC_ACQUIRE) < done_steps + 1) {
      if ((++spins & 4095u) == 0) {
        const hipError_t q = hipStreamQuery(e->stream);
        if (q == hipSuccess) {
          if (__atomic_load_n(&h_dec_log[0], __ATOMIC_ACQUIRE) >= done_steps + 1) break;
          set_error("greedy decode: a step completed without emitting its tokens");
          return VSTAR_ERR_HIP;
        }
        if (q != hipErrorNotReady) { set_error(std::string("greedy decode: ") + hipGetErrorString(q)); return VSTAR_ERR_HIP; }
      }
      __builtin_ia32_pause();
    }
    const volatile int32_t* row = h_dec_log + 2 + (int64_t)done_steps * n;
    for (int i = 0; i < n; ++i) {
      if (fin[i]) continue;
      const int32_t t = row[i];
      out_ids[(int64_t)i * out_ld + n_out[i]++] = t;
      if (t == eos_id || n_out[i] >= caps[i]) { fin[i] = 1; --alive; }
    }
    ++done_steps;
  }
  LCHK(hipEventRecord(ev1, e->stream));
  LCHK(hipStreamSynchronize(e->stream));
  float ms = 0;
  const int timed = launched - launched0;
  if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess && timed > 0) last_ms = ms / timed;
  e->collect_profile();
  return 0;
}

#undef LCHK

}  // namespace VS_NS
using namespace VS_NS;
