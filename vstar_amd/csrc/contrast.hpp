// contrast.hpp — the device side of contrastive search (HF 4.31 generate(penalty_alpha, top_k): contrastive_search + _ranking_fast)
// behind the language-model forward (contrast.hip).  DESIGN.md §8.11.  Compiled once (not per dtype), one launcher per storage type
// T (fp16 / bf16: the logits AND the hidden rows), like logprob.hpp / beam.hpp.
//
// State of one sequence: the hidden history Hs[0 .. L) — the final-norm output of every position so far, T [L, hidden] — and the fp32
// reciprocal norm of every row.  A step sees a group of m (1 .. 32) candidate rows c with probability p_c and final-norm hidden row h_c:
//   pen_c   = max_{j < L} cos(h_c, Hs[j])
//   score_c = (1 - alpha) * p_c - alpha * pen_c;  the winner s is the largest score, the lowest c on a tie
//   Hs[L]   = h_s (and its reciprocal norm);  the next candidates are the top k of softmax(logits row of s)
// THE ARITHMETIC (fixed here once; tests/_contrast_oracle.py restates it):
//   hidden row   fill: rstd = rsqrtf(sum_sq / hidden + eps) with sum_sq in the ROW ORDER below over float(x)^2, then
//                T(w * T(x * rstd)) — the library's RMSNorm rounding points — for prefill rows and candidate rows alike
//   ROW ORDER    a row of `hidden` (% 8 == 0) elements is hidden / 8 pieces of 8; lane l of a wave owns pieces l, l + 64, ...; it adds
//                its products in fp32, piece by piece, element by element (every T * T product is exact in fp32, so a fused and an
//                unfused multiply-add agree); the 64 lane sums are added by the xor butterfly 32, 16, 8, 4, 2, 1.  A dot product and a
//                squared norm depend on their own two rows only and repeat bit for bit, whatever the launch geometry
//   rnorm        1.0f / sqrtf(sum of squares of the STORED row, ROW ORDER), both correctly rounded; 0 for an all-zero row
//   cos          dot * rnorm_candidate * rnorm_history, two fp32 multiplies in this order; a zero-norm row on either side gives 0
//                (a stated deviation: HF yields NaN).  pen is the fmaxf over j (a NaN cosine is skipped; L >= 1)
//   score        double: dsub(dmul(1.0 - (double)alpha, (double)p), dmul((double)alpha, (double)pen)), each operation rounded on its
//                own (no contraction): reproducible exactly from the returned fp32 p and pen
//   top k        logprob.hpp's top-n order (value descending, index ascending, by VALUE, a NaN sorts as -inf) through the same select
//                (row_select.hpp); p = (float)exp((double)x - lse), lse = rowlse::row_lse, the scoring tail's double log-sum-exp
// Probabilities and cosines are exact where HF rounds them to fp16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VSTAR_CONTRAST_MAX_GROUP 32     // candidate rows of one group
#define VSTAR_CONTRAST_MAX_K 32         // next candidates per group (= VSTAR_VQA_MAX_TOP_LOGPROBS)

// contrast_fill: out row dst_row[r] (an index into `out` [*, hidden] and `rnorm`; < 0: the row is skipped) = the final-norm row of
// x[src_row ? src_row[r] : r] (x [*, hidden], gain w [hidden]) and its reciprocal norm.  One wave per row.
hipError_t vstar_contrast_fill_f16(const uint16_t* x, const int32_t* src_row, const uint16_t* w, float eps, int rows, int hidden,
                                   const int64_t* dst_row, uint16_t* out, float* rnorm, hipStream_t s);
hipError_t vstar_contrast_fill_bf16(const uint16_t* x, const int32_t* src_row, const uint16_t* w, float eps, int rows, int hidden,
                                    const int64_t* dst_row, uint16_t* out, float* rnorm, hipStream_t s);
// rnorm[r] of the stored rows h [rows, hidden] alone (the op-level entry, whose candidate rows arrive already normalised)
hipError_t vstar_contrast_rnorm_f16(const uint16_t* h, int rows, int hidden, float* rnorm, hipStream_t s);
hipError_t vstar_contrast_rnorm_bf16(const uint16_t* h, int rows, int hidden, float* rnorm, hipStream_t s);

// What a step's groups are (DEVICE arrays): rows goff[g] .. goff[g+1]-1 (1 .. 32 of them) are group g's candidates; its history is
// rows hist_base[g] .. hist_base[g] + hist_len[g] - 1 of `hist` / `hist_rn` (hist_len >= 1), and the winner is appended at
// hist_base[g] + hist_len[g].
struct vstar_contrast_groups {
  int n_groups;
  int max_group;               // host-known bounds of the device arrays: the largest group (<= 32) and the longest history (>= 1);
  int max_len;                 // they size the launch, the kernels read the device values
  const int32_t* goff;         // [n_groups + 1]
  const int64_t* hist_base;    // [n_groups]
  const int32_t* hist_len;     // [n_groups]
};

// contrast_penalty: pen[r] = max_j cos(cand[r], history row j of r's group) for every candidate row r of every group.  The history
// is streamed from HBM once, 16 bytes per lane and load, a wave per history row; the group's candidate rows are staged in LDS in
// chunks of 1024 hidden elements (<= 64 KiB); L is partitioned over workgroups and the partial maxima meet in an ordered-integer
// atomicMax (max is order-independent): the launcher's first kernel writes the image of -inf, and `pen` [rows] holds ordered-integer
// IMAGES until contrast_select turns them into the floats, in place.  cand [rows, hidden], cand_rn [rows].
hipError_t vstar_contrast_penalty_f16(const uint16_t* cand, const float* cand_rn, int rows, int hidden, const uint16_t* hist,
                                      const float* hist_rn, const vstar_contrast_groups& g, float* pen, hipStream_t s);
hipError_t vstar_contrast_penalty_bf16(const uint16_t* cand, const float* cand_rn, int rows, int hidden, const uint16_t* hist,
                                       const float* hist_rn, const vstar_contrast_groups& g, float* pen, hipStream_t s);

// contrast_select: per group (one workgroup) the score and the pick sel[g] (row in group); the winner's hidden row and reciprocal norm
// appended to the history; the k_next (2 .. 32, <= vocab) best tokens of the winner's logits row x[goff[g] + sel[g]] ([rows, ld] raw
// 16-bit elements, the first `vocab` used) with their probabilities, next_tok / next_prob [n_groups, k_next].  prob [rows]: p_c.
hipError_t vstar_contrast_select_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const uint16_t* cand, const float* cand_rn,
                                     int hidden, const float* prob, float* pen, float alpha, int k_next, uint16_t* hist,
                                     float* hist_rn, const vstar_contrast_groups& g, int32_t* sel, int32_t* next_tok, float* next_prob,
                                     hipStream_t s);
hipError_t vstar_contrast_select_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const uint16_t* cand, const float* cand_rn,
                                      int hidden, const float* prob, float* pen, float alpha, int k_next, uint16_t* hist,
                                      float* hist_rn, const vstar_contrast_groups& g, int32_t* sel, int32_t* next_tok, float* next_prob,
                                      hipStream_t s);
// the begin call's form: no candidates, no history — only the top k_next of every row of x (sel == row)
hipError_t vstar_contrast_topk_f16(const uint16_t* x, int rows, int vocab, int64_t ld, int k_next, int32_t* next_tok, float* next_prob,
                                   hipStream_t s);
hipError_t vstar_contrast_topk_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, int k_next, int32_t* next_tok, float* next_prob,
                                    hipStream_t s);

// contrast_adopt: for every group whose winner's slot row_slot[goff[g] + sel[g]] is not owner[g], K and V row pos[g] of that slot
// becomes row pos[g] of the owner, in every layer and head — driven by the device-resident sel, no host round trip.  The cache is
// [layers][slots][heads][ctx][128] cells of cell_bytes (2: 16-bit cells; 1: e4m3 code bytes, with the E8M0 bytes ks / vs
// [layers][slots][heads][ctx][4]); layer_stride and slot_stride count cells.
struct vstar_contrast_kv {
  void *k, *v;
  uint8_t *ks, *vs;
  int cell_bytes, layers, heads, ctx;
  int64_t layer_stride, slot_stride;
};
hipError_t vstar_contrast_adopt(const vstar_contrast_kv& kv, int n_groups, const int32_t* goff, const int32_t* sel,
                                const int32_t* row_slot, const int32_t* owner, const int32_t* pos, hipStream_t s);

// host-side check of a step's host arguments; nullptr when valid, else the message (it names the field)
const char* vstar_contrast_check(int rows, int vocab, int n_groups, const int32_t* group_off, const float* cand_prob, float alpha,
                                 int k_next);
