// tails_lp.hpp — the four decode tails (sample / beam / score / spec .hip), the logits-edit stage (edit.hip), the log-probability stage (logprob.hip), the guidance stage (guide.hip) and the contrastive-search kernels (contrast.hip) under `_lp` names, as argmax_rows_lp has one: each
// forwards to the launcher of the including instantiation's storage type (VSTAR_LP_F16: fp16, else bf16).  The .hip files stay
// compiled once, dtype-explicit; the arguments are documented at the launchers (sample.hpp, beam.hpp, score.hpp, spec.hpp, edit.hpp, logprob.hpp, contrast.hpp, guide.hpp).
#pragma once
#include "common.hpp"
#include "sample.hpp"
#include "beam.hpp"
#include "score.hpp"
#include "spec.hpp"
#include "edit.hpp"
#include "logprob.hpp"
#include "contrast.hpp"
#include "guide.hpp"

#ifdef VSTAR_LP_F16
#define VSTAR_TAIL_LP(name) name##_f16
#else
#define VSTAR_TAIL_LP(name) name##_bf16
#endif
namespace VS_NS {      // (one definition per instantiation: the two differ)
inline hipError_t vstar_sample_rows_lp(const lp_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                       const vstar_vqa_warpers* d_warpers, int32_t* tokens, float* u_out, int32_t* n_kept, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_sample_rows)(x, rows, vocab, ld, d_params, d_warpers, tokens, u_out, n_kept, nullptr, s);
}
inline hipError_t vstar_beam_select_lp(const lp_t* x, int rows, int vocab, int64_t ld, const float* d_scores, int n_groups, const int32_t* d_goff,
                                       int n_cand, void* ws, float* cand_s, int32_t* cand_tok, int32_t* cand_row, float* lp_out, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_beam_select)(x, rows, vocab, ld, d_scores, n_groups, d_goff, n_cand, ws, cand_s, cand_tok, cand_row, lp_out, s);
}
inline hipError_t vstar_score_rows_lp(const lp_t* x, int rows, int vocab, int64_t ld, const int32_t* d_targets, float* nll, int32_t* rank,
                                      double* lse_out, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_score_rows)(x, rows, vocab, ld, d_targets, nll, rank, lse_out, s);
}
inline hipError_t vstar_verify_rows_lp(const lp_t* x, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups, const int32_t* draft,
                                       const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers, int32_t* choice, int32_t* flag,
                                       int32_t* n_accept, int32_t* tokens, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_verify_rows)(x, rows, vocab, ld, group_off, n_groups, draft, params, warpers, choice, flag, n_accept, tokens, s);
}
inline hipError_t vstar_edit_rows_lp(lp_t* x, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok, const float* penalty,
                                     hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_edit_rows)(x, rows, vocab, ld, off, tok, penalty, s);
}
inline hipError_t vstar_guide_rows_lp(lp_t* x, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row, const int32_t* neg_row,
                                      const float* scale, const float* log_beta, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_guide_rows)(x, vocab, ld, n_pairs, cond_row, neg_row, scale, log_beta, s);
}
inline hipError_t vstar_logprob_rows_lp(const lp_t* x, int rows, int vocab, int64_t ld, const int32_t* d_tokens, int n_top, float* lp_tok,
                                        int32_t* rank, float* top_lp, int32_t* top_tok, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_logprob_rows)(x, rows, vocab, ld, d_tokens, n_top, lp_tok, rank, top_lp, top_tok, s);
}
inline hipError_t vstar_contrast_fill_lp(const lp_t* x, const int32_t* src_row, const lp_t* w, float eps, int rows, int hidden,
                                         const int64_t* dst_row, lp_t* out, float* rnorm, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_contrast_fill)(x, src_row, w, eps, rows, hidden, dst_row, out, rnorm, s);
}
inline hipError_t vstar_contrast_penalty_lp(const lp_t* cand, const float* cand_rn, int rows, int hidden, const lp_t* hist, const float* hist_rn,
                                            const vstar_contrast_groups& g, float* pen, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_contrast_penalty)(cand, cand_rn, rows, hidden, hist, hist_rn, g, pen, s);
}
inline hipError_t vstar_contrast_select_lp(const lp_t* x, int rows, int vocab, int64_t ld, const lp_t* cand, const float* cand_rn, int hidden,
                                           const float* prob, float* pen, float alpha, int k_next, lp_t* hist, float* hist_rn,
                                           const vstar_contrast_groups& g, int32_t* sel, int32_t* next_tok, float* next_prob, hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_contrast_select)(x, rows, vocab, ld, cand, cand_rn, hidden, prob, pen, alpha, k_next, hist, hist_rn, g, sel, next_tok,
                                              next_prob, s);
}
inline hipError_t vstar_contrast_topk_lp(const lp_t* x, int rows, int vocab, int64_t ld, int k_next, int32_t* next_tok, float* next_prob,
                                         hipStream_t s) {
  return VSTAR_TAIL_LP(vstar_contrast_topk)(x, rows, vocab, ld, k_next, next_tok, next_prob, s);
}
}  // namespace VS_NS
#undef VSTAR_TAIL_LP
