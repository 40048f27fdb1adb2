// vqa_ops.hip — the operator-level entry points ("doors") of the fp16 half of libvstar_hip.so: vstar_vqa_op_* (include/vstar_vqa.h,
// include/vstar_hip.h).  A door checks its arguments on the host, runs ONE launcher (or a short fixed sequence) on device buffers the
// caller owns, synchronises the device and reports; none of them takes an engine handle.  Built once, with -DVSTAR_LP_F16; the bf16
// doors are ops.hip, and what both share is op_doors.hpp.
#ifndef VSTAR_LP_F16
#error "vqa_ops.hip is the fp16 instantiation: build with -DVSTAR_LP_F16"
#endif
#include <algorithm>
#include <type_traits>
#include "tails_lp.hpp"      // the launchers and host checks of the tails (sample / beam / score / spec / edit / logprob / contrast)
#include "op_doors.hpp"
#include "../../include/vstar_vqa.h"

namespace {
// the op's launcher for the logits' storage type, then hipDeviceSynchronize: both skipped after a failure.  P is deduced from the
// launchers alone (common_type<P>::type is a non-deduced context), so the arguments convert to the launchers' parameter types: an
// OpBuf<T> becomes its T* (OpBuf<char> a void*), nullptr the null stream
template <class... P>
void op_launch(hipError_t& e, int dtype, hipError_t (*f16)(P...), hipError_t (*bf16)(P...), typename std::common_type<P>::type... a) {
  if (e == hipSuccess) e = (dtype == VSTAR_F16 ? f16 : bf16)(a...);
  if (e == hipSuccess) e = hipDeviceSynchronize();
}
}  // namespace

// the body of vstar_vqa_op_gemm_w8 / _w4: the quantised skinny GEMV on row-major q + scale (layout 0) or on the tile-major image
// packed here from them (layout 1)
static int op_gemm_wq(int fmt, const char* fn, const char* bad_arg, const void* A, const void* Wq, const void* scale, const void* bias,
                      const void* res, void* C, int M, int N, int K, int epilogue, int kernel, const void* norm_w, float norm_eps, int layout) {
  const bool w4 = fmt == SKINNY_W_INT4G128;
  if (!A || !Wq || !scale || !C || M <= 0 || N <= 0 || K <= 0 || K % (w4 ? 128 : 64) || (kernel != 1 && kernel != 3) || (layout != 0 && layout != 1)) {
    tls_error() = std::string(fn) + bad_arg;
    return VSTAR_ERR_INVALID;
  }
  const int nt = epilogue == VSTAR_EPI_SILU_MUL ? 2 : 1;
  GemmParams p = op_dense_gemm(A, nullptr, bias, res, C, M, N, K, epilogue, norm_w, norm_eps);
  if (kernel == 3) p.tile_force = -1;
  if (!gemm_skinny_eligible(p)) return op_refuse(fn, "outside the weight-streaming kernels' domain (M <= 64)");
  if (layout == 1 && N % (16 * nt)) return op_refuse(fn, "the tile-major layout needs whole 16-row (SiLU-mul: 32-row) tiles");
  hipError_t e = hipSuccess;
  OpBuf<char> tiles(e, w4 ? skinny_tiles_w4_bytes(N, K, nt) : (size_t)N * K, layout == 1);
  if (layout == 1 && e == hipSuccess)
    e = w4 ? skinny_pack_tiles_w4((const uint32_t*)Wq, (const lp_t*)scale, tiles.p, N, K, nt, nullptr)
           : skinny_pack_tiles_w8((const int8_t*)Wq, (int8_t*)tiles.p, N, K, nt, nullptr);
  p.dw = SkinnyWeights{fmt, Wq, scale, tiles.p};
  if (e == hipSuccess) e = gemm_skinny_lp(p, epilogue, false, nullptr);
  return op_sync_device(e, fn);
}

// the shared rules of the two norm doors; returns the violated rule, or null
static const char* norm_op_check(const void* x, int64_t x_rows, const void* gamma, const void* y, int rows, int cols, const int32_t* row_index) {
  if (!x || !gamma || !y) return "x, gamma and y are required";
  if (rows < 1 || rows > (1 << 20)) return "rows in [1, 2^20]";
  if (cols < 8 || cols > 4096 || cols % 8) return "cols % 8 == 0, 8 <= cols <= 4096";
  if (!row_index) return x_rows < rows ? "x_rows < rows" : nullptr;
  for (int r = 0; r < rows; ++r)
    if (row_index[r] < 0 || row_index[r] >= x_rows) return "row_index entries must lie in [0, x_rows)";
  return nullptr;
}

extern "C" {

// ---- the tails at op level, on device logits the caller owns: checks, scratch (OpBuf), launch + synchronise, copies back ----
int vstar_vqa_op_contrast(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const void* dev_cand_hidden, int hidden,
                          void* dev_hist, float* dev_hist_rnorm, int n_groups, int cap, const int32_t* hist_len, const int32_t* group_off,
                          const float* cand_prob, float alpha, int k_next, int32_t* sel_out, int32_t* next_tok, float* next_prob,
                          float* penalty_out) {
  const char* m = nullptr;
  if (!dev_logits) m = "dev_logits is NULL";
  else if (!dev_cand_hidden) m = "dev_cand_hidden is NULL";
  else if (!dev_hist || !dev_hist_rnorm) m = "dev_hist / dev_hist_rnorm is NULL";
  else if (!hist_len) m = "hist_len is NULL";
  else if (!sel_out || !next_tok || !next_prob) m = "sel_out / next_tok / next_prob is NULL";
  else if (dtype != VSTAR_F16 && dtype != VSTAR_BF16) m = "dtype must be F16 or BF16";
  else if (ld < vocab) m = "ld must be >= vocab";
  else if (hidden <= 0 || hidden % 8) m = "hidden must be a positive multiple of 8";
  else m = vstar_contrast_check(rows, vocab, n_groups, group_off, cand_prob, alpha, k_next);
  int max_len = 0, max_group = 0;
  for (int g = 0; !m && g < n_groups; ++g) {
    if (hist_len[g] < 1 || hist_len[g] >= cap) m = "hist_len must be in [1, cap)";
    max_len = std::max(max_len, hist_len[g]);
    max_group = std::max(max_group, group_off[g + 1] - group_off[g]);
  }
  if (m) return op_refuse("vstar_vqa_op_contrast", m);
  hipError_t e = hipSuccess;
  std::vector<int64_t> hbase((size_t)n_groups);
  for (int g = 0; g < n_groups; ++g) hbase[(size_t)g] = (int64_t)g * cap;
  const size_t nk = (size_t)n_groups * k_next;
  OpBuf<int32_t> d_goff(e, (size_t)n_groups + 1), d_hlen(e, n_groups), d_sel(e, n_groups), d_nt(e, nk);
  OpBuf<int64_t> d_hbase(e, n_groups);
  OpBuf<float> d_rn(e, rows), d_prob(e, rows), d_pen(e, rows), d_np(e, nk);
  d_goff.upload(group_off);
  d_hlen.upload(hist_len);
  d_hbase.upload(hbase.data());
  d_prob.upload(cand_prob);
  const vstar_contrast_groups gr{n_groups, max_group, max_len, d_goff, d_hbase, d_hlen};
  const bool bf = dtype == VSTAR_BF16;
  const uint16_t* cand = (const uint16_t*)dev_cand_hidden;
  if (e == hipSuccess) e = (bf ? vstar_contrast_rnorm_bf16 : vstar_contrast_rnorm_f16)(cand, rows, hidden, d_rn, nullptr);
  if (e == hipSuccess) e = (bf ? vstar_contrast_penalty_bf16 : vstar_contrast_penalty_f16)(cand, d_rn, rows, hidden, (const uint16_t*)dev_hist, dev_hist_rnorm, gr, d_pen, nullptr);
  if (e == hipSuccess)
    e = (bf ? vstar_contrast_select_bf16 : vstar_contrast_select_f16)((const uint16_t*)dev_logits, rows, vocab, ld, cand, d_rn, hidden, d_prob, d_pen, alpha, k_next,
                                                                      (uint16_t*)dev_hist, dev_hist_rnorm, gr, d_sel, d_nt, d_np, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  d_sel.download(sel_out);
  d_nt.download(next_tok);
  d_np.download(next_prob);
  d_pen.download(penalty_out);
  return op_result(e, "vstar_vqa_op_contrast");
}

int vstar_vqa_op_sample(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* params,
                        int32_t* tokens, float* u_out, int32_t* n_kept) {
  return vstar_vqa_op_sample_warp(dev_logits, dtype, rows, vocab, ld, params, nullptr, tokens, u_out, n_kept, nullptr);
}

int vstar_vqa_op_sample_warp(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* params,
                             const vstar_vqa_warpers* warpers, int32_t* tokens, float* u_out, int32_t* n_kept, uint8_t* kept_mask) {
  const char* fn = "vstar_vqa_op_sample";
  if (!dev_logits || !params || !tokens || rows <= 0 || rows > 65535 || vocab <= 0 || vocab > (1 << 22) || ld < vocab ||
      (dtype != VSTAR_F16 && dtype != VSTAR_BF16))
    return op_refuse(fn, "bad argument");
  if (!vstar_sample_params_valid(params, rows)) return op_refuse(fn, "temperature must be > 0 and finite, top_k >= 0, top_p >= 0");
  if (const char* m = warpers ? vstar_warpers_check(warpers, rows) : nullptr) return op_refuse("vstar_vqa_op_sample_warp", m);
  hipError_t e = hipSuccess;
  OpBuf<vstar_vqa_sampling> d_p(e, rows);
  OpBuf<vstar_vqa_warpers> d_w(e, rows, warpers != nullptr);
  OpBuf<int32_t> d_tok(e, rows), d_kept(e, rows);
  OpBuf<float> d_u(e, rows);
  OpBuf<uint8_t> d_mask(e, (size_t)rows * vocab, kept_mask != nullptr);
  d_p.upload(params);
  d_w.upload(warpers);
  op_launch(e, dtype, vstar_sample_rows_f16, vstar_sample_rows_bf16, (const uint16_t*)dev_logits, rows, vocab, ld, d_p, d_w, d_tok, d_u, d_kept,
            d_mask, nullptr);
  d_tok.download(tokens);
  d_u.download(u_out);
  d_kept.download(n_kept);
  d_mask.download(kept_mask);
  return op_result(e, fn);
}

int vstar_vqa_op_beam_select(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const float* beam_scores, int n_groups,
                             const int32_t* group_off, int n_cand, float* cand_scores, int32_t* cand_tokens, int32_t* cand_rows,
                             float* lp_out) {
  const char* fn = "vstar_vqa_op_beam_select";
  if (!dev_logits || !cand_scores || !cand_tokens || !cand_rows || rows > 65535 || ld < vocab ||
      (dtype != VSTAR_F16 && dtype != VSTAR_BF16))
    return op_refuse(fn, "bad argument");
  if (const char* m = vstar_beam_check(rows, vocab, beam_scores, n_groups, group_off, n_cand)) return op_refuse(fn, m);
  const size_t nc = (size_t)n_groups * n_cand;
  hipError_t e = hipSuccess;
  OpBuf<float> d_sc(e, rows), d_cs(e, nc), d_lp(e, (size_t)rows * vocab, lp_out != nullptr);
  OpBuf<int32_t> d_go(e, (size_t)n_groups + 1), d_ct(e, nc), d_cr(e, nc);
  OpBuf<char> d_ws(e, vstar_beam_ws_bytes(rows, n_cand));
  d_sc.upload(beam_scores);
  d_go.upload(group_off);
  op_launch(e, dtype, vstar_beam_select_f16, vstar_beam_select_bf16, (const uint16_t*)dev_logits, rows, vocab, ld, d_sc, n_groups, d_go,
            n_cand, d_ws, d_cs, d_ct, d_cr, d_lp, nullptr);
  d_cs.download(cand_scores);
  d_ct.download(cand_tokens);
  d_cr.download(cand_rows);
  d_lp.download(lp_out);
  return op_result(e, fn);
}

int vstar_vqa_op_score(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* targets, float* nll,
                       int32_t* target_rank, double* lse_out) {
  const char* fn = "vstar_vqa_op_score";
  if (!dev_logits || !nll || rows > 65535 || ld < vocab || (dtype != VSTAR_F16 && dtype != VSTAR_BF16)) return op_refuse(fn, "bad argument");
  if (const char* m = vstar_score_check(rows, vocab, targets)) return op_refuse(fn, m);
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_t(e, rows), d_r(e, rows, target_rank != nullptr);
  OpBuf<float> d_n(e, rows);
  OpBuf<double> d_l(e, rows, lse_out != nullptr);
  d_t.upload(targets);
  op_launch(e, dtype, vstar_score_rows_f16, vstar_score_rows_bf16, (const uint16_t*)dev_logits, rows, vocab, ld, d_t, d_n, d_r, d_l, nullptr);
  d_n.download(nll);
  d_r.download(target_rank);
  d_l.download(lse_out);
  return op_result(e, fn);
}

int vstar_vqa_op_verify(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                        const int32_t* draft, const vstar_vqa_sampling* params, int32_t* n_accept_out, int32_t* tokens_out) {
  return vstar_vqa_op_verify_warp(dev_logits, dtype, rows, vocab, ld, group_off, n_groups, draft, params, nullptr, n_accept_out, tokens_out);
}

int vstar_vqa_op_verify_warp(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                             const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers,
                             int32_t* n_accept_out, int32_t* tokens_out) {
  const char* fn = "vstar_vqa_op_verify";
  if (!dev_logits || !n_accept_out || !tokens_out || rows > 65535 || ld < vocab || (dtype != VSTAR_F16 && dtype != VSTAR_BF16))
    return op_refuse(fn, "bad argument");
  if (const char* m = vstar_verify_check(rows, vocab, n_groups, group_off, draft)) return op_refuse(fn, m);
  if (params && !vstar_sample_params_valid(params, rows)) return op_refuse(fn, "temperature must be > 0 and finite, top_k >= 0, top_p >= 0");
  if (const char* m = warpers ? vstar_warpers_check(warpers, rows) : nullptr) return op_refuse("vstar_vqa_op_verify_warp", m);
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_go(e, (size_t)n_groups + 1), d_dr(e, rows), d_ch(e, rows), d_fl(e, rows), d_ac(e, n_groups), d_tok(e, rows);
  OpBuf<vstar_vqa_sampling> d_p(e, rows, params != nullptr);
  OpBuf<vstar_vqa_warpers> d_w(e, rows, params != nullptr && warpers != nullptr);
  d_go.upload(group_off);
  d_dr.upload(draft);
  d_p.upload(params);
  d_w.upload(warpers);
  op_launch(e, dtype, vstar_verify_rows_f16, vstar_verify_rows_bf16, (const uint16_t*)dev_logits, rows, vocab, ld, d_go, n_groups, d_dr, d_p,
            d_w, d_ch, d_fl, d_ac, d_tok, nullptr);
  d_ac.download(n_accept_out);
  d_tok.download(tokens_out);
  return op_result(e, fn);
}

int vstar_vqa_op_edit(void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok,
                      const float* penalty) {
  const char* fn = "vstar_vqa_op_edit";
  if (!dev_logits || rows > 65535 || ld < vocab || (dtype != VSTAR_F16 && dtype != VSTAR_BF16)) return op_refuse(fn, "bad argument");
  if (const char* m = vstar_edit_check(rows, vocab, off, tok, penalty)) return op_refuse(fn, m);
  hipError_t e = hipSuccess;
  const size_t n_tok = (size_t)off[3 * rows];
  OpBuf<int32_t> d_off(e, (size_t)3 * rows + 1), d_tok(e, n_tok, n_tok != 0);
  OpBuf<float> d_pen(e, rows, penalty != nullptr);
  d_off.upload(off);
  d_tok.upload(tok);
  d_pen.upload(penalty);
  op_launch(e, dtype, vstar_edit_rows_f16, vstar_edit_rows_bf16, (uint16_t*)dev_logits, rows, vocab, ld, d_off, d_tok, d_pen, nullptr);
  return op_result(e, fn);
}

int vstar_vqa_op_logprobs(const void* dev_logits, int dtype, int rows, int vocab, int64_t ld, const int32_t* tokens, int n_top,
                          float* token_logprob, int32_t* token_rank, float* top_logprob, int32_t* top_token) {
  const char* fn = "vstar_vqa_op_logprobs";
  if (!dev_logits || !tokens || !token_logprob || rows > 65535 || ld < vocab || (dtype != VSTAR_F16 && dtype != VSTAR_BF16))
    return op_refuse(fn, "bad argument");
  if (const char* m = vstar_logprob_check(rows, vocab, tokens, n_top)) return op_refuse(fn, m);
  if (n_top > 0 ? (!top_logprob || !top_token) : (top_logprob || top_token))
    return op_refuse(fn, "top_logprob and top_token are required with n_top > 0 and must be null with n_top == 0");
  hipError_t e = hipSuccess;
  const size_t nt = (size_t)rows * n_top;
  OpBuf<int32_t> d_t(e, rows), d_r(e, rows, token_rank != nullptr), d_tt(e, nt, nt != 0);
  OpBuf<float> d_l(e, rows), d_tl(e, nt, nt != 0);
  d_t.upload(tokens);
  op_launch(e, dtype, vstar_logprob_rows_f16, vstar_logprob_rows_bf16, (const uint16_t*)dev_logits, rows, vocab, ld, d_t, n_top, d_l, d_r,
            d_tl, d_tt, nullptr);
  d_l.download(token_logprob);
  d_r.download(token_rank);
  d_tl.download(top_logprob);
  d_tt.download(top_token);
  return op_result(e, fn);
}

// the guidance kernel (guide.hip) on device logits: the records are checked, uploaded, one launch
int vstar_vqa_guide_rows(void* dev_logits, int dtype, int rows, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row,
                         const int32_t* neg_row, const float* scale, const float* log_beta) {
  const char* fn = "vstar_vqa_guide_rows";
  if (!dev_logits || !cond_row || !neg_row || !scale || !log_beta) return op_refuse(fn, "a NULL pointer");
  if (dtype != VSTAR_F16 && dtype != VSTAR_BF16) return op_refuse(fn, "dtype must be F16 or BF16");
  if (ld < vocab) return op_refuse(fn, "ld must be >= vocab");
  if (const char* m = vstar_guide_check(rows, vocab, n_pairs, cond_row, neg_row, scale, log_beta)) return op_refuse(fn, m);
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_c(e, n_pairs), d_n(e, n_pairs);
  OpBuf<float> d_s(e, n_pairs), d_b(e, n_pairs);
  d_c.upload(cond_row);
  d_n.upload(neg_row);
  d_s.upload(scale);
  d_b.upload(log_beta);
  op_launch(e, dtype, vstar_guide_rows_f16, vstar_guide_rows_bf16, (uint16_t*)dev_logits, vocab, ld, n_pairs, d_c, d_n, d_s, d_b, nullptr);
  return op_result(e, fn);
}

// ---- GEMM, the weight-only quantisers and their GEMVs, the KV quantiser ----
int vstar_vqa_op_gemm(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K,
                      int epilogue, int kernel, const void* norm_w, float norm_eps) {
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || K % 64) { tls_error() = "bad argument"; return VSTAR_ERR_INVALID; }
  GemmParams p = op_dense_gemm(A, W, bias, res, C, M, N, K, epilogue, norm_w, norm_eps);
  if (kernel == 3) p.tile_force = -1;      // the register-streaming skinny kernel even where the LDS-ring variant would run
  if (kernel == 4) p.tile_force = GEMM_TILE_4W;      // round 6: the 4-wave / AGPR 256^2 kernel, error outside its domain
  if (kernel == 5) p.tile_force = 256;               // the 8-wave 256^2 kernel
  const bool skinny = kernel == 1 || kernel == 3 || (kernel == 0 && gemm_skinny_eligible(p));
  return op_sync_device(skinny ? gemm_skinny_lp(p, epilogue, false, nullptr) : gemm_lp(p, epilogue, false, nullptr), "vstar_vqa_op_gemm");
}

int vstar_vqa_op_quantize_w8(const void* dev_W_f16, int rows, int K, void* dev_q_i8, float* dev_scale_f32, void* dev_What_f16) {
  const char* fn = "vstar_vqa_op_quantize_w8";
  if (!dev_W_f16 || !dev_q_i8 || !dev_scale_f32 || rows <= 0 || K <= 0 || K % 8) return op_refuse(fn, "bad argument (K must be a multiple of 8)");
  return op_sync_device(quantize_rows_w8((const lp_t*)dev_W_f16, rows, K, (int8_t*)dev_q_i8, dev_scale_f32, (lp_t*)dev_What_f16, nullptr), fn);
}

int vstar_vqa_op_gemm_w8(const void* A, const void* Wq, const float* scale, const void* bias, const void* res, void* C, int M, int N,
                         int K, int epilogue, int kernel, const void* norm_w, float norm_eps, int layout) {
  return op_gemm_wq(SKINNY_W_INT8, "vstar_vqa_op_gemm_w8", ": bad argument (kernel 1 or 3, layout 0 or 1, K % 64 == 0)", A, Wq, scale, bias, res,
                    C, M, N, K, epilogue, kernel, norm_w, norm_eps, layout);
}

int vstar_vqa_op_quantize_w4(const void* dev_W_f16, int rows, int K, void* dev_q_u32, void* dev_scale_f16, void* dev_What_f16) {
  const char* fn = "vstar_vqa_op_quantize_w4";
  if (!dev_W_f16 || !dev_q_u32 || !dev_scale_f16 || rows <= 0 || K <= 0 || K % 128) return op_refuse(fn, "bad argument (K must be a multiple of 128)");
  return op_sync_device(quantize_groups_w4((const lp_t*)dev_W_f16, rows, K, (uint32_t*)dev_q_u32, (lp_t*)dev_scale_f16, (lp_t*)dev_What_f16, nullptr), fn);
}

int vstar_vqa_op_gemm_w4(const void* A, const void* Wq, const void* scale, const void* bias, const void* res, void* C, int M, int N,
                         int K, int epilogue, int kernel, const void* norm_w, float norm_eps, int layout) {
  return op_gemm_wq(SKINNY_W_INT4G128, "vstar_vqa_op_gemm_w4",
                    ": bad argument (kernel 1 or 3, layout 0 or 1, K % 128 == 0, weights and scales not null)", A, Wq, scale, bias, res, C, M, N,
                    K, epilogue, kernel, norm_w, norm_eps, layout);
}

int vstar_vqa_op_kv_quantize(const void* dev_x_f16, int rows, void* dev_codes_u8, void* dev_scales_u8, void* dev_xhat_f16) {
  const char* fn = "vstar_vqa_op_kv_quantize";
  if (!dev_x_f16 || !dev_codes_u8 || !dev_scales_u8 || rows <= 0 || rows > (1 << 24))
    return op_refuse(fn, "bad argument (x, codes and scales not null, 0 < rows <= 2^24)");
  return op_sync_device(kv_quantize_rows((const lp_t*)dev_x_f16, rows, (uint8_t*)dev_codes_u8, (uint8_t*)dev_scales_u8, (lp_t*)dev_xhat_f16, nullptr), fn);
}

// ---- op-level doors of the decode-side kernels: the checks and bodies are op_doors.hpp's (shared with the bf16 doors of ops.hip) ----
int vstar_vqa_op_rope_kv_append(void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                                const vstar_vqa_kv_rows* rows) {
  return door_rope_kv_append("vstar_vqa_op_rope_kv_append", dev_qkv, dev_cos_sin, table_rows, kv, rows);
}

int vstar_vqa_op_cached_attention(void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                                  const vstar_vqa_kv_rows* rows, int max_keys, int path, int repeat, void* dev_out, int* path_ran) {
  return door_cached_attention("vstar_vqa_op_cached_attention", dev_qkv, dev_cos_sin, table_rows, kv, rows, max_keys, path, repeat, dev_out,
                               path_ran);
}

int vstar_vqa_op_perceiver_attention(const void* dev_q, const void* dev_kv, void* dev_out, int n, int L, int NK, int H, int DH) {
  const char* fn = "vstar_vqa_op_perceiver_attention";
  if (!dev_q || !dev_kv || !dev_out || n < 1 || L < 1 || H < 1 || (DH != 32 && DH != 64 && DH != 96) || NK < 1 || NK > 512 ||
      (int64_t)n * L * H > (1 << 24))
    return op_refuse(fn, "bad argument (pointers not null, DH in {32, 64, 96}, 1 <= NK <= 512, n * L * H in [1, 2^24])");
  return op_sync_device(perceiver_attention((const lp_t*)dev_q, (const lp_t*)dev_kv, (lp_t*)dev_out, n, L, NK, H, DH, nullptr), fn);
}

int vstar_vqa_op_embed_rows(const int32_t* host_src, int R, const void* dev_table, int vocab, const void* dev_feats,
                            int64_t n_feat_rows, void* dev_x, int C) {
  return door_embed_rows("vstar_vqa_op_embed_rows", host_src, R, dev_table, vocab, dev_feats, n_feat_rows, dev_x, C);
}

int vstar_vqa_op_argmax_rows(const void* dev_x, int rows, int cols, int64_t ld, int32_t* host_out) {
  return door_argmax_rows("vstar_vqa_op_argmax_rows", dev_x, rows, cols, ld, host_out);
}

// ---- op-level doors of the fp16 PREFILL kernels (attention.hip, norm.hip, elementwise.hip built with -DVSTAR_LP_F16;
// tests/test_f16_prefill_gpu.py): every buffer comes with its extent in rows, a violated rule is VSTAR_ERR_INVALID with a message before
// anything is allocated or launched; no arithmetic here ----
int vstar_vqa_op_attention(const void* dev_qkv, int64_t qkv_rows, void* dev_out, int64_t out_rows, int B, int S, int H, int D, int causal) {
  const char* fn = "vstar_vqa_op_attention";
  if (!dev_qkv || !dev_out) return op_refuse(fn, "qkv and out are required");
  if (D != 64 && D != 128) return op_refuse(fn, "D must be 64 or 128");
  if (B < 1 || S < 1 || H < 1 || H > 256 || (causal != 0 && causal != 1)) return op_refuse(fn, "B, S >= 1, H in [1, 256], causal 0 or 1");
  if ((int64_t)B * S > (1 << 24) || (int64_t)S * 3 * H * D * 2 >= ((int64_t)1 << 31))
    return op_refuse(fn, "B * S <= 2^24 and one sequence's qkv rows below 2^31 bytes");
  if (qkv_rows < (int64_t)B * S || out_rows < (int64_t)B * S) return op_refuse(fn, "qkv_rows / out_rows < B * S");
  return op_sync_device(attn_forward((const lp_t*)dev_qkv, (lp_t*)dev_out, B, S, H, D, causal, 1.0f / sqrtf((float)D), nullptr), fn);
}

int vstar_vqa_op_layernorm(const void* dev_x, int64_t x_rows, const void* dev_gamma, const void* dev_beta, void* dev_y, int rows, int cols,
                           float eps, const int32_t* host_row_index, int act) {
  const char* fn = "vstar_vqa_op_layernorm";
  const char* bad = (act != 0 && act != 1) ? "act must be 0 or 1" : norm_op_check(dev_x, x_rows, dev_gamma, dev_y, rows, cols, host_row_index);
  if (bad) return op_refuse(fn, bad);
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_idx(e, rows, host_row_index != nullptr);
  d_idx.upload(host_row_index);
  if (e == hipSuccess)
    e = layernorm_lp((const lp_t*)dev_x, (const lp_t*)dev_gamma, (const lp_t*)dev_beta, (lp_t*)dev_y, rows, cols, eps, d_idx, act, nullptr);
  return op_sync_device(e, fn);
}

int vstar_vqa_op_rmsnorm(const void* dev_x, int64_t x_rows, const void* dev_gamma, void* dev_y, int rows, int cols, float eps,
                         const int32_t* host_row_index) {
  const char* fn = "vstar_vqa_op_rmsnorm";
  const char* bad = norm_op_check(dev_x, x_rows, dev_gamma, dev_y, rows, cols, host_row_index);
  if (bad) return op_refuse(fn, bad);
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_idx(e, rows, host_row_index != nullptr);
  d_idx.upload(host_row_index);
  if (e == hipSuccess) e = rmsnorm_lp((const lp_t*)dev_x, (const lp_t*)dev_gamma, (lp_t*)dev_y, rows, cols, eps, d_idx, nullptr);
  return op_sync_device(e, fn);
}

int vstar_vqa_op_add_bcast(const void* dev_a, const void* dev_b, void* dev_out, int64_t rows, int cols, int64_t b_rows) {
  const char* fn = "vstar_vqa_op_add_bcast";
  if (!dev_a || !dev_b || !dev_out) return op_refuse(fn, "a, b and out are required");
  if (rows < 1 || rows > (1 << 24) || b_rows < 1 || b_rows > rows) return op_refuse(fn, "rows in [1, 2^24], b_rows in [1, rows]");
  if (cols < 8 || cols > 65536 || cols % 8) return op_refuse(fn, "cols % 8 == 0, 8 <= cols <= 65536");
  return op_sync_device(add_bcast((const lp_t*)dev_a, (const lp_t*)dev_b, (lp_t*)dev_out, rows, cols, b_rows, nullptr), fn);
}

int vstar_vqa_op_vit_assemble_tokens(const void* dev_patch, const void* dev_cls, const void* dev_pos, void* dev_tokens, int B, int P, int C) {
  const char* fn = "vstar_vqa_op_vit_assemble_tokens";
  if (!dev_patch || !dev_cls || !dev_pos || !dev_tokens) return op_refuse(fn, "patch, cls, pos and tokens are required");
  if (B < 1 || P < 1 || (int64_t)B * (P + 1) > (1 << 24)) return op_refuse(fn, "B, P >= 1, B * (P + 1) <= 2^24");
  if (C < 8 || C > 65536 || C % 8) return op_refuse(fn, "C % 8 == 0, 8 <= C <= 65536");
  return op_sync_device(vit_assemble_tokens((const lp_t*)dev_patch, (const lp_t*)dev_cls, (const lp_t*)dev_pos, (lp_t*)dev_tokens, B, P, C, nullptr), fn);
}

}  // extern "C"
