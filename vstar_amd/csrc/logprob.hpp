// logprob.hpp — the log-probability stage behind the picking tails of the language-model forward (logprob.hip): per logits row
// the log-probability and rank of the token the tail just chose and the n best alternatives, on rows that stay on the device.
// DESIGN.md §8.9.  Compiled once (not per dtype), one launcher per storage type, like score.hpp / beam.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VSTAR_LOGPROB_MAX_TOP 32

// One workgroup per row r of x ([rows, ld] raw 16-bit elements, the first `vocab` of each row used), chosen token
// t = d_tokens[r] (DEVICE):
//   lse          = rowlse::row_lse: the scoring tail's double log-sum-exp, same order, same bits
//   lp_tok[r]    = (float)((double)x[t] - lse): one round-to-nearest-even double -> fp32, the sign-flipped nll of
//                  vstar_score_rows for target t.  x[t] = -inf gives -inf; NaN logits follow IEEE arithmetic; a row whose
//                  maximum is +inf gives NaN.
//   rank[r]      = #{i : x_i > x[t]} (nullable; NaN compares false)
//   top_tok / top_lp [r, 0 .. n), n = min(n_top, vocab): the n largest elements under (value descending, index ascending), in
//                  that order; -0 and +0 tie, a NaN sorts as -inf (it never outranks a number); top_lp = (float)((double)x[i] -
//                  lse).  Entries [n, n_top) of a row are -1 / NaN.  The row stride of both arrays is n_top.
//   t < 0 (the verify tail's rows behind the acceptance; t >= vocab likewise): the row is not read; lp_tok = NaN, rank = -1,
//                  top_tok = -1, top_lp = NaN.
// 0 <= n_top <= VSTAR_LOGPROB_MAX_TOP; n_top == 0 skips the select and top_lp / top_tok may be null.  All outputs are DEVICE
// arrays.  Rows of up to 32768 elements are staged in LDS once; longer rows re-read their logits.  One launch, stream-ordered,
// no host synchronisation, capturable.  rows <= 65535, 1 <= vocab <= 2^22, ld >= vocab.
hipError_t vstar_logprob_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_tokens, int n_top,
                                  float* lp_tok, int32_t* rank, float* top_lp, int32_t* top_tok, hipStream_t s);
hipError_t vstar_logprob_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_tokens, int n_top,
                                   float* lp_tok, int32_t* rank, float* top_lp, int32_t* top_tok, hipStream_t s);
// host-side check of the arguments (tokens: a host copy, or null where they are device data that is in range by construction);
// a token of -1 or less is valid (an unread row).  nullptr when valid, else the message
const char* vstar_logprob_check(int rows, int vocab, const int32_t* tokens, int n_top);
