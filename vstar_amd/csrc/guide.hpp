// guide.hpp — the guidance stage of the language-model decode (guide.hip): HF generate's classifier-free guidance
// (UnbatchedClassifierFreeGuidanceLogitsProcessor; visual contrastive decoding in the LLaVA literature) as one pass over a
// (conditional, negative) pair of logits rows that stay on the device, between lm_head and the logits edits.  Compiled once (not per
// dtype), one launcher per storage type, like beam.hpp / edit.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// x: [rows, ld] raw 16-bit elements.  All pointers DEVICE; n_pairs records, pair p:
//   cond_row[p], neg_row[p]   two different rows of x; no row appears in two records
//   scale[p]                  gamma, fp32, finite and >= 0
//   log_beta[p]               fp32, <= 0; -inf = the plausibility cut is off
// Per pair, T the storage type, x_c / x_u the first `vocab` elements of the conditional / negative row:
//   lse_c, lse_u = rowlse::row_lse of the two rows: the scoring / beam tails' double log-sum-exp in its fixed order, bit for bit
//   c_i = x_c[i] - lse_c, u_i = x_u[i] - lse_u, g_i = gamma * (c_i - u_i) + u_i, every operation an IEEE double operation rounded on
//   its own (no contraction); g_i is rounded ONCE to T (round to odd to fp32, then to nearest even); a finite g_i beyond T's range
//   becomes T's largest finite magnitude: finite operands never produce an infinity
//   plausibility cut (log_beta > -inf): element i is kept iff (float)x_c[i] - (float)max_j x_c[j] >= log_beta — an exact fp32
//   difference of two 16-bit values against a host-computed constant; a dropped element becomes -inf, the row maximum always stays
//   non-finite operands: x_c[i] -inf or NaN -> -inf;  x_u[i] non-finite with x_c[i] finite -> c_i rounded once (nothing to contrast
//   against);  lse_c or lse_u non-finite (a NaN or +inf element, a row of -inf) -> the whole row -inf
// The result overwrites the CONDITIONAL row, columns [0, vocab) only: columns [vocab, ld), the negative row and every row in no pair
// are never written.  Rows of up to 32768 elements keep both operand rows in LDS (2 x 64 KiB of the CU's 160 KiB), longer rows are
// re-read through L2.  One launch (one workgroup of 16 waves per pair), stream-ordered, no host synchronisation, capturable.
// 1 <= vocab <= 2^22, n_pairs <= 65535, any ld >= vocab; the records are checked by the caller with vstar_guide_check.
hipError_t vstar_guide_rows_f16(uint16_t* x, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row, const int32_t* neg_row,
                                const float* scale, const float* log_beta, hipStream_t s);
hipError_t vstar_guide_rows_bf16(uint16_t* x, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row, const int32_t* neg_row,
                                 const float* scale, const float* log_beta, hipStream_t s);
// host-side check of the records (host copies): the rows differ, lie in [0, rows) and appear once; gamma finite and >= 0; log_beta
// <= 0 and not NaN; nullptr when valid, else the message
const char* vstar_guide_check(int rows, int vocab, int n_pairs, const int32_t* cond_row, const int32_t* neg_row, const float* scale,
                              const float* log_beta);
