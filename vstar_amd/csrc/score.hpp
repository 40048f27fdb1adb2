// score.hpp — the scoring tail of the language-model forward (score.hip): the negative log-likelihood of one target token per
// logits row, on rows that stay on the device.  DESIGN.md §8.3.  Compiled once (not per dtype), one launcher per storage type,
// like sample.hpp / beam.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One workgroup per row r of x ([rows, ld] raw 16-bit elements, the first `vocab` of each row used), target d_targets[r] (DEVICE):
//   lse     = max + log(sum exp(x_i - max)) in double, fixed per-thread and reduction order (row_lse.hpp, shared with beam.hip)
//   nll[r]  = (float)(lse - (double)x[target]): one round-to-nearest-even double -> fp32.  x[target] = -inf gives +inf; NaN
//             logits follow IEEE arithmetic (NaN); a row whose maximum is +inf gives NaN (inf - inf).
//   rank[r] = #{i : x_i > x[target]} (nullable; 0 = the arg-max is the target, NaN compares false)
//   lse_out[r] (nullable, double): the log-sum-exp itself.
// All outputs are DEVICE arrays.  Rows of up to 32768 elements are staged in LDS once; longer rows re-read their logits.
// Stream-ordered, no host synchronisation, capturable.  rows <= 65535, 1 <= vocab <= 2^22; the targets are checked by the
// caller with vstar_score_check.
hipError_t vstar_score_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_targets, float* nll,
                                int32_t* rank, double* lse_out, hipStream_t s);
hipError_t vstar_score_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_targets, float* nll,
                                 int32_t* rank, double* lse_out, hipStream_t s);
// host-side check of the arguments (host copy of the targets); nullptr when valid, else the message
const char* vstar_score_check(int rows, int vocab, const int32_t* targets);
