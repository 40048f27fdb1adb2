// spec.hpp — the verify tail of speculative decoding (spec.hip): per logits row a token is chosen (arg-max, or the
// §8.1 draw with an accept / residual step) and compared with the draft token that was fed as the next row; per group (one
// sequence, rows in position order) the number of accepted drafts and the chosen tokens come back.  Compiled once (not per
// dtype), one launcher per storage type, like sample.hpp / beam.hpp / score.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vstar_vqa.h"

#define VSTAR_VERIFY_MAX_GROUP 16      /* rows of one group: the current token + up to 15 drafts */

// x: [rows, ld] raw 16-bit elements, the first `vocab` of each row used.  All pointers DEVICE:
//   group_off[n_groups + 1]  rows group_off[g] .. group_off[g+1]-1 form group g (1 .. 16 rows)
//   draft[rows]              the token row j's choice is compared with; -1 = not compared (always so on a group's last row)
//   params[rows] or nullptr  nullptr: greedy — the choice of a row is argmax_rows_lp's token (first index of the largest number;
//                            NaN and -inf never win; 0 when nothing does).  Else the sampled rule of DESIGN.md §8.5.
//   warpers[rows] or nullptr the §8.10 stages behind top-p, as in sample.hpp; read only with params (greedy ignores them)
//   choice / flag [rows]     scratch: the token chosen per row and whether it accepted its draft
//   n_accept[n_groups]       a = the number of leading rows of the group that accepted their draft
//   tokens[rows]             rows r0 .. r0+a of a group: the chosen tokens (a accepted drafts + one more); the rest -1
// Two launches (one workgroup of 16 waves per row, then one thread per group), stream-ordered, no host synchronisation,
// capturable.  rows <= 65535, 1 <= vocab <= 2^22; the arguments are checked by the caller with vstar_verify_check.
hipError_t vstar_verify_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                                 const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers, int32_t* choice,
                                 int32_t* flag, int32_t* n_accept, int32_t* tokens, hipStream_t s);
hipError_t vstar_verify_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                                  const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers, int32_t* choice,
                                  int32_t* flag, int32_t* n_accept, int32_t* tokens, hipStream_t s);
// host-side check of the arguments (host copies); nullptr when valid, else the message
const char* vstar_verify_check(int rows, int vocab, int n_groups, const int32_t* group_off, const int32_t* draft);
