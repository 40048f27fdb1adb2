// edit.hpp — the logits-edit stage (edit.hip): HF generate's logits-processor list reduced to three sorted token
// lists per row — penalised (repetition penalty), banned (-inf) and allowed (everything else -inf) — applied in place to the
// logits rows between lm_head and the tail that picks a token.  Compiled once (not per dtype), one launcher per storage type,
// like sample.hpp / beam.hpp / score.hpp / spec.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// x: [rows, ld] raw 16-bit elements, the first `vocab` of each row edited in place, columns [vocab, ld) never written.  All
// pointers DEVICE:
//   off[3 * rows + 1]   CSR offsets into tok, non-decreasing, off[0] == 0.  Row j's penalised ids are tok[off[3j] .. off[3j+1]), its
//                       banned ids tok[off[3j+1] .. off[3j+2]), its allowed ids tok[off[3j+2] .. off[3j+3]); each list strictly
//                       increasing, ids in [0, vocab)
//   penalty[rows]       fp32 theta per row, finite and > 0; read only where the row's penalised list is non-empty
// Per row, T the storage type:
//   1. penalised t:  x[t] = T(f32(x[t]) < 0 ? f32(x[t]) * theta : f32(x[t]) / theta) — IEEE fp32 multiply / divide, one
//      round-to-nearest-even to T (NaN stays NaN, -0 takes the divide)
//   2. banned t:     x[t] = -inf
//   3. a non-empty allowed list:  x[t] = -inf for every t in [0, vocab) not in it
// in this order (a ban wins over a penalty; allowed and banned is -inf).  A row whose three lists are empty is neither read nor
// written.  One launch (one workgroup of 16 waves per row), stream-ordered, no host synchronisation, capturable.  rows <= 65535,
// 1 <= vocab <= 2^22, any ld >= vocab (rows need not be 16-byte aligned); the lists are checked by the caller with vstar_edit_check.
hipError_t vstar_edit_rows_f16(uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok, const float* penalty,
                               hipStream_t s);
hipError_t vstar_edit_rows_bf16(uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok, const float* penalty,
                                hipStream_t s);
// host-side check of the lists (host copies): offsets, id range, strict order, theta; nullptr when valid, else the message
const char* vstar_edit_check(int rows, int vocab, const int32_t* off, const int32_t* tok, const float* penalty);
