// sample.hpp — the sampling tail of the language-model decode (sample.hip): HF 4.31 generate(do_sample=True) on logits rows that
// stay on the device.  Compiled once (not per dtype): both storage types have a launcher of their own, so the two instantiations
// of llm_cached.hpp (bf16 VSM engine, fp16 VQA engine) call distinct symbols.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vstar_vqa.h"

// One workgroup per row: tokens[r] = the draw of row r of x ([rows, ld] raw 16-bit elements, the first `vocab` of each row
// used) under d_params[r] (DEVICE array).  u_out / n_kept (nullable, device): the uniform drawn and the size of the kept set.
// Stream-ordered, no host synchronisation, capturable.  rows <= 65535, 1 <= vocab <= 2^22; parameters are checked by the caller.
hipError_t vstar_sample_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                 int32_t* tokens, float* u_out, int32_t* n_kept, hipStream_t s);
hipError_t vstar_sample_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                  int32_t* tokens, float* u_out, int32_t* n_kept, hipStream_t s);
// host-side check of one parameter record (temperature > 0 and finite, top_k >= 0, top_p in [0, 1] or above, not NaN)
bool vstar_sample_params_valid(const vstar_vqa_sampling& p);
inline bool vstar_sample_params_valid(const vstar_vqa_sampling* p, int n) {      // ... of n records
  for (int i = 0; i < n; ++i)
    if (!vstar_sample_params_valid(p[i])) return false;
  return true;
}
