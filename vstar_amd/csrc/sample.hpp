// sample.hpp — the sampling tail of the language-model decode (sample.hip): HF 4.31 generate(do_sample=True) on logits rows that
// stay on the device.  Compiled once (not per dtype): both storage types have a launcher of their own, so the two instantiations
// of llm_cached.hpp (bf16 VSM engine, fp16 VQA engine) call distinct symbols.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vstar_vqa.h"

// One workgroup per row: tokens[r] = the draw of row r of x ([rows, ld] raw 16-bit elements, the first `vocab` of each row
// used) under d_params[r] (DEVICE array).  u_out / n_kept (nullable, device): the uniform drawn and the size of the kept set.
// d_warpers (nullable, DEVICE, one record per row): the min-p / typical-p / epsilon / eta stages of DESIGN.md §8.10 behind top-p;
// kept_mask (nullable, device, uint8 [rows, vocab]): 1 where the token is in the kept set the draw was made from.  With both null
// the launch is the §8.1 kernel, bit for bit and instruction for instruction.
// Stream-ordered, no host synchronisation, capturable.  rows <= 65535, 1 <= vocab <= 2^22; parameters are checked by the caller.
hipError_t vstar_sample_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                 const vstar_vqa_warpers* d_warpers, int32_t* tokens, float* u_out, int32_t* n_kept,
                                 uint8_t* kept_mask, hipStream_t s);
hipError_t vstar_sample_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                  const vstar_vqa_warpers* d_warpers, int32_t* tokens, float* u_out, int32_t* n_kept,
                                  uint8_t* kept_mask, hipStream_t s);
// host-side check of n warper records: nullptr when valid, else the message, which names the field (min_p in [0, 1], typical_p > 0,
// epsilon_cutoff and eta_cutoff in [0, 1); NaN fails)
const char* vstar_warpers_check(const vstar_vqa_warpers* w, int n);
// host-side check of one parameter record (temperature > 0 and finite, top_k >= 0, top_p in [0, 1] or above, not NaN)
bool vstar_sample_params_valid(const vstar_vqa_sampling& p);
inline bool vstar_sample_params_valid(const vstar_vqa_sampling* p, int n) {      // ... of n records
  for (int i = 0; i < n; ++i)
    if (!vstar_sample_params_valid(p[i])) return false;
  return true;
}
