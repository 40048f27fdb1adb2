// beam.hpp — the beam-search tail of the language-model decode (beam.hip): HF 4.31 beam_search candidate selection on logits
// rows that stay on the device.  DESIGN.md §8.2.  Compiled once (not per dtype), one launcher per storage type, like sample.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int VSTAR_BEAM_MAX_K = 16;           // beams per group (rows of one sample)
constexpr int VSTAR_BEAM_MAX_CAND = 32;        // candidates per group (2k)

// Candidates of beam search for `rows` logits rows x ([rows, ld] raw 16-bit elements, the first `vocab` of each used), row r
// carrying the fp32 beam score d_scores[r]; rows d_goff[g] .. d_goff[g+1]-1 form group g (one sample).  Per row:
// lp = log_softmax(x) (log-sum-exp in double, rounded to the storage type), s = score + float(lp) (one fp32 add).  Per group:
// the n_cand largest s over all of its rows, sorted by (s descending, row_in_group * vocab + token ascending), written to
// cand_s / cand_tok / cand_row [n_groups, n_cand] (device).  lp_out (nullable, device, [rows, vocab] fp32): the rounded lp.
// ws: device workspace of vstar_beam_ws_bytes(rows, n_cand) bytes.  Stream-ordered, no host synchronisation; the arguments are
// checked by the caller with vstar_beam_check.
hipError_t vstar_beam_select_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const float* d_scores, int n_groups,
                                 const int32_t* d_goff, int n_cand, void* ws, float* cand_s, int32_t* cand_tok, int32_t* cand_row,
                                 float* lp_out, hipStream_t s);
hipError_t vstar_beam_select_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const float* d_scores, int n_groups,
                                  const int32_t* d_goff, int n_cand, void* ws, float* cand_s, int32_t* cand_tok, int32_t* cand_row,
                                  float* lp_out, hipStream_t s);
size_t vstar_beam_ws_bytes(int rows, int n_cand);
// host-side check of the arguments (host copies of scores / group offsets); nullptr when valid, else the message
const char* vstar_beam_check(int rows, int vocab, const float* scores, int n_groups, const int32_t* goff, int n_cand);
