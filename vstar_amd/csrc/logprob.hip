// logprob.hip — the log-probability stage behind the picking tails of the language-model forward: per logits row the
// log-probability and rank of the token the tail just chose and the n_top (<= 32) best alternatives, so that a confidence moves a
// handful of floats to the host instead of a vocabulary row.  DESIGN.md §8.9.
//
// One launch, one workgroup (16 waves) per row:
//   lse    row_lse.hpp: max, then sum exp(x - max) in double (deterministic; the same code and bits as score.hip / beam.hip)
//   lp     (float)((double)x[t] - lse), one rounding; rank = #{i : x_i > x[t]}, counted in the pass that fills the first histogram
//   K_T    the n-th largest order-preserving 16-bit key of the RAW logits (NaN -> -inf, -0 -> +0): a radix select over the two key
//          bytes (LDS histograms, row_select.hpp) — the keys are exact images of the values, so equal keys are equal values
//   pick   every i with key > K_T, then the lowest-index ties at K_T — an exact scan in index order over thread-contiguous chunks
//   sort   the n picks are ranked in the workgroup under (key descending, index ascending) and written in rank order
// Rows of up to CACHE elements keep their bits in LDS after the first read; longer rows re-read the logits from L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "logprob.hpp"
#include "row_lse.hpp"
#include "row_select.hpp"

namespace {

using rowlse::bits2f;
using rowlse::CACHE;
using rowlse::THREADS;
using rowlse::WAVES;
using rowsel::value_key;
constexpr int MAX_VOCAB = 1 << 22;
constexpr int MAX_TOP = VSTAR_LOGPROB_MAX_TOP;

template <bool CACHED>
struct LogprobSmem : rowlse::Scratch {
  uint16_t bits[CACHED ? CACHE : 1];   // raw logits bits
  uint32_t hist[256];
  int sel;
  uint32_t sel_above;
  uint32_t pick_key[MAX_TOP];
  int32_t pick_idx[MAX_TOP];
};

template <bool BF16, bool CACHED>
__global__ __launch_bounds__(THREADS) void logprob_rows_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                               const int32_t* __restrict__ tokens, int n_top,
                                                               float* __restrict__ lp_tok, int32_t* __restrict__ rank,
                                                               float* __restrict__ top_lp, int32_t* __restrict__ top_tok) {
  __shared__ LogprobSmem<CACHED> sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xr = x + (int64_t)row * ld;
  const int t = tokens[row];
  if ((uint32_t)t >= (uint32_t)vocab) {              // (uniform) no token on this row: nothing of it is read
    if (tid == 0) {
      lp_tok[row] = NAN;
      if (rank) rank[row] = -1;
    }
    if (tid < n_top) {
      top_lp[(int64_t)row * n_top + tid] = NAN;
      top_tok[(int64_t)row * n_top + tid] = -1;
    }
    return;
  }
  if (tid < 256) sm.hist[tid] = 0;
  const double lse = rowlse::row_lse<BF16, CACHED>(sm, xr, vocab);
  auto raw = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.bits[i];
    else return xr[i];
  };
  const float xt = bits2f<BF16>(xr[t]);
  if (tid == 0) lp_tok[row] = (float)((double)xt - lse);
  if (!rank && !n_top) return;                       // (uniform: kernel arguments)
  // ---- the rank of the chosen token, and the high-byte histogram of the value keys ----
  uint32_t n_above = 0;
  for (int i = tid; i < vocab; i += THREADS) {
    const uint32_t b = raw(i);
    n_above += bits2f<BF16>(b) > xt;
    if (n_top) atomicAdd(&sm.hist[value_key<BF16>(b) >> 8], 1u);
  }
  if (rank) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_above += __shfl_xor(n_above, o, 64);
    if ((tid & 63) == 0) sm.wu[tid >> 6] = n_above;
    __syncthreads();
    if (tid == 0) {
      uint32_t s = 0;
      for (int w = 0; w < WAVES; ++w) s += sm.wu[w];
      rank[row] = (int32_t)s;
    }
    __syncthreads();                                 // (sm.wu is the scans' scratch below)
  }
  if (!n_top) return;
  // ---- K_T and the picks (row_select.hpp; both bins exist: n <= vocab) ----
  const uint32_t n = (uint32_t)(n_top < vocab ? n_top : vocab);
  rowsel::pick_top<BF16>(sm, raw, vocab, n);
  // ---- sort: each pick's rank among the n under (key descending, index ascending) ----
  if (tid >= n_top) return;
  float* ol = top_lp + (int64_t)row * n_top;
  int32_t* ot = top_tok + (int64_t)row * n_top;
  if ((uint32_t)tid >= n) {                          // n_top > vocab: the entries behind the row's elements
    ol[tid] = NAN;
    ot[tid] = -1;
    return;
  }
  const int32_t ii = sm.pick_idx[tid];
  const uint32_t r = rowsel::pick_rank(sm, n, (uint32_t)tid);
  ot[r] = ii;
  ol[r] = (float)((double)bits2f<BF16>(raw(ii)) - lse);
}

template <bool BF16>
hipError_t logprob_rows(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_tokens, int n_top, float* lp_tok,
                        int32_t* rank, float* top_lp, int32_t* top_tok, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || !d_tokens || !lp_tok || rows > 65535 || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab || n_top < 0 || n_top > MAX_TOP ||
      (n_top && (!top_lp || !top_tok)))
    return hipErrorInvalidValue;
  if (vocab <= CACHE)
    hipLaunchKernelGGL((logprob_rows_kernel<BF16, true>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_tokens, n_top, lp_tok, rank,
                       top_lp, top_tok);
  else
    hipLaunchKernelGGL((logprob_rows_kernel<BF16, false>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_tokens, n_top, lp_tok, rank,
                       top_lp, top_tok);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_logprob_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_tokens, int n_top,
                                  float* lp_tok, int32_t* rank, float* top_lp, int32_t* top_tok, hipStream_t s) {
  return logprob_rows<false>(x, rows, vocab, ld, d_tokens, n_top, lp_tok, rank, top_lp, top_tok, s);
}

hipError_t vstar_logprob_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_tokens, int n_top,
                                   float* lp_tok, int32_t* rank, float* top_lp, int32_t* top_tok, hipStream_t s) {
  return logprob_rows<true>(x, rows, vocab, ld, d_tokens, n_top, lp_tok, rank, top_lp, top_tok, s);
}

const char* vstar_logprob_check(int rows, int vocab, const int32_t* tokens, int n_top) {
  if (rows <= 0) return "logprobs: no rows";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "logprobs: vocabulary size out of range [1, 2^22]";
  if (n_top < 0 || n_top > MAX_TOP) return "logprobs: n_top out of range [0, 32]";
  if (tokens)
    for (int r = 0; r < rows; ++r)
      if (tokens[r] >= vocab) return "logprobs: a token id is outside [0, vocab) (negative: no token on that row)";
  return nullptr;
}
