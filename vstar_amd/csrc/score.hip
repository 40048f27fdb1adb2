// score.hip — the scoring tail of the language-model forward: per logits row the negative log-likelihood of one target token
// (and optionally the target's rank), so that option scoring / teacher forcing moves n floats to the host instead of n x vocab
// logits.  DESIGN.md §8.3.
//
// One launch, one workgroup (16 waves) per row:
//   lse   row_lse.hpp: max, then sum exp(x - max) in double (deterministic; the same code and bits as beam.hip's row kernel)
//   nll   (float)(lse - (double)x[target]), one rounding
//   rank  #{i : x_i > x[target]}: one more pass over the row (in LDS when it fits), an integer sum
// Rows of up to CACHE elements keep their bits in LDS after the first read; longer rows re-read the logits from L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "score.hpp"
#include "row_lse.hpp"

namespace {

using rowlse::bits2f;
using rowlse::CACHE;
using rowlse::THREADS;
using rowlse::WAVES;
constexpr int MAX_VOCAB = 1 << 22;

template <bool CACHED>
struct ScoreSmem : rowlse::Scratch {
  uint16_t bits[CACHED ? CACHE : 1];   // raw logits bits
};

template <bool BF16, bool CACHED>
__global__ __launch_bounds__(THREADS) void score_rows_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                             const int32_t* __restrict__ targets, float* __restrict__ nll,
                                                             int32_t* __restrict__ rank, double* __restrict__ lse_out) {
  __shared__ ScoreSmem<CACHED> sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xr = x + (int64_t)row * ld;
  const int t = targets[row];                        // in [0, vocab): checked on the host (vstar_score_check)
  const double lse = rowlse::row_lse<BF16, CACHED>(sm, xr, vocab);
  const float xt = bits2f<BF16>(xr[t]);
  if (tid == 0) {
    nll[row] = (float)(lse - (double)xt);
    if (lse_out) lse_out[row] = lse;
  }
  if (!rank) return;                                 // (uniform: a kernel argument)
  uint32_t n = 0;
  for (int i = tid; i < vocab; i += THREADS) {
    uint32_t b;
    if constexpr (CACHED) b = sm.bits[i];
    else b = xr[i];
    n += bits2f<BF16>(b) > xt;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) sm.wu[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    uint32_t s = 0;
    for (int w = 0; w < WAVES; ++w) s += sm.wu[w];
    rank[row] = (int32_t)s;
  }
}

template <bool BF16>
hipError_t score_rows(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_targets, float* nll, int32_t* rank,
                      double* lse_out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || !d_targets || !nll || rows > 65535 || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab) return hipErrorInvalidValue;
  if (vocab <= CACHE)
    hipLaunchKernelGGL((score_rows_kernel<BF16, true>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_targets, nll, rank, lse_out);
  else
    hipLaunchKernelGGL((score_rows_kernel<BF16, false>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_targets, nll, rank, lse_out);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_score_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_targets, float* nll,
                                int32_t* rank, double* lse_out, hipStream_t s) {
  return score_rows<false>(x, rows, vocab, ld, d_targets, nll, rank, lse_out, s);
}

hipError_t vstar_score_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* d_targets, float* nll,
                                 int32_t* rank, double* lse_out, hipStream_t s) {
  return score_rows<true>(x, rows, vocab, ld, d_targets, nll, rank, lse_out, s);
}

const char* vstar_score_check(int rows, int vocab, const int32_t* targets) {
  if (rows <= 0 || !targets) return "score: no rows / targets";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "score: vocabulary size out of range [1, 2^22]";
  for (int r = 0; r < rows; ++r)
    if (targets[r] < 0 || targets[r] >= vocab) return "score: a target id is outside [0, vocab)";
  return nullptr;
}
