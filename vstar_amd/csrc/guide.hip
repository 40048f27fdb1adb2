// guide.hip — the guidance stage of the language-model decode: classifier-free guidance / visual contrastive decoding of one logits
// row against another, g = gamma * (log_softmax(x_c) - log_softmax(x_u)) + log_softmax(x_u), on rows that never leave the device.
// DESIGN.md §8.12; the arguments and the semantics are documented at the launchers (guide.hpp).
//
// One workgroup (16 waves) per pair, pairs independent:
//   lse    rowlse::row_lse of the conditional and of the negative row (row_lse.hpp: the bits of the scoring / beam tails)
//   max    the conditional row's maximum once more, only when the pair has a plausibility cut
//   g      per element in double, every operation rounded on its own, ONE rounding to the storage type (round to odd to fp32, then
//          to nearest even, as beam.hip rounds lp), written over the conditional row
// Rows of up to CACHE elements keep the raw bits of BOTH rows in LDS after the first read (2 x 64 KiB); longer rows re-read the
// logits from L2.  Every element of the conditional row is read and written by the same thread, and only after both log-sum-exps.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include <vector>
#include "guide.hpp"
#include "row_lse.hpp"

namespace {

using rowlse::bits2f;
using rowlse::CACHE;
using rowlse::THREADS;
using rowlse::WAVES;
constexpr int MAX_VOCAB = 1 << 22;

template <bool CACHED>
struct GuideSmem {
  uint16_t bc[CACHED ? CACHE : 1];     // raw bits of the conditional row
  uint16_t bu[CACHED ? CACHE : 1];     // raw bits of the negative row
  float wf[WAVES];
  double wd[WAVES];
};
// one row's view of the shared memory for rowlse's helpers, which use the members bits / wf / wd by name
struct RowView {
  uint16_t* bits;
  float* wf;
  double* wd;
};

template <bool BF16> __device__ __forceinline__ uint32_t f2bits(float f) {     // round to nearest even (torch's cast)
  if constexpr (BF16) return __builtin_bit_cast(uint16_t, (__bf16)f);
  else return __builtin_bit_cast(uint16_t, (_Float16)f);
}
// double -> float rounded to odd (beam.hip): rounding that float to nearest-even in 16 bits equals ONE correct rounding of the double
__device__ __forceinline__ float f64_to_f32_odd(double d) {
  const float f = (float)d;
  const double df = (double)f;
  if (df == d || d != d) return f;
  uint32_t b = __float_as_uint(f);
  if (fabs(df) > fabs(d)) b -= 1;                  // rounded away from zero (or to inf): step back toward zero (same sign)
  return __uint_as_float(b | 1u);
}
// a FINITE double rounded once to the storage type; beyond its range: the largest finite magnitude
template <bool BF16> __device__ __forceinline__ uint16_t round_sat(double v) {
  constexpr uint32_t INF = BF16 ? 0x7f80u : 0x7c00u;
  uint32_t b = f2bits<BF16>(f64_to_f32_odd(v));
  if ((b & 0x7fffu) == INF) b -= 1;
  return (uint16_t)b;
}

template <bool BF16, bool CACHED>
__global__ __launch_bounds__(THREADS) void guide_rows_kernel(uint16_t* x, int vocab, int64_t ld, const int32_t* __restrict__ cond_row,
                                                             const int32_t* __restrict__ neg_row, const float* __restrict__ scale,
                                                             const float* __restrict__ log_beta) {
  __shared__ GuideSmem<CACHED> sm;
  constexpr uint16_t NEG_INF = BF16 ? 0xff80u : 0xfc00u;
  const int p = blockIdx.x, tid = threadIdx.x;
  uint16_t* xc = x + (int64_t)cond_row[p] * ld;
  const uint16_t* xu = x + (int64_t)neg_row[p] * ld;
  const double gamma = (double)scale[p];
  const float lb = log_beta[p];
  RowView vc{sm.bc, sm.wf, sm.wd}, vu{sm.bu, sm.wf, sm.wd};
  const double lse_c = rowlse::row_lse<BF16, CACHED>(vc, xc, vocab);
  const double lse_u = rowlse::row_lse<BF16, CACHED>(vu, xu, vocab);
  auto raw_c = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.bc[i];
    else return xc[i];
  };
  auto raw_u = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.bu[i];
    else return xu[i];
  };
  const bool cut = lb > -INFINITY;                   // (uniform over the workgroup: the barriers of block_max are safe)
  float mx = -INFINITY;
  if (cut) {
    for (int i = tid; i < vocab; i += THREADS) mx = fmaxf(mx, bits2f<BF16>(raw_c(i)));
    mx = rowlse::block_max(vc, mx);
  }
  const bool dead = !(fabs(lse_c) < INFINITY) || !(fabs(lse_u) < INFINITY);      // a non-finite log-sum-exp: the row is -inf
  for (int i = tid; i < vocab; i += THREADS) {
    const float fc = bits2f<BF16>(raw_c(i));
    uint16_t out = NEG_INF;
    if (!dead && fabsf(fc) < INFINITY && !(cut && !(fc - mx >= lb))) {
      const double c = __dsub_rn((double)fc, lse_c);
      const float fu = bits2f<BF16>(raw_u(i));
      double g = c;                                  // a non-finite negative operand: nothing to contrast against
      if (fabsf(fu) < INFINITY) {
        const double u = __dsub_rn((double)fu, lse_u);
        g = __dadd_rn(__dmul_rn(gamma, __dsub_rn(c, u)), u);
      }
      out = round_sat<BF16>(g);
    }
    xc[i] = out;
  }
}

template <bool BF16>
hipError_t guide_rows(uint16_t* x, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row, const int32_t* neg_row, const float* scale,
                      const float* log_beta, hipStream_t s) {
  if (n_pairs <= 0) return hipSuccess;
  if (!x || ((uintptr_t)x & 1) || !cond_row || !neg_row || !scale || !log_beta || n_pairs > 65535 || vocab <= 0 || vocab > MAX_VOCAB ||
      ld < vocab)
    return hipErrorInvalidValue;
  if (vocab <= CACHE)
    hipLaunchKernelGGL((guide_rows_kernel<BF16, true>), dim3(n_pairs), dim3(THREADS), 0, s, x, vocab, ld, cond_row, neg_row, scale, log_beta);
  else
    hipLaunchKernelGGL((guide_rows_kernel<BF16, false>), dim3(n_pairs), dim3(THREADS), 0, s, x, vocab, ld, cond_row, neg_row, scale, log_beta);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_guide_rows_f16(uint16_t* x, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row, const int32_t* neg_row,
                                const float* scale, const float* log_beta, hipStream_t s) {
  return guide_rows<false>(x, vocab, ld, n_pairs, cond_row, neg_row, scale, log_beta, s);
}

hipError_t vstar_guide_rows_bf16(uint16_t* x, int vocab, int64_t ld, int n_pairs, const int32_t* cond_row, const int32_t* neg_row,
                                 const float* scale, const float* log_beta, hipStream_t s) {
  return guide_rows<true>(x, vocab, ld, n_pairs, cond_row, neg_row, scale, log_beta, s);
}

const char* vstar_guide_check(int rows, int vocab, int n_pairs, const int32_t* cond_row, const int32_t* neg_row, const float* scale,
                              const float* log_beta) {
  if (rows <= 0 || n_pairs <= 0 || n_pairs > 65535 || !cond_row || !neg_row || !scale || !log_beta) return "guide: no rows / pairs / records";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "guide: vocabulary size out of range [1, 2^22]";
  for (int p = 0; p < n_pairs; ++p) {
    if (cond_row[p] == neg_row[p]) return "guide: cond_row and neg_row of a pair must differ";
    if (cond_row[p] < 0 || cond_row[p] >= rows || neg_row[p] < 0 || neg_row[p] >= rows) return "guide: a row is outside [0, rows)";
  }
  std::vector<char> seen((size_t)rows, 0);
  for (int p = 0; p < n_pairs; ++p)
    if (seen[(size_t)cond_row[p]]++ || seen[(size_t)neg_row[p]]++) return "guide: a row appears in two records";
  for (int p = 0; p < n_pairs; ++p) {
    if (!std::isfinite(scale[p]) || scale[p] < 0.f) return "guide: the guidance scale must be finite and >= 0";
    if (!(log_beta[p] <= 0.f)) return "guide: log_beta must be <= 0 (-inf = no plausibility cut) and not NaN";
  }
  return nullptr;
}
