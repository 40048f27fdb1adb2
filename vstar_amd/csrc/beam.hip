// beam.hip — the beam-search tail of the language-model decode: HF 4.31 beam_search's candidate selection
// (log_softmax -> + beam score -> topk(2k) over k x V) on logits rows that never leave the device.  DESIGN.md §8.2.
//
// Two launches:
//   row kernel    one workgroup (16 waves) per row:
//                   lse   max, then sum exp(x - max) in double (deterministic: fixed per-thread order, fixed reduction order)
//                   lp    (x - lse) rounded to the storage type (torch: fp32 log_softmax of the half logits, cast back), mapped
//                         to order-preserving 16-bit keys (NaN -> -inf, -0 -> +0)
//                   s_T   count-weighted radix select over the two key bytes (LDS histograms): the n-th largest key K_T; since
//                         s = score + lp is monotone in lp, s_T = score + lp(K_T) is the n-th largest s
//                   pick  every i with s_i > s_T, then the lowest-index ties at s_T — an exact scan in index order over thread-
//                         contiguous chunks (the fp32 add can collapse DIFFERENT lp onto one s, so ties are resolved on s)
//                 -> n = min(n_cand, vocab) (s, token) pairs per row, unordered, in the workspace
//   merge kernel  one workgroup per group: the rank of each of its <= 16 x 32 row candidates under (s desc, flat index asc),
//                 flat = row_in_group * vocab + token; ranks < n_cand are written in rank order.
// Rows of up to CACHE elements keep their bits / keys in LDS after the first read; longer rows re-read the logits from L2.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "beam.hpp"
#include "row_lse.hpp"
#include "row_select.hpp"

namespace {

using rowlse::bits2f;
using rowlse::CACHE;                   // rows up to this length stay in LDS (64 KiB)
using rowlse::THREADS;
using rowlse::WAVES;
using rowsel::block_scan;
using rowsel::select_bin;
constexpr int MAX_VOCAB = 1 << 22;
constexpr int MERGE_THREADS = VSTAR_BEAM_MAX_K * VSTAR_BEAM_MAX_CAND;

template <bool CACHED>
struct BeamSmem {
  uint16_t bits[CACHED ? CACHE : 1];   // raw logits bits, then (in place) the lp keys
  uint32_t hist[256];
  float wf[WAVES];
  double wd[WAVES];
  uint32_t wu[WAVES];
  int sel;
  uint32_t sel_above;
};

template <bool BF16> __device__ __forceinline__ uint32_t f2bits(float f) {     // round to nearest even (torch's cast)
  if constexpr (BF16) return __builtin_bit_cast(uint16_t, (__bf16)f);
  else return __builtin_bit_cast(uint16_t, (_Float16)f);
}
// double -> float rounded to odd (truncate, then set the last bit if inexact): rounding that float to nearest-even in 16 bits
// (11 or 8 significant bits, <= 24 - 2) equals ONE correct rounding of the double to 16 bits — no double rounding
__device__ __forceinline__ float f64_to_f32_odd(double d) {
  const float f = (float)d;
  const double df = (double)f;
  if (df == d || d != d) return f;
  uint32_t b = __float_as_uint(f);
  if (fabs(df) > fabs(d)) b -= 1;                  // rounded away from zero: step back toward zero (same sign)
  return __uint_as_float(b | 1u);
}
// lp key of logit bits x: order-preserving 16-bit key of (x - lse) rounded once to the storage type, NaN -> -inf, -0 -> +0
template <bool BF16> __device__ __forceinline__ uint32_t lp_key(uint32_t x, double lse) {
  constexpr uint32_t NEG_INF = BF16 ? 0xff80u : 0xfc00u;
  uint32_t b = f2bits<BF16>(f64_to_f32_odd((double)bits2f<BF16>(x) - lse));
  if ((b & 0x7fffu) > (NEG_INF & 0x7fffu)) b = NEG_INF;
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
template <bool BF16> __device__ __forceinline__ float key_lp(uint32_t key) {
  return bits2f<BF16>((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu));
}

template <bool BF16, bool CACHED>
__global__ __launch_bounds__(THREADS) void beam_rows_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                            const float* __restrict__ scores, int n_cand, float* __restrict__ ws_s,
                                                            int32_t* __restrict__ ws_t, float* __restrict__ lp_out) {
  __shared__ BeamSmem<CACHED> sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xr = x + (int64_t)row * ld;
  const float bs = scores[row];
  const uint32_t n_row = (uint32_t)(n_cand < vocab ? n_cand : vocab);
  if (tid < 256) sm.hist[tid] = 0;
  // ---- max (and the row into LDS), log-sum-exp in double: row_lse.hpp, shared with the scoring tail ----
  const double lse = rowlse::row_lse<BF16, CACHED>(sm, xr, vocab);
  auto raw = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.bits[i];
    else return xr[i];
  };
  // ---- lp keys (in place in LDS: each thread rewrites the elements it read), the high-byte histogram ----
  for (int i = tid; i < vocab; i += THREADS) {
    const uint32_t key = lp_key<BF16>(raw(i), lse);
    if constexpr (CACHED) sm.bits[i] = (uint16_t)key;
    if (lp_out) lp_out[(int64_t)row * vocab + i] = key_lp<BF16>(key);
    atomicAdd(&sm.hist[key >> 8], 1u);
  }
  auto key_at = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.bits[i];
    else return lp_key<BF16>(xr[i], lse);
  };
  // ---- K_T: the n_row-th largest key (both bins exist: n_row <= vocab) ----
  int hb, lb;
  uint32_t above, a2;
  select_bin(sm, n_row, hb, above);                  // (synchronises: the cached keys are visible from here on)
  for (int i = tid; i < vocab; i += THREADS) {
    const uint32_t key = key_at(i);
    if ((int)(key >> 8) == hb) atomicAdd(&sm.hist[key & 255u], 1u);
  }
  select_bin(sm, n_row - above, lb, a2);
  const uint32_t kt = ((uint32_t)hb << 8) | (uint32_t)lb;
  const float st = bs + key_lp<BF16>(kt);
  // ---- pick: s > s_T, then the lowest-index ties at s_T, in index order over thread-contiguous chunks ----
  const int C = (vocab + THREADS - 1) / THREADS;
  const int c0 = tid * C < vocab ? tid * C : vocab, c1 = c0 + C < vocab ? c0 + C : vocab;
  uint32_t n_gt = 0, n_eq = 0;
  for (int i = c0; i < c1; ++i) {
    const float s = bs + key_lp<BF16>(key_at(i));
    n_gt += s > st;
    n_eq += s == st;
  }
  uint32_t gt_excl, gt_tot, eq_excl, eq_tot;
  block_scan(sm, n_gt, gt_excl, gt_tot);
  block_scan(sm, n_eq, eq_excl, eq_tot);
  const uint32_t need_eq = n_row - gt_tot;           // gt_tot < n_row <= gt_tot + eq_tot
  if (n_gt || (n_eq && eq_excl < need_eq)) {
    uint32_t pg = gt_excl, pe = eq_excl;
    float* os = ws_s + (int64_t)row * n_cand;
    int32_t* ot = ws_t + (int64_t)row * n_cand;
    for (int i = c0; i < c1; ++i) {
      const float s = bs + key_lp<BF16>(key_at(i));
      if (s > st) { os[pg] = s; ot[pg] = i; ++pg; }
      else if (s == st && pe < need_eq) { os[gt_tot + pe] = s; ot[gt_tot + pe] = i; ++pe; }
    }
  }
}

__global__ __launch_bounds__(MERGE_THREADS) void beam_merge_kernel(const float* __restrict__ ws_s, const int32_t* __restrict__ ws_t,
                                                                   const int32_t* __restrict__ goff, int vocab, int n_cand,
                                                                   float* __restrict__ cand_s, int32_t* __restrict__ cand_tok,
                                                                   int32_t* __restrict__ cand_row) {
  __shared__ float cs[MERGE_THREADS];
  __shared__ int32_t cf[MERGE_THREADS];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int r0 = goff[g], nr = goff[g + 1] - r0;
  const int n_row = n_cand < vocab ? n_cand : vocab, total = nr * n_row;
  float si = 0.f;
  int32_t fi = 0;
  if (tid < total) {
    const int r = tid / n_row, p = tid - r * n_row;
    const int64_t w = (int64_t)(r0 + r) * n_cand + p;
    si = ws_s[w];
    fi = r * vocab + ws_t[w];
    cs[tid] = si;
    cf[tid] = fi;
  }
  __syncthreads();
  if (tid >= total) return;
  int rank = 0;
  for (int j = 0; j < total; ++j) {
    const float sj = cs[j];
    rank += (sj > si) || (sj == si && cf[j] < fi);
  }
  if (rank < n_cand) {
    const int64_t o = (int64_t)g * n_cand + rank;
    cand_s[o] = si;
    cand_tok[o] = fi % vocab;
    cand_row[o] = fi / vocab;
  }
}

template <bool BF16>
hipError_t beam_select(const uint16_t* x, int rows, int vocab, int64_t ld, const float* d_scores, int n_groups, const int32_t* d_goff,
                       int n_cand, void* ws, float* cand_s, int32_t* cand_tok, int32_t* cand_row, float* lp_out, hipStream_t s) {
  if (rows <= 0 || n_groups <= 0) return hipSuccess;
  if (!x || !d_scores || !d_goff || !ws || !cand_s || !cand_tok || !cand_row || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab ||
      n_cand <= 0 || n_cand > VSTAR_BEAM_MAX_CAND)
    return hipErrorInvalidValue;
  float* ws_s = (float*)ws;
  int32_t* ws_t = (int32_t*)(ws_s + (size_t)rows * n_cand);
  if (vocab <= CACHE)
    hipLaunchKernelGGL((beam_rows_kernel<BF16, true>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_scores, n_cand, ws_s, ws_t, lp_out);
  else
    hipLaunchKernelGGL((beam_rows_kernel<BF16, false>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_scores, n_cand, ws_s, ws_t, lp_out);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(n_groups), dim3(MERGE_THREADS), 0, s, ws_s, ws_t, d_goff, vocab, n_cand, cand_s, cand_tok,
                     cand_row);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_beam_select_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const float* d_scores, int n_groups,
                                 const int32_t* d_goff, int n_cand, void* ws, float* cand_s, int32_t* cand_tok, int32_t* cand_row,
                                 float* lp_out, hipStream_t s) {
  return beam_select<false>(x, rows, vocab, ld, d_scores, n_groups, d_goff, n_cand, ws, cand_s, cand_tok, cand_row, lp_out, s);
}

hipError_t vstar_beam_select_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const float* d_scores, int n_groups,
                                  const int32_t* d_goff, int n_cand, void* ws, float* cand_s, int32_t* cand_tok, int32_t* cand_row,
                                  float* lp_out, hipStream_t s) {
  return beam_select<true>(x, rows, vocab, ld, d_scores, n_groups, d_goff, n_cand, ws, cand_s, cand_tok, cand_row, lp_out, s);
}

size_t vstar_beam_ws_bytes(int rows, int n_cand) { return (size_t)rows * n_cand * 8 + 256; }

const char* vstar_beam_check(int rows, int vocab, const float* scores, int n_groups, const int32_t* goff, int n_cand) {
  if (rows <= 0 || n_groups <= 0 || n_groups > rows || !scores || !goff) return "beam select: no rows / groups";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "beam select: vocabulary size out of range [1, 2^22]";
  if (n_cand <= 0 || n_cand > VSTAR_BEAM_MAX_CAND) return "beam select: n_cand out of range [1, 32]";
  if (goff[0] != 0 || goff[n_groups] != rows) return "beam select: group offsets must run from 0 to the row count";
  for (int g = 0; g < n_groups; ++g) {
    const int nr = goff[g + 1] - goff[g];
    if (nr < 1 || nr > VSTAR_BEAM_MAX_K) return "beam select: a group must have 1 .. 16 rows";
    if ((int64_t)nr * vocab < n_cand) return "beam select: n_cand exceeds the candidates of a group (rows x vocab)";
  }
  for (int r = 0; r < rows; ++r)
    if (std::isnan(scores[r]) || scores[r] == INFINITY) return "beam select: a beam score is NaN or +inf";
  return nullptr;
}
