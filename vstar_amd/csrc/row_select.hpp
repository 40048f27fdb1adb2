// row_select.hpp — the workgroup helpers of the radix selects over one logits row (beam.hip, logprob.hip, contrast.hip): an
// exclusive scan in thread order, the search of a 256-bin LDS histogram for the bin that holds the n-th largest key, and the top-n
// select built on them.  One workgroup of rowlse::THREADS threads; the shared-memory struct is a template parameter and is used by
// member name (hist[256], wu[WAVES], sel, sel_above; the top-n select also pick_key[], pick_idx[]).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "row_lse.hpp"

namespace rowsel {

using rowlse::WAVES;

// exclusive prefix of v in thread order, and the block total
template <typename Sm> __device__ __forceinline__ void block_scan(Sm& sm, uint32_t v, uint32_t& excl, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const uint32_t n = __shfl_up(inc, o, 64); if (lane >= o) inc += n; }
  if (lane == 63) sm.wu[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
  for (int w = 0; w < WAVES; ++w) { const uint32_t x = sm.wu[w]; base += w < wave ? x : 0; tot += x; }
  __syncthreads();
  excl = base + inc - v;
  total = tot;
}

// The bin b of sm.hist with above(b) < need <= above(b) + hist[b] (above(b) = the count in the bins > b).  Wave 0 scans;
// the histogram is cleared for the next select.
template <typename Sm> __device__ __forceinline__ void select_bin(Sm& sm, uint32_t need, int& bin, uint32_t& above) {
  __syncthreads();                                   // histogram complete
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    uint32_t h[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { h[j] = sm.hist[4 * l + j]; s += h[j]; }
    uint32_t suf = s;                                // sum over lanes >= l
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t n = __shfl_down(suf, o, 64); if (l + o < 64) suf += n; }
    uint32_t a = suf - s;
    int found = -1;
    uint32_t fa = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      if (a < need && need <= a + h[j]) { found = 4 * l + j; fa = a; }
      a += h[j];
    }
    const uint64_t any = __ballot(found >= 0);
    if (found >= 0) { sm.sel = found; sm.sel_above = fa; }
    if (l == 0 && !any) sm.sel = -1;
  }
  __syncthreads();
  bin = sm.sel;
  above = sm.sel_above;
  __syncthreads();
  if (threadIdx.x < 256) sm.hist[threadIdx.x] = 0;
  __syncthreads();
}

// ---- the top-n select of one row (logprob.hip, contrast.hip): one body, so both give the same picks ----
// order-preserving 16-bit key of the VALUE of logit bits b: NaN -> -inf, -0 -> +0
template <bool BF16> __device__ __forceinline__ uint32_t value_key(uint32_t b) {
  constexpr uint32_t NEG_INF = BF16 ? 0xff80u : 0xfc00u;
  if ((b & 0x7fffu) > (NEG_INF & 0x7fffu)) b = NEG_INF;
  if (b == 0x8000u) b = 0;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}

// The n (1 <= n <= vocab, n <= the capacity of sm.pick_key / sm.pick_idx) largest elements of the row raw(0 .. vocab) under (value
// descending, index ascending), unsorted, into sm.pick_key / sm.pick_idx [0, n).  On entry sm.hist holds the histogram of the HIGH
// key bytes of the row (the caller's first pass fills it, next to whatever else it counts there).  K_T, the n-th largest key, by a
// radix select over the two key bytes; then every i with key > K_T and the lowest-index ties at K_T, an exact scan in index order
// over thread-contiguous chunks.  Synchronises: the picks are visible to every thread on return.
template <bool BF16, typename Sm, typename Raw>
__device__ __forceinline__ void pick_top(Sm& sm, Raw raw, int vocab, uint32_t n) {
  constexpr int THREADS = rowlse::THREADS;
  const int tid = threadIdx.x;
  int hb, lb;
  uint32_t above, a2;
  select_bin(sm, n, hb, above);
  for (int i = tid; i < vocab; i += THREADS) {
    const uint32_t key = value_key<BF16>(raw(i));
    if ((int)(key >> 8) == hb) atomicAdd(&sm.hist[key & 255u], 1u);
  }
  select_bin(sm, n - above, lb, a2);
  const uint32_t kt = ((uint32_t)hb << 8) | (uint32_t)lb;
  const int C = (vocab + THREADS - 1) / THREADS;
  const int c0 = tid * C < vocab ? tid * C : vocab, c1 = c0 + C < vocab ? c0 + C : vocab;
  uint32_t n_gt = 0, n_eq = 0;
  for (int i = c0; i < c1; ++i) {
    const uint32_t key = value_key<BF16>(raw(i));
    n_gt += key > kt;
    n_eq += key == kt;
  }
  uint32_t gt_excl, gt_tot, eq_excl, eq_tot;
  block_scan(sm, n_gt, gt_excl, gt_tot);
  block_scan(sm, n_eq, eq_excl, eq_tot);
  const uint32_t need_eq = n - gt_tot;               // gt_tot < n <= gt_tot + eq_tot
  if (n_gt || (n_eq && eq_excl < need_eq)) {
    uint32_t pg = gt_excl, pe = eq_excl;
    for (int i = c0; i < c1; ++i) {
      const uint32_t key = value_key<BF16>(raw(i));
      if (key > kt) { sm.pick_key[pg] = key; sm.pick_idx[pg] = i; ++pg; }
      else if (key == kt && pe < need_eq) { sm.pick_key[gt_tot + pe] = key; sm.pick_idx[gt_tot + pe] = i; ++pe; }
    }
  }
  __syncthreads();
}

// the rank of pick j among the n picks under (key descending, index ascending): the position it is written at
template <typename Sm> __device__ __forceinline__ uint32_t pick_rank(const Sm& sm, uint32_t n, uint32_t j) {
  const uint32_t ki = sm.pick_key[j];
  const int32_t ii = sm.pick_idx[j];
  uint32_t r = 0;
  for (uint32_t q = 0; q < n; ++q) {
    const uint32_t kq = sm.pick_key[q];
    r += (kq > ki) || (kq == ki && sm.pick_idx[q] < ii);
  }
  return r;
}

}  // namespace rowsel
