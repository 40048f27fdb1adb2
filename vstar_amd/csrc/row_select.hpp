// row_select.hpp — the two workgroup helpers of the radix selects over one logits row (beam.hip, logprob.hip): an exclusive scan
// in thread order and the search of a 256-bin LDS histogram for the bin that holds the n-th largest key.  One workgroup of
// rowlse::THREADS threads; the shared-memory struct is a template parameter and is used by member name (hist[256], wu[WAVES],
// sel, sel_above).  Device code only.
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

}  // namespace rowsel
