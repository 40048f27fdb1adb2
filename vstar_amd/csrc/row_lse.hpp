// row_lse.hpp — the log-sum-exp of one logits row by one workgroup of 16 waves, shared by the tails that need it (beam.hip,
// score.hip) so that both compute the same bits: max, then sum exp(x - max) in double with a fixed per-thread order (elements
// tid, tid + 1024, ...) and a fixed reduction order (butterfly inside a wave, then the waves in index order).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rowlse {

constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int CACHE = 32768;           // rows up to this length stay in LDS (64 KiB)

// Reduction scratch of a workgroup.  The helpers below are templates over the shared-memory struct and use its members wf / wd
// (and `bits[]` when the row is cached) by name: score.hip's struct derives from Scratch, beam.hip's BeamSmem declares the same
// members itself next to its histogram.
struct Scratch {
  float wf[WAVES];
  double wd[WAVES];
  uint32_t wu[WAVES];
};

template <bool BF16> __device__ __forceinline__ float bits2f(uint32_t b) {
  if constexpr (BF16) return __uint_as_float(b << 16);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
}

template <typename Sm> __device__ __forceinline__ float block_max(Sm& sm, float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) sm.wf[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = sm.wf[0];
  for (int w = 1; w < WAVES; ++w) m = fmaxf(m, sm.wf[w]);
  __syncthreads();
  return m;
}

// sum in a fixed order: lane 0's butterfly result per wave, then the waves in index order (every thread gets the same bits)
template <typename Sm> __device__ __forceinline__ double block_sum(Sm& sm, double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sm.wd[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < WAVES; ++w) s += sm.wd[w];
  __syncthreads();
  return s;
}

// lse = max + log(sum exp(x_i - max)) of the row xr[0 .. vocab), every thread of the workgroup gets the same double.  CACHED: the
// raw 16-bit elements are left in sm.bits[0 .. vocab) (visible to every thread on return); otherwise the row is read twice.
// fmaxf skips NaN, so a NaN element reaches the sum and the result is NaN; a row whose maximum is +-inf gives NaN (inf - inf).
template <bool BF16, bool CACHED, typename Sm>
__device__ __forceinline__ double row_lse(Sm& sm, const uint16_t* __restrict__ xr, int vocab) {
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  for (int i = tid; i < vocab; i += THREADS) {
    const uint16_t b = xr[i];
    if constexpr (CACHED) sm.bits[i] = b;
    mx = fmaxf(mx, bits2f<BF16>(b));
  }
  mx = block_max(sm, mx);                            // (synchronises: the cached bits are visible from here on)
  double se = 0.0;
  const double dmx = (double)mx;
  for (int i = tid; i < vocab; i += THREADS) {
    uint32_t b;
    if constexpr (CACHED) b = sm.bits[i];
    else b = xr[i];
    se += exp((double)bits2f<BF16>(b) - dmx);
  }
  return dmx + log(block_sum(sm, se));
}

}  // namespace rowlse
