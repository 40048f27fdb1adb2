// sample.hip — the sampling tail of the language-model decode: HF 4.31 generate(do_sample=True) (TemperatureLogitsWarper ->
// TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial) on logits rows that never leave the device.  DESIGN.md §8.
//
// One workgroup (16 waves) per row, every row with its own vstar_vqa_sampling record:
//   scores   s_i = lp(float(x_i) / t), rounded to the storage type like torch's `half_tensor / t`; mapped to order-preserving
//            16-bit keys (NaN -> -inf, -0 -> +0), so "s_i >= s_j" is "key_i >= key_j"
//   masses   m_i = round(exp(s_i - max s) * 2^40), unsigned 64-bit fixed point (the maximal score has exactly 2^40): every sum
//            below is an exact integer sum, so the result is independent of the summation order — deterministic without a
//            fixed reduction tree, and a row's draw depends on that row alone
//   top-k    count-weighted radix select over the two key bytes (LDS histograms, integer atomics): the k-th largest key Tk;
//            kept = key >= Tk (every tie at the k-th value is kept)
//   top-p    the same select weighted by mass over the keys >= Tk: the smallest key Tp whose strictly-greater mass is
//            < top_p * Z_k; kept = key >= max(Tk, Tp) (the maximal score is always kept, so top_p = 0 keeps its ties)
//   draw     u = (philox4x32_10(ctr = (step, stream lo, stream hi, 0), key = (seed lo, seed hi)).x >> 8) * 2^-24; thread-
//            contiguous chunks of the row, an exact exclusive scan of their kept masses, and the thread whose chunk holds
//            floor(u * Z) walks it: the token is the smallest kept index whose inclusive prefix mass exceeds floor(u * Z)
// Rows of up to CACHE elements keep their keys in LDS after the first read (32001 at 7B: one HBM/L2 read per row); longer rows
// re-read the logits from L2 in every pass.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "sample.hpp"

namespace {

typedef unsigned long long u64;
constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int CACHE = 32768;           // keys of rows up to this length stay in LDS (64 KiB)
constexpr int UNROLL = 8;              // independent global loads in flight per thread in the streaming passes
constexpr int MAX_VOCAB = 1 << 22;     // keeps the fixed-point total mass below 2^62

template <bool CACHED>
struct SampleSmem {
  uint16_t keys[CACHED ? CACHE : 1];
  u64 hist[256];
  u64 wtot[WAVES];
  uint32_t wmax[WAVES];
  u64 sel_above, sel_need;
  int sel;
  uint32_t u24;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const u64 p0 = (u64)0xD2511F53u * c[0], p1 = (u64)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[1] = (uint32_t)p1;
    c[3] = (uint32_t)p0;
    c[0] = n0;
    c[2] = n2;
  }
}

template <bool BF16> __device__ __forceinline__ float bits2f(uint32_t b) {
  if constexpr (BF16) return __uint_as_float(b << 16);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
}
template <bool BF16> __device__ __forceinline__ uint32_t f2bits(float f) {     // round to nearest even (torch's cast)
  if constexpr (BF16) return __builtin_bit_cast(uint16_t, (__bf16)f);
  else return __builtin_bit_cast(uint16_t, (_Float16)f);
}

template <bool BF16> __device__ __forceinline__ uint32_t score_key(uint16_t x, float t) {
  constexpr uint32_t NEG_INF = BF16 ? 0xff80u : 0xfc00u;
  uint32_t b = t == 1.f ? x : f2bits<BF16>(bits2f<BF16>(x) / t);
  if ((b & 0x7fffu) > (NEG_INF & 0x7fffu)) b = NEG_INF;          // NaN -> -inf
  if (b == 0x8000u) b = 0;                                       // -0 -> +0 (equal scores, equal keys)
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
template <bool BF16> __device__ __forceinline__ float key_score(uint32_t key) {
  return bits2f<BF16>((key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu));
}
// exp(s - smax) in 2^-40 units; the maximal key has exactly 2^40 (also when the maximum is +-inf)
template <bool BF16> __device__ __forceinline__ u64 key_mass(uint32_t key, uint32_t kmax, float smax) {
  if (key == kmax) return 1ull << 40;
  return (u64)__builtin_rintf(expf(key_score<BF16>(key) - smax) * 0x1p40f);
}

// f(i, key) for every element of the row, read from global memory (UNROLL loads in flight)
template <bool BF16, typename F>
__device__ __forceinline__ void stream_keys(const uint16_t* __restrict__ xr, int vocab, float t, F&& f) {
  for (int i0 = threadIdx.x; i0 < vocab; i0 += THREADS * UNROLL) {
    uint16_t v[UNROLL];
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) { const int i = i0 + j * THREADS; v[j] = i < vocab ? xr[i] : (uint16_t)0; }
#pragma unroll
    for (int j = 0; j < UNROLL; ++j) { const int i = i0 + j * THREADS; if (i < vocab) f(i, score_key<BF16>(v[j], t)); }
  }
}

template <typename Sm> __device__ __forceinline__ void clear_hist(Sm& sm) {
  if (threadIdx.x < 256) sm.hist[threadIdx.x] = 0;
  __syncthreads();
}

template <typename Sm> __device__ __forceinline__ uint32_t block_max(Sm& sm, uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
  if ((threadIdx.x & 63) == 0) sm.wmax[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = 0;
  for (int w = 0; w < WAVES; ++w) m = sm.wmax[w] > m ? sm.wmax[w] : m;
  __syncthreads();
  return m;
}

// exclusive prefix of v in thread order, and the block total (exact: integers)
template <typename Sm> __device__ __forceinline__ void block_scan(Sm& sm, u64 v, u64& excl, u64& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const u64 n = __shfl_up(inc, o, 64); if (lane >= o) inc += n; }
  if (lane == 63) sm.wtot[wave] = inc;
  __syncthreads();
  u64 base = 0, tot = 0;
  for (int w = 0; w < WAVES; ++w) { const u64 x = sm.wtot[w]; base += w < wave ? x : 0; tot += x; }
  __syncthreads();
  excl = base + inc - v;
  total = tot;
}

// The bin b of sm.hist with above(b) < need <= above(b) + hist[b], above(b) = the sum over the bins > b; bin = -1 if there is
// none.  frac >= 0 replaces `need` by ceil(frac * the histogram total).  Wave 0 scans; everyone gets the result.
template <typename Sm>
__device__ __forceinline__ void select_bin(Sm& sm, u64 need, float frac, int& bin, u64& above, u64& need_out) {
  __syncthreads();                                   // histogram complete
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    u64 h[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { h[j] = sm.hist[4 * l + j]; s += h[j]; }
    u64 suf = s;                                     // sum over lanes >= l
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u64 n = __shfl_down(suf, o, 64); if (l + o < 64) suf += n; }
    if (frac >= 0.f) need = (u64)ceil((double)frac * (double)__shfl(suf, 0, 64));
    u64 a = suf - s, fa = 0;
    int found = -1;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
      if (a < need && need <= a + h[j]) { found = 4 * l + j; fa = a; }
      a += h[j];
    }
    const u64 any = __ballot(found >= 0);
    if (found >= 0) { sm.sel = found; sm.sel_above = fa; }
    if (l == 0) { sm.sel_need = need; if (!any) sm.sel = -1; }
  }
  __syncthreads();
  bin = sm.sel;
  above = sm.sel_above;
  need_out = sm.sel_need;
  __syncthreads();                                   // sel / hist free again
}

template <bool BF16, bool CACHED>
__global__ __launch_bounds__(THREADS) void sample_rows_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                              const vstar_vqa_sampling* __restrict__ params,
                                                              int32_t* __restrict__ tokens, float* __restrict__ u_out,
                                                              int32_t* __restrict__ n_kept) {
  __shared__ SampleSmem<CACHED> sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xr = x + (int64_t)row * ld;
  const vstar_vqa_sampling P = params[row];
  const float t = P.temperature;
  const int k = P.top_k > 0 ? (P.top_k < vocab ? P.top_k : vocab) : 0;
  if (tid < 256) sm.hist[tid] = 0;
  if (tid == 0) {
    uint32_t c[4] = {P.step, (uint32_t)P.stream, (uint32_t)(P.stream >> 32), 0u};
    philox4x32_10(c, (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
    sm.u24 = c[0] >> 8;
  }
  __syncthreads();
  // ---- pass 0: keys (into LDS), their maximum, the high-byte counts for top-k ----
  uint32_t kmax = 0;
  stream_keys<BF16>(xr, vocab, t, [&](int i, uint32_t key) {
    if constexpr (CACHED) sm.keys[i] = (uint16_t)key;
    kmax = key > kmax ? key : kmax;
    if (k) atomicAdd(&sm.hist[key >> 8], 1ull);
  });
  kmax = block_max(sm, kmax);                        // (synchronises: the cached keys are visible from here on)
  const float smax = key_score<BF16>(kmax);
  auto each = [&](auto&& f) {
    if constexpr (CACHED) {
      for (int i = tid; i < vocab; i += THREADS) f(i, (uint32_t)sm.keys[i]);
    } else {
      stream_keys<BF16>(xr, vocab, t, f);
    }
  };
  auto key_at = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.keys[i];
    else return score_key<BF16>(xr[i], t);
  };
  // ---- top-k: the k-th largest key ----
  uint32_t tk = 0;
  if (k) {
    int hb, lb;
    u64 above, a2, need;
    select_bin(sm, (u64)k, -1.f, hb, above, need);
    clear_hist(sm);
    each([&](int, uint32_t key) { if ((int)(key >> 8) == hb) atomicAdd(&sm.hist[key & 255u], 1ull); });
    select_bin(sm, (u64)k - above, -1.f, lb, a2, need);
    if (hb >= 0 && lb >= 0) tk = ((uint32_t)hb << 8) | (uint32_t)lb;
  }
  // ---- top-p over the keys >= tk: the smallest key whose strictly-greater mass is < top_p * Z_k ----
  uint32_t tkeep = tk;
  if (P.top_p < 1.f) {
    clear_hist(sm);
    each([&](int, uint32_t key) {
      if (key >= tk) { const u64 m = key_mass<BF16>(key, kmax, smax); if (m) atomicAdd(&sm.hist[key >> 8], m); }
    });
    int hb, lb;
    u64 above, a2, need, n2;
    select_bin(sm, 0, P.top_p, hb, above, need);     // need = ceil(top_p * Z_k); 0 (top_p = 0): no bin
    uint32_t tp = kmax;
    if (hb >= 0) {
      clear_hist(sm);
      each([&](int, uint32_t key) {
        if ((int)(key >> 8) == hb && key >= tk) { const u64 m = key_mass<BF16>(key, kmax, smax); if (m) atomicAdd(&sm.hist[key & 255u], m); }
      });
      select_bin(sm, need - above, -1.f, lb, a2, n2);
      if (lb >= 0) tp = ((uint32_t)hb << 8) | (uint32_t)lb;
    }
    tp = tp < kmax ? tp : kmax;
    tkeep = tp > tk ? tp : tk;
  }
  // ---- draw: inverse CDF in vocabulary order over the kept set ----
  const int C = (vocab + THREADS - 1) / THREADS;
  const int c0 = tid * C < vocab ? tid * C : vocab, c1 = c0 + C < vocab ? c0 + C : vocab;
  u64 msum = 0, cnt = 0;
  for (int i = c0; i < c1; ++i) {
    const uint32_t key = key_at(i);
    if (key >= tkeep) { msum += key_mass<BF16>(key, kmax, smax); ++cnt; }
  }
  u64 excl, Z, cexcl, ctot;
  block_scan(sm, msum, excl, Z);
  block_scan(sm, cnt, cexcl, ctot);
  const u64 u = sm.u24;
  const u64 target = (Z >> 24) * u + (((Z & 0xffffffull) * u) >> 24);     // floor(u * Z * 2^-24), exact
  if (excl <= target && target < excl + msum) {      // exactly one thread: the prefix masses tile [0, Z) and target < Z
    u64 acc = excl;
    for (int i = c0; i < c1; ++i) {
      const uint32_t key = key_at(i);
      if (key >= tkeep) {
        acc += key_mass<BF16>(key, kmax, smax);
        if (acc > target) { tokens[row] = i; break; }
      }
    }
  }
  if (tid == 0) {
    if (u_out) u_out[row] = (float)u * 0x1p-24f;
    if (n_kept) n_kept[row] = (int32_t)ctot;
  }
}

template <bool BF16>
hipError_t sample_rows(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params, int32_t* tokens,
                       float* u_out, int32_t* n_kept, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || !d_params || !tokens || rows > 65535 || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab) return hipErrorInvalidValue;
  if (vocab <= CACHE)
    hipLaunchKernelGGL((sample_rows_kernel<BF16, true>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_params, tokens, u_out, n_kept);
  else
    hipLaunchKernelGGL((sample_rows_kernel<BF16, false>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_params, tokens, u_out, n_kept);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_sample_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                 int32_t* tokens, float* u_out, int32_t* n_kept, hipStream_t s) {
  return sample_rows<false>(x, rows, vocab, ld, d_params, tokens, u_out, n_kept, s);
}

hipError_t vstar_sample_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                  int32_t* tokens, float* u_out, int32_t* n_kept, hipStream_t s) {
  return sample_rows<true>(x, rows, vocab, ld, d_params, tokens, u_out, n_kept, s);
}

bool vstar_sample_params_valid(const vstar_vqa_sampling& p) {
  return p.temperature > 0.f && std::isfinite(p.temperature) && p.top_k >= 0 && p.top_p >= 0.f;     // (NaN fails both)
}
