// sample_core.hpp — the row-level pieces of the sampling tail, shared by the tails that draw from a warped logits row (sample.hip,
// spec.hip) so that both build the same kept set, the same fixed-point masses and the same draw, bit for bit: the Philox stream,
// the order-preserving score keys, the 2^-40 masses, the count / mass weighted radix select (top-k, top-p), the four further
// warpers of DESIGN.md §8.10 (min-p, typical-p, epsilon, eta) and the exact block scan behind the inverse-CDF draw.  DESIGN.md §8.1
// (1)-(4).  Device code only; one workgroup of 16 waves per row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/vstar_vqa.h"

namespace samplecore {

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

// the 24-bit uniform of one draw: u = u24 * 2^-24, key (seed lo, seed hi), counter (step, stream lo, stream hi, 0)
__device__ __forceinline__ uint32_t philox_u24(uint64_t seed, uint64_t stream, uint32_t step) {
  uint32_t c[4] = {step, (uint32_t)stream, (uint32_t)(stream >> 32), 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return c[0] >> 8;
}

// floor(u24 * 2^-24 * Z), exact (Z < 2^62)
__device__ __forceinline__ u64 scale_u24(u64 Z, u64 u24) { return (Z >> 24) * u24 + (((Z & 0xffffffull) * u24) >> 24); }

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

// the block totals of an integer (exact) and of a double: per-thread value -> xor butterfly inside the wave (a + b == b + a: every
// lane holds the same bits) -> the 16 wave sums added in wave order by everyone.  A fixed order: the double is deterministic.
template <typename Sm> __device__ __forceinline__ void block_sums(Sm& sm, u64& z, double& a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { z += __shfl_xor(z, o, 64); a += __shfl_xor(a, o, 64); }
  u64 zt = 0;
  double at = 0.0;
  if ((threadIdx.x & 63) == 0) sm.wtot[threadIdx.x >> 6] = z;
  __syncthreads();
  for (int w = 0; w < WAVES; ++w) zt += sm.wtot[w];
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm.wtot[threadIdx.x >> 6] = (u64)__double_as_longlong(a);
  __syncthreads();
  for (int w = 0; w < WAVES; ++w) at += __longlong_as_double((long long)sm.wtot[w]);
  __syncthreads();
  z = zt;
  a = at;
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

// The warped row of one workgroup: after keep() every thread knows the key threshold of the kept set (kept = key >= tkeep), the
// maximal key and its score; the keys of a CACHED row sit in sm.keys.  The caller zeroes sm.hist[0 .. 256) and synchronises
// before keep() (sample.hip does it together with its Philox word).  WARP: the row may go on through warp() (§8.10), after which
// the kept set is the band tkeep <= key <= tcap; without it tcap is never read and the code is the §8.1 code.
template <bool BF16, bool CACHED, bool WARP = false>
struct WarpedRow {
  SampleSmem<CACHED>& sm;
  const uint16_t* __restrict__ xr;
  int vocab;
  float t;
  uint32_t kmax = 0, tkeep = 0, tcap = 0xffffu;
  float smax = 0.f;

  __device__ __forceinline__ WarpedRow(SampleSmem<CACHED>& sm_, const uint16_t* xr_, int vocab_, float t_)
      : sm(sm_), xr(xr_), vocab(vocab_), t(t_) {}

  __device__ __forceinline__ uint32_t key_at(int i) const {
    if constexpr (CACHED) return sm.keys[i];
    else return score_key<BF16>(xr[i], t);
  }
  template <typename F> __device__ __forceinline__ void each(F&& f) const {
    if constexpr (CACHED) {
      for (int i = threadIdx.x; i < vocab; i += THREADS) f(i, (uint32_t)sm.keys[i]);
    } else {
      stream_keys<BF16>(xr, vocab, t, f);
    }
  }
  __device__ __forceinline__ u64 mass(uint32_t key) const { return key_mass<BF16>(key, kmax, smax); }
  __device__ __forceinline__ bool kept(uint32_t key) const {
    if constexpr (WARP) return key >= tkeep && key <= tcap;
    else return key >= tkeep;
  }
  // l = s - smax as key_mass takes it (0 at the maximal key, also when the maximum is infinite)
  __device__ __forceinline__ float ell(uint32_t key) const { return key == kmax ? 0.f : key_score<BF16>(key) - smax; }

  // §8.1 (1)-(3): keys, top-k, top-p
  __device__ __forceinline__ void keep(const vstar_vqa_sampling& P) {
    const int k = P.top_k > 0 ? (P.top_k < vocab ? P.top_k : vocab) : 0;
    // ---- pass 0: keys (into LDS), their maximum, the high-byte counts for top-k ----
    uint32_t km = 0;
    stream_keys<BF16>(xr, vocab, t, [&](int i, uint32_t key) {
      if constexpr (CACHED) sm.keys[i] = (uint16_t)key;
      km = key > km ? key : km;
      if (k) atomicAdd(&sm.hist[key >> 8], 1ull);
    });
    kmax = block_max(sm, km);                          // (synchronises: the cached keys are visible from here on)
    smax = key_score<BF16>(kmax);
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
    tkeep = tk;
    if (P.top_p < 1.f) {
      clear_hist(sm);
      each([&](int, uint32_t key) {
        if (key >= tk) { const u64 m = mass(key); if (m) atomicAdd(&sm.hist[key >> 8], m); }
      });
      int hb, lb;
      u64 above, a2, need, n2;
      select_bin(sm, 0, P.top_p, hb, above, need);     // need = ceil(top_p * Z_k); 0 (top_p = 0): no bin
      uint32_t tp = kmax;
      if (hb >= 0) {
        clear_hist(sm);
        each([&](int, uint32_t key) {
          if ((int)(key >> 8) == hb && key >= tk) { const u64 m = mass(key); if (m) atomicAdd(&sm.hist[key & 255u], m); }
        });
        select_bin(sm, need - above, -1.f, lb, a2, n2);
        if (lb >= 0) tp = ((uint32_t)hb << 8) | (uint32_t)lb;
      }
      tp = tp < kmax ? tp : kmax;
      tkeep = tp > tk ? tp : tk;
    }
  }

  // ---- §8.10: min-p -> typical-p -> epsilon -> eta on the set keep() left; a stage that is off runs nothing ----
  // Z = the mass of the kept set (exact), A = sum m * l over it (double, fixed order); tokens of mass 0 take part in nothing
  __device__ __forceinline__ void sums(u64& Z, double& A) const {
    u64 z = 0;
    double a = 0.0;
    each([&](int, uint32_t key) {
      if (kept(key)) { const u64 m = mass(key); if (m) { z += m; a += (double)m * (double)ell(key); } }
    });
    block_sums(sm, z, a);
    Z = z;
    A = a;
  }
  // tkeep = max(tkeep, the smallest key whose mass is >= thr), but never above ktop, the largest key of the kept set: mass is
  // monotone in the key, so this is a bisection of the key space (every thread the same 16 steps, no pass over the row)
  __device__ __forceinline__ void raise_floor(double thr, uint32_t ktop) {
    constexpr uint32_t NEG_INF_KEY = BF16 ? 0x007fu : 0x03ffu;       // below it lie NaN patterns only: no element has such a key
    uint32_t lo = tkeep > NEG_INF_KEY ? tkeep : NEG_INF_KEY, hi = ktop;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((double)mass(mid) >= thr) hi = mid; else lo = mid + 1;
    }
    tkeep = hi > tkeep ? hi : tkeep;
  }
  // d = |l - mu| as a non-negative fp32, complemented: a SMALLER distance is a LARGER word, so select_bin's "from the top" is
  // "from the smallest distance"
  __device__ __forceinline__ uint32_t rdist(uint32_t key, double mu) const {
    return ~__float_as_uint(fabsf((float)((double)ell(key) - mu)));
  }
  __device__ __forceinline__ void warp(const vstar_vqa_warpers& W) {
    static_assert(WARP, "warp() needs the band");
    uint32_t ktop = kmax;                              // the largest key of the kept set
    u64 Z = 0;
    double A = 0.0;
    bool fresh = false;                                // Z / A are those of the current kept set
    if (W.min_p > 0.f) raise_floor((double)W.min_p * 0x1p40, ktop);      // p_i >= min_p * max p  <=>  m_i >= min_p * 2^40
    if (W.typical_p < 1.f) {
      sums(Z, A);
      const double mu = A / (double)Z;                 // E_p[l]; Z > 0: the maximal key is kept
      // the threshold distance D: the largest d whose strictly-smaller mass is < typical_p * Z — a mass-weighted radix select over
      // the four bytes of the complemented distance word
      uint32_t pre = 0;
      u64 need = 0;
      bool found = true;
#pragma unroll
      for (int byte = 3; byte >= 0; --byte) {
        const int sh = 8 * byte;
        clear_hist(sm);
        each([&](int, uint32_t key) {
          if (!kept(key)) return;
          const u64 m = mass(key);
          if (!m) return;
          const uint32_t r = rdist(key, mu);
          if (byte == 3 || (r >> (sh + 8)) == pre) atomicAdd(&sm.hist[(r >> sh) & 255u], m);
        });
        int b;
        u64 above, n2;
        select_bin(sm, need, byte == 3 ? W.typical_p : -1.f, b, above, n2);      // byte 3: need = ceil(typical_p * Z) >= 1
        found = found && b >= 0;
        need = n2 - above;
        pre = (pre << 8) | (uint32_t)(b & 255);
      }
      if (found) {                                     // the band: the keys of the kept set with d <= D (all ties in d)
        uint32_t hi = 0, lo = 0;
        each([&](int, uint32_t key) {
          if (kept(key) && rdist(key, mu) >= pre) { hi = key > hi ? key : hi; lo = (0xffffu - key) > lo ? (0xffffu - key) : lo; }
        });
        hi = block_max(sm, hi);
        lo = 0xffffu - block_max(sm, lo);
        if (lo <= hi) { tkeep = lo; tcap = hi; ktop = hi; }      // (always: the selected token is in it)
      }
    }
    if (W.epsilon_cutoff > 0.f) {
      if (!fresh) sums(Z, A);
      const uint32_t t0 = tkeep;
      raise_floor((double)W.epsilon_cutoff * (double)Z, ktop);           // p_i >= eps  <=>  m_i >= eps * Z
      fresh = tkeep == t0;
    }
    if (W.eta_cutoff > 0.f) {
      if (!fresh) sums(Z, A);
      const double eps = (double)W.eta_cutoff, Zd = (double)Z;
      const double H = log(Zd * 0x1p-40) - A / Zd;     // -sum p ln p with ln m_i = l_i + 40 ln 2
      const double eta = fmin(eps, sqrt(eps) * exp(-H));
      raise_floor(eta * Zd, ktop);
    }
  }
};

// §8.1 (4), the inverse CDF in vocabulary order over the kept set: thread-contiguous chunks [c0, c1) of the row, their kept mass
// `msum` and count, and an exact exclusive scan of both (excl, total Z; ctot = the size of the kept set).
struct ChunkScan {
  int c0, c1;
  u64 msum, excl, Z, ctot;
};

template <bool BF16, bool CACHED, bool WARP>
__device__ __forceinline__ ChunkScan chunk_scan(const WarpedRow<BF16, CACHED, WARP>& w) {
  ChunkScan c;
  const int tid = threadIdx.x, C = (w.vocab + THREADS - 1) / THREADS;
  c.c0 = tid * C < w.vocab ? tid * C : w.vocab;
  c.c1 = c.c0 + C < w.vocab ? c.c0 + C : w.vocab;
  c.msum = 0;
  u64 cnt = 0;
  for (int i = c.c0; i < c.c1; ++i) {
    const uint32_t key = w.key_at(i);
    if (w.kept(key)) { c.msum += w.mass(key); ++cnt; }
  }
  u64 cexcl;
  block_scan(w.sm, c.msum, c.excl, c.Z);
  block_scan(w.sm, cnt, cexcl, c.ctot);
  return c;
}

// *out = the smallest kept index whose inclusive prefix mass exceeds `target` (< the total): exactly one thread — the one whose
// chunk holds the target — walks its chunk and stores.  skip >= 0 takes that index (mass m_skip, 0 if it is not kept) out of the
// kept set: the prefix masses are those of the remaining tokens, and target < Z - m_skip.
template <bool BF16, bool CACHED, bool WARP>
__device__ __forceinline__ void chunk_pick(const WarpedRow<BF16, CACHED, WARP>& w, const ChunkScan& c, u64 target, int skip, u64 m_skip,
                                           int32_t* __restrict__ out) {
  u64 excl = c.excl, msum = c.msum;
  if (skip >= 0) {
    if (skip < c.c0) excl -= m_skip;
    else if (skip < c.c1) msum -= m_skip;
  }
  if (excl <= target && target < excl + msum) {      // exactly one thread: the prefix masses tile [0, total) and target < total
    u64 acc = excl;
    for (int i = c.c0; i < c.c1; ++i) {
      const uint32_t key = w.key_at(i);
      if (w.kept(key) && i != skip) {
        acc += w.mass(key);
        if (acc > target) { *out = i; break; }
      }
    }
  }
}

}  // namespace samplecore
