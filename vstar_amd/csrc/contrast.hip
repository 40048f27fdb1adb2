// contrast.hip — the device side of contrastive search behind the language-model forward: the degeneration penalty over a per-slot
// hidden-state history, the pick, the top-k of the winner's logits row and the adoption of the winner's K/V row.  The contract and
// the arithmetic are stated in contrast.hpp; DESIGN.md §8.11.
//
//   fill     a wave per row: RMSNorm with the library's rounding points into the history (prefill rows) or the candidate buffer
//            (a step's rows), and the reciprocal norm of the stored row
//   penalty  grid (L partitions, groups), 8 waves: the group's candidate rows are staged in LDS 1024 hidden elements at a time, each
//            wave streams two history rows per pass with one 16-byte load per lane and piece and keeps one fp32 accumulator per
//            (row, candidate) and lane; butterfly, two multiplies, fmaxf; one ordered-integer atomicMax per candidate and wave
//   select   a workgroup of 16 waves per group: score and pick (double, uncontracted), append, then row_lse + the top-n select of
//            logprob.hip (row_select.hpp) on the winner's logits row
//   adopt    grid (layers x heads, groups), one wave: K and V row of the winner's slot -> the owner's, skipped where they coincide
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "contrast.hpp"
#include "row_lse.hpp"
#include "row_select.hpp"

namespace {

using rowlse::bits2f;
using rowlse::CACHE;
using rowlse::THREADS;
using rowsel::value_key;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;
constexpr int MAX_VOCAB = 1 << 22;
constexpr int MAX_GROUP = VSTAR_CONTRAST_MAX_GROUP;
constexpr int MAX_K = VSTAR_CONTRAST_MAX_K;

template <bool BF16> __device__ __forceinline__ uint16_t f2bits(float f) {
  if constexpr (BF16) return __builtin_bit_cast(unsigned short, (__bf16)f);
  else return __builtin_bit_cast(unsigned short, (_Float16)f);
}

// the xor butterfly 32, 16, 8, 4, 2, 1 of ROW ORDER: every lane ends with the same bits
__device__ __forceinline__ float butterfly(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float rnorm_of(float sq) { return sq > 0.f ? 1.0f / sqrtf(sq) : 0.f; }

// order-preserving signed image of a float (for atomicMax) and back
__device__ __forceinline__ int32_t f2ord(float f) { const int32_t b = __float_as_int(f); return b >= 0 ? b : b ^ 0x7fffffff; }
__device__ __forceinline__ float ord2f(int32_t k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// ---------------------------------------------------------------- fill ----------------------------------------------------------------
template <bool BF16, bool NORM>
__global__ __launch_bounds__(256) void contrast_fill_kernel(const uint16_t* __restrict__ x, const int32_t* __restrict__ src_row,
                                                            const uint16_t* __restrict__ w, float eps, int rows, int hidden,
                                                            const int64_t* __restrict__ dst_row, uint16_t* __restrict__ out,
                                                            float* __restrict__ rnorm) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int64_t d = NORM ? dst_row[r] : (int64_t)r;
  if (d < 0) return;
  const int pieces = hidden >> 3;
  const u16x8* xr = (const u16x8*)(x + (int64_t)(NORM && src_row ? src_row[r] : r) * hidden);
  float sq = 0.f;
  if constexpr (NORM) {
    float ss = 0.f;
    for (int p = lane; p < pieces; p += 64) {
      const u16x8 v = xr[p];
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float f = bits2f<BF16>(v[e]); ss = fmaf(f, f, ss); }
    }
    const float rstd = rsqrtf(butterfly(ss) / (float)hidden + eps);
    const u16x8* wr = (const u16x8*)w;
    u16x8* orow = (u16x8*)(out + d * hidden);
    for (int p = lane; p < pieces; p += 64) {
      const u16x8 v = xr[p], gw = wr[p];
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t = bits2f<BF16>(f2bits<BF16>(bits2f<BF16>(v[e]) * rstd));
        o[e] = f2bits<BF16>(bits2f<BF16>(gw[e]) * t);
        const float f = bits2f<BF16>(o[e]);
        sq = fmaf(f, f, sq);
      }
      orow[p] = o;
    }
  } else {
    for (int p = lane; p < pieces; p += 64) {
      const u16x8 v = xr[p];
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float f = bits2f<BF16>(v[e]); sq = fmaf(f, f, sq); }
    }
  }
  sq = butterfly(sq);
  if (lane == 0) rnorm[d] = rnorm_of(sq);
}

// -------------------------------------------------------------- penalty ---------------------------------------------------------------
constexpr int PEN_THREADS = 512, PEN_WAVES = PEN_THREADS / 64, PEN_RPW = 2, PEN_TILE = PEN_WAVES * PEN_RPW;
constexpr int PEN_CHUNK = 128;         // pieces of 8 elements staged per candidate: 1024 hidden elements, 2 pieces per lane

__global__ void contrast_pen_init_kernel(float* pen, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows) ((int32_t*)pen)[i] = f2ord(-INFINITY);
}

template <bool BF16, int MC>
__global__ __launch_bounds__(PEN_THREADS) void contrast_penalty_kernel(const uint16_t* __restrict__ cand, const float* __restrict__ cand_rn,
                                                                       int hidden, const uint16_t* __restrict__ hist,
                                                                       const float* __restrict__ hist_rn, const int32_t* __restrict__ goff,
                                                                       const int64_t* __restrict__ hist_base,
                                                                       const int32_t* __restrict__ hist_len, int rows_per_wg,
                                                                       float* pen) {
  __shared__ u16x8 stage[MC * PEN_CHUNK];
  const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = goff[g];
  int m = goff[g + 1] - r0;
  m = m < MC ? m : MC;                                // (the launcher picked MC >= every group)
  const int L = hist_len[g];
  const int j0 = blockIdx.x * rows_per_wg;
  if (j0 >= L) return;                                // (uniform)
  const int j1 = j0 + rows_per_wg < L ? j0 + rows_per_wg : L;
  const int pieces = hidden >> 3;
  const int64_t base = hist_base[g];
  const u16x8* cand8 = (const u16x8*)cand;
  const u16x8* hist8 = (const u16x8*)hist;
  float wmax[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) wmax[c] = -INFINITY;
  for (int jt = j0; jt < j1; jt += PEN_TILE) {
    float acc[PEN_RPW][MC];
#pragma unroll
    for (int rr = 0; rr < PEN_RPW; ++rr)
#pragma unroll
      for (int c = 0; c < MC; ++c) acc[rr][c] = 0.f;
    const int jr = jt + wave * PEN_RPW;               // this wave's rows jr, jr + 1 (valid below j1)
    for (int c0 = 0; c0 < pieces; c0 += PEN_CHUNK) {
      __syncthreads();                                // the chunk before is consumed
      for (int i = tid; i < m * PEN_CHUNK; i += PEN_THREADS) {
        const int c = i / PEN_CHUNK, p = i % PEN_CHUNK;
        if (c0 + p < pieces) stage[c * PEN_CHUNK + p] = cand8[(int64_t)(r0 + c) * pieces + c0 + p];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < PEN_CHUNK / 64; ++q) {
        const int p = q * 64 + lane;
        if (c0 + p >= pieces) continue;
        float hv[PEN_RPW][8];
#pragma unroll
        for (int rr = 0; rr < PEN_RPW; ++rr) {
          u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
          if (jr + rr < j1) v = hist8[(base + jr + rr) * pieces + c0 + p];
#pragma unroll
          for (int e = 0; e < 8; ++e) hv[rr][e] = bits2f<BF16>(v[e]);
        }
#pragma unroll
        for (int c = 0; c < MC; ++c) {
          if (c < m) {
            const u16x8 cv = stage[c * PEN_CHUNK + p];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float cf = bits2f<BF16>(cv[e]);
#pragma unroll
              for (int rr = 0; rr < PEN_RPW; ++rr) acc[rr][c] = fmaf(hv[rr][e], cf, acc[rr][c]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int rr = 0; rr < PEN_RPW; ++rr) {
      const bool live = jr + rr < j1;                 // (wave-uniform)
      const float hrn = live ? hist_rn[base + jr + rr] : 0.f;
#pragma unroll
      for (int c = 0; c < MC; ++c) {
        if (c < m) {
          const float dot = butterfly(acc[rr][c]);
          const float cs = dot * cand_rn[r0 + c] * hrn;
          if (live) wmax[c] = fmaxf(wmax[c], cs);
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < MC; ++c)
      if (c < m) atomicMax((int32_t*)pen + r0 + c, f2ord(wmax[c]));
  }
}

// --------------------------------------------------------------- select ---------------------------------------------------------------
template <bool CACHED>
struct ContrastSmem : rowlse::Scratch {
  uint16_t bits[CACHED ? CACHE : 1];   // raw logits bits of the winner's row
  uint32_t hist[256];
  int sel;
  uint32_t sel_above;
  uint32_t pick_key[MAX_K];
  int32_t pick_idx[MAX_K];
  double score[MAX_GROUP];
  int win;
};

// goff == null: the begin call's form (row g, no candidates, no history)
template <bool BF16, bool CACHED>
__global__ __launch_bounds__(THREADS) void contrast_select_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                                  const uint16_t* __restrict__ cand, const float* __restrict__ cand_rn,
                                                                  int hidden, const float* __restrict__ prob, float* pen, float alpha,
                                                                  int k_next, uint16_t* hist, float* hist_rn,
                                                                  const int32_t* __restrict__ goff, const int64_t* __restrict__ hist_base,
                                                                  const int32_t* __restrict__ hist_len, int32_t* __restrict__ sel,
                                                                  int32_t* __restrict__ next_tok, float* __restrict__ next_prob) {
  __shared__ ContrastSmem<CACHED> sm;
  const int g = blockIdx.x, tid = threadIdx.x;
  int row = g;
  if (goff) {
    const int r0 = goff[g];
    int m = goff[g + 1] - r0;
    m = m < MAX_GROUP ? m : MAX_GROUP;
    if (tid < m) {
      const float pn = ord2f(((const int32_t*)pen)[r0 + tid]);      // the penalty kernel's ordered image -> the float, in place
      pen[r0 + tid] = pn;
      const double a = (double)alpha;
      sm.score[tid] = __dsub_rn(__dmul_rn(__dsub_rn(1.0, a), (double)prob[r0 + tid]), __dmul_rn(a, (double)pn));
    }
    __syncthreads();
    if (tid == 0) {
      int best = 0;
      for (int c = 1; c < m; ++c)
        if (sm.score[c] > sm.score[best]) best = c;   // strict: the lowest c wins a tie
      sm.win = best;
      sel[g] = best;
    }
    __syncthreads();
    row = r0 + sm.win;
    const int64_t dst = hist_base[g] + hist_len[g];
    const u16x8* src8 = (const u16x8*)(cand + (int64_t)row * hidden);
    u16x8* dst8 = (u16x8*)(hist + dst * hidden);
    for (int p = tid; p < (hidden >> 3); p += THREADS) dst8[p] = src8[p];
    if (tid == 0) hist_rn[dst] = cand_rn[row];
  }
  // ---- the top k_next of the row and their probabilities ----
  const uint16_t* xr = x + (int64_t)row * ld;
  if (tid < 256) sm.hist[tid] = 0;
  const double lse = rowlse::row_lse<BF16, CACHED>(sm, xr, vocab);
  auto raw = [&](int i) -> uint32_t {
    if constexpr (CACHED) return sm.bits[i];
    else return xr[i];
  };
  for (int i = tid; i < vocab; i += THREADS) atomicAdd(&sm.hist[value_key<BF16>(raw(i)) >> 8], 1u);
  const uint32_t n = (uint32_t)k_next;                // (<= vocab: the host check)
  rowsel::pick_top<BF16>(sm, raw, vocab, n);
  if ((uint32_t)tid >= n) return;
  const uint32_t r = rowsel::pick_rank(sm, n, (uint32_t)tid);
  const int32_t ii = sm.pick_idx[tid];
  next_tok[(int64_t)g * k_next + r] = ii;
  next_prob[(int64_t)g * k_next + r] = (float)exp((double)bits2f<BF16>(raw(ii)) - lse);
}

// ---------------------------------------------------------------- adopt ---------------------------------------------------------------
__global__ __launch_bounds__(64) void contrast_adopt_kernel(vstar_contrast_kv kv, const int32_t* __restrict__ goff,
                                                            const int32_t* __restrict__ sel, const int32_t* __restrict__ row_slot,
                                                            const int32_t* __restrict__ owner, const int32_t* __restrict__ pos) {
  const int g = blockIdx.y, t = threadIdx.x;
  const int src = row_slot[goff[g] + sel[g]], dst = owner[g];
  if (src == dst) return;
  const int layer = blockIdx.x / kv.heads, head = blockIdx.x % kv.heads;
  const int64_t in_slot = ((int64_t)head * kv.ctx + pos[g]) * 128;
  const int64_t cs = (int64_t)layer * kv.layer_stride + (int64_t)src * kv.slot_stride + in_slot;
  const int64_t cd = (int64_t)layer * kv.layer_stride + (int64_t)dst * kv.slot_stride + in_slot;
  const int n16 = 128 * kv.cell_bytes / 16;           // 16-byte pieces of one row: 16 (16-bit cells) or 8 (code bytes)
  const int which = t >> 5, p = t & 31;               // lanes 0 .. 31: K, 32 .. 63: V
  if (p < n16) {
    const char* s = (const char*)(which ? kv.v : kv.k) + cs * kv.cell_bytes;
    char* d = (char*)(which ? kv.v : kv.k) + cd * kv.cell_bytes;
    ((uint4*)d)[p] = ((const uint4*)s)[p];
  } else if (kv.cell_bytes == 1 && p == 31) {         // the row's four E8M0 bytes
    const uint8_t* sc = which ? kv.vs : kv.ks;
    uint8_t* dc = which ? kv.vs : kv.ks;
    *(uint32_t*)(dc + cd / 32) = *(const uint32_t*)(sc + cs / 32);
  }
}

template <bool BF16>
hipError_t fill(const uint16_t* x, const int32_t* src_row, const uint16_t* w, float eps, int rows, int hidden, const int64_t* dst_row,
                uint16_t* out, float* rnorm, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || !w || !dst_row || !out || !rnorm || hidden <= 0 || hidden % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL((contrast_fill_kernel<BF16, true>), dim3((rows + 3) / 4), dim3(256), 0, s, x, src_row, w, eps, rows, hidden, dst_row,
                     out, rnorm);
  return hipGetLastError();
}

template <bool BF16> hipError_t rnorm_rows(const uint16_t* h, int rows, int hidden, float* rnorm, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!h || !rnorm || hidden <= 0 || hidden % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL((contrast_fill_kernel<BF16, false>), dim3((rows + 3) / 4), dim3(256), 0, s, h, nullptr, nullptr, 0.f, rows, hidden,
                     nullptr, nullptr, rnorm);
  return hipGetLastError();
}

bool groups_ok(const vstar_contrast_groups& g, int rows) {
  return g.n_groups >= 1 && g.n_groups <= 65535 && g.n_groups <= rows && g.goff && g.hist_base && g.hist_len && g.max_group >= 1 &&
         g.max_group <= MAX_GROUP && g.max_len >= 1;
}

template <bool BF16>
hipError_t penalty(const uint16_t* cand, const float* cand_rn, int rows, int hidden, const uint16_t* hist, const float* hist_rn,
                   const vstar_contrast_groups& g, float* pen, hipStream_t s) {
  if (!cand || !cand_rn || !hist || !hist_rn || !pen || rows <= 0 || hidden <= 0 || hidden % 8 || !groups_ok(g, rows)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(contrast_pen_init_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, pen, rows);
  // L over workgroups: whole tiles of PEN_TILE rows, about two workgroups per CU over all groups
  const int tiles = (g.max_len + PEN_TILE - 1) / PEN_TILE;
  int per_group = 512 / g.n_groups;
  per_group = per_group < 1 ? 1 : per_group;
  per_group = per_group < tiles ? per_group : tiles;
  const int rows_per_wg = (tiles + per_group - 1) / per_group * PEN_TILE;
  const dim3 grid((g.max_len + rows_per_wg - 1) / rows_per_wg, g.n_groups);
#define VSTAR_PEN(MC)                                                                                                                  \
  hipLaunchKernelGGL((contrast_penalty_kernel<BF16, MC>), grid, dim3(PEN_THREADS), 0, s, cand, cand_rn, hidden, hist, hist_rn, g.goff, \
                     g.hist_base, g.hist_len, rows_per_wg, pen)
  if (g.max_group <= 4) VSTAR_PEN(4);
  else if (g.max_group <= 8) VSTAR_PEN(8);
  else if (g.max_group <= 16) VSTAR_PEN(16);
  else VSTAR_PEN(32);
#undef VSTAR_PEN
  return hipGetLastError();
}

template <bool BF16>
hipError_t select(const uint16_t* x, int rows, int vocab, int64_t ld, const uint16_t* cand, const float* cand_rn, int hidden,
                  const float* prob, float* pen, float alpha, int k_next, uint16_t* hist, float* hist_rn, const vstar_contrast_groups* g,
                  int32_t* sel, int32_t* next_tok, float* next_prob, hipStream_t s) {
  if (!x || rows <= 0 || rows > 65535 || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab || k_next < 1 || k_next > MAX_K || k_next > vocab ||
      !next_tok || !next_prob)
    return hipErrorInvalidValue;
  if (g && (!cand || !cand_rn || !prob || !pen || !hist || !hist_rn || !sel || hidden <= 0 || hidden % 8 || !groups_ok(*g, rows)))
    return hipErrorInvalidValue;
  const dim3 grid(g ? g->n_groups : rows);
  const int32_t* goff = g ? g->goff : nullptr;
  const int64_t* hb = g ? g->hist_base : nullptr;
  const int32_t* hl = g ? g->hist_len : nullptr;
  if (vocab <= CACHE)
    hipLaunchKernelGGL((contrast_select_kernel<BF16, true>), grid, dim3(THREADS), 0, s, x, vocab, ld, cand, cand_rn, hidden, prob, pen, alpha,
                       k_next, hist, hist_rn, goff, hb, hl, sel, next_tok, next_prob);
  else
    hipLaunchKernelGGL((contrast_select_kernel<BF16, false>), grid, dim3(THREADS), 0, s, x, vocab, ld, cand, cand_rn, hidden, prob, pen, alpha,
                       k_next, hist, hist_rn, goff, hb, hl, sel, next_tok, next_prob);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_contrast_fill_f16(const uint16_t* x, const int32_t* src_row, const uint16_t* w, float eps, int rows, int hidden,
                                   const int64_t* dst_row, uint16_t* out, float* rnorm, hipStream_t s) {
  return fill<false>(x, src_row, w, eps, rows, hidden, dst_row, out, rnorm, s);
}
hipError_t vstar_contrast_fill_bf16(const uint16_t* x, const int32_t* src_row, const uint16_t* w, float eps, int rows, int hidden,
                                    const int64_t* dst_row, uint16_t* out, float* rnorm, hipStream_t s) {
  return fill<true>(x, src_row, w, eps, rows, hidden, dst_row, out, rnorm, s);
}
hipError_t vstar_contrast_rnorm_f16(const uint16_t* h, int rows, int hidden, float* rnorm, hipStream_t s) { return rnorm_rows<false>(h, rows, hidden, rnorm, s); }
hipError_t vstar_contrast_rnorm_bf16(const uint16_t* h, int rows, int hidden, float* rnorm, hipStream_t s) { return rnorm_rows<true>(h, rows, hidden, rnorm, s); }

hipError_t vstar_contrast_penalty_f16(const uint16_t* cand, const float* cand_rn, int rows, int hidden, const uint16_t* hist,
                                      const float* hist_rn, const vstar_contrast_groups& g, float* pen, hipStream_t s) {
  return penalty<false>(cand, cand_rn, rows, hidden, hist, hist_rn, g, pen, s);
}
hipError_t vstar_contrast_penalty_bf16(const uint16_t* cand, const float* cand_rn, int rows, int hidden, const uint16_t* hist,
                                       const float* hist_rn, const vstar_contrast_groups& g, float* pen, hipStream_t s) {
  return penalty<true>(cand, cand_rn, rows, hidden, hist, hist_rn, g, pen, s);
}

hipError_t vstar_contrast_select_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const uint16_t* cand, const float* cand_rn,
                                     int hidden, const float* prob, float* pen, float alpha, int k_next, uint16_t* hist, float* hist_rn,
                                     const vstar_contrast_groups& g, int32_t* sel, int32_t* next_tok, float* next_prob, hipStream_t s) {
  return select<false>(x, rows, vocab, ld, cand, cand_rn, hidden, prob, pen, alpha, k_next, hist, hist_rn, &g, sel, next_tok, next_prob, s);
}
hipError_t vstar_contrast_select_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const uint16_t* cand, const float* cand_rn,
                                      int hidden, const float* prob, float* pen, float alpha, int k_next, uint16_t* hist, float* hist_rn,
                                      const vstar_contrast_groups& g, int32_t* sel, int32_t* next_tok, float* next_prob, hipStream_t s) {
  return select<true>(x, rows, vocab, ld, cand, cand_rn, hidden, prob, pen, alpha, k_next, hist, hist_rn, &g, sel, next_tok, next_prob, s);
}
hipError_t vstar_contrast_topk_f16(const uint16_t* x, int rows, int vocab, int64_t ld, int k_next, int32_t* next_tok, float* next_prob,
                                   hipStream_t s) {
  return select<false>(x, rows, vocab, ld, nullptr, nullptr, 0, nullptr, nullptr, 0.f, k_next, nullptr, nullptr, nullptr, nullptr, next_tok,
                       next_prob, s);
}
hipError_t vstar_contrast_topk_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, int k_next, int32_t* next_tok, float* next_prob,
                                    hipStream_t s) {
  return select<true>(x, rows, vocab, ld, nullptr, nullptr, 0, nullptr, nullptr, 0.f, k_next, nullptr, nullptr, nullptr, nullptr, next_tok,
                      next_prob, s);
}

hipError_t vstar_contrast_adopt(const vstar_contrast_kv& kv, int n_groups, const int32_t* goff, const int32_t* sel,
                                const int32_t* row_slot, const int32_t* owner, const int32_t* pos, hipStream_t s) {
  if (n_groups <= 0) return hipSuccess;
  if (!kv.k || !kv.v || (kv.cell_bytes != 1 && kv.cell_bytes != 2) || (kv.cell_bytes == 1 && (!kv.ks || !kv.vs)) || kv.layers <= 0 ||
      kv.heads <= 0 || n_groups > 65535 || !goff || !sel || !row_slot || !owner || !pos)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(contrast_adopt_kernel, dim3(kv.layers * kv.heads, n_groups), dim3(64), 0, s, kv, goff, sel, row_slot, owner, pos);
  return hipGetLastError();
}

const char* vstar_contrast_check(int rows, int vocab, int n_groups, const int32_t* group_off, const float* cand_prob, float alpha,
                                 int k_next) {
  if (rows <= 0 || rows > 65535) return "contrast: rows out of range [1, 65535]";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "contrast: vocabulary size out of range [1, 2^22]";
  if (!(alpha >= 0.f && alpha <= 1.f)) return "contrast: alpha must be in [0, 1]";
  if (k_next < 2 || k_next > MAX_K || k_next > vocab) return "contrast: k_next must be in [2, 32] and <= the vocabulary size";
  if (n_groups < 1 || n_groups > rows || !group_off) return "contrast: n_groups out of range / no group_off";
  if (group_off[0] != 0 || group_off[n_groups] != rows) return "contrast: group_off must cover the rows (group_off[0] == 0, group_off[n_groups] == rows)";
  for (int g = 0; g < n_groups; ++g) {
    const int m = group_off[g + 1] - group_off[g];
    if (m < 1 || m > MAX_GROUP) return "contrast: group_off: a group must have 1 .. 32 rows";
  }
  if (!cand_prob) return "contrast: no cand_prob";
  for (int r = 0; r < rows; ++r)
    if (!(cand_prob[r] >= 0.f && cand_prob[r] <= 1.f)) return "contrast: cand_prob must be finite and in [0, 1]";
  return nullptr;
}
