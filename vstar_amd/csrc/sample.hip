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
//   warpers  (nullable) min-p -> typical-p -> epsilon -> eta between top-p and the draw, one vstar_vqa_warpers
//            record per row; typical-p turns the kept set into a band Tlo <= key <= Thi.  Without records the kernel is the one
//            above and nothing else (its own instantiation)
// Rows of up to CACHE elements keep their keys in LDS after the first read (32001 at 7B: one HBM/L2 read per row); longer rows
// re-read the logits from L2 in every pass.  The row-level code lives in sample_core.hpp, shared with spec.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "sample.hpp"
#include "sample_core.hpp"

namespace {

using namespace samplecore;

template <bool BF16, bool CACHED, bool WARP>
__global__ __launch_bounds__(THREADS) void sample_rows_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                              const vstar_vqa_sampling* __restrict__ params,
                                                              const vstar_vqa_warpers* __restrict__ warpers,
                                                              int32_t* __restrict__ tokens, float* __restrict__ u_out,
                                                              int32_t* __restrict__ n_kept, uint8_t* __restrict__ kept_mask) {
  __shared__ SampleSmem<CACHED> sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const vstar_vqa_sampling P = params[row];
  if (tid < 256) sm.hist[tid] = 0;
  if (tid == 0) sm.u24 = philox_u24(P.seed, P.stream, P.step);
  __syncthreads();
  WarpedRow<BF16, CACHED, WARP> w(sm, x + (int64_t)row * ld, vocab, P.temperature);
  w.keep(P);                                         // keys, top-k, top-p (sample_core.hpp)
  if constexpr (WARP) {                              // min-p, typical-p, epsilon, eta (§8.10); the kept mask for the tests
    if (warpers) w.warp(warpers[row]);
    if (kept_mask) {
      uint8_t* mr = kept_mask + (int64_t)row * vocab;
      w.each([&](int i, uint32_t key) { mr[i] = w.kept(key) ? 1 : 0; });
    }
  }
  // ---- draw: inverse CDF in vocabulary order over the kept set ----
  const ChunkScan c = chunk_scan(w);
  const u64 u = sm.u24;
  chunk_pick(w, c, scale_u24(c.Z, u), -1, 0, tokens + row);      // floor(u * Z * 2^-24), exact
  if (tid == 0) {
    if (u_out) u_out[row] = (float)u * 0x1p-24f;
    if (n_kept) n_kept[row] = (int32_t)c.ctot;
  }
}

// warpers == kept_mask == null: the §8.1 kernel as it always was (no band, no added instruction); else the WARP instantiation
template <bool BF16>
hipError_t sample_rows(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                       const vstar_vqa_warpers* d_warpers, int32_t* tokens, float* u_out, int32_t* n_kept, uint8_t* kept_mask,
                       hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || !d_params || !tokens || rows > 65535 || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab) return hipErrorInvalidValue;
  const bool warp = d_warpers || kept_mask, cached = vocab <= CACHE;
#define VSTAR_SAMPLE_LAUNCH(C, W)                                                                                               \
  hipLaunchKernelGGL((sample_rows_kernel<BF16, C, W>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, d_params, d_warpers, tokens, \
                     u_out, n_kept, kept_mask)
  if (warp) { if (cached) VSTAR_SAMPLE_LAUNCH(true, true); else VSTAR_SAMPLE_LAUNCH(false, true); }
  else { if (cached) VSTAR_SAMPLE_LAUNCH(true, false); else VSTAR_SAMPLE_LAUNCH(false, false); }
#undef VSTAR_SAMPLE_LAUNCH
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_sample_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                 const vstar_vqa_warpers* d_warpers, int32_t* tokens, float* u_out, int32_t* n_kept,
                                 uint8_t* kept_mask, hipStream_t s) {
  return sample_rows<false>(x, rows, vocab, ld, d_params, d_warpers, tokens, u_out, n_kept, kept_mask, s);
}

hipError_t vstar_sample_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const vstar_vqa_sampling* d_params,
                                  const vstar_vqa_warpers* d_warpers, int32_t* tokens, float* u_out, int32_t* n_kept,
                                  uint8_t* kept_mask, hipStream_t s) {
  return sample_rows<true>(x, rows, vocab, ld, d_params, d_warpers, tokens, u_out, n_kept, kept_mask, s);
}

bool vstar_sample_params_valid(const vstar_vqa_sampling& p) {
  return p.temperature > 0.f && std::isfinite(p.temperature) && p.top_k >= 0 && p.top_p >= 0.f;     // (NaN fails both)
}

const char* vstar_warpers_check(const vstar_vqa_warpers* w, int n) {
  for (int i = 0; i < n; ++i) {      // (written so that NaN fails)
    if (!(w[i].min_p >= 0.f && w[i].min_p <= 1.f)) return "warpers: min_p must be in [0, 1] (0 = off)";
    if (!(w[i].typical_p > 0.f)) return "warpers: typical_p must be > 0 (>= 1 = off)";
    if (!(w[i].epsilon_cutoff >= 0.f && w[i].epsilon_cutoff < 1.f)) return "warpers: epsilon_cutoff must be in [0, 1) (0 = off)";
    if (!(w[i].eta_cutoff >= 0.f && w[i].eta_cutoff < 1.f)) return "warpers: eta_cutoff must be in [0, 1) (0 = off)";
  }
  return nullptr;
}
