// spec.hip — the verify tail of speculative decoding: a decode step feeds a sequence its current token plus a few guessed
// (draft) tokens as one multi-row continuation; this tail chooses a token per logits row, compares it with the draft that was
// fed as the NEXT row, and returns per sequence how many drafts hold and the tokens chosen.  DESIGN.md §8.5.
//
// Launch 1, one workgroup (16 waves) per row, rows independent:
//   greedy   the arg-max of the row under argmax_rows_lp's rule (decode.hip): the first index of the largest number, NaN and
//            -inf never win, 0 when nothing does; flag = (choice == draft)
//   sampled  the kept set and the 2^-40 fixed-point masses of sample.hip (sample_core.hpp: the same code, the same bits), Z their
//            sum.  No draft (-1): the plain draw, u from Philox (step, stream) — bit-identical to vstar_sample_rows.  Draft x:
//            accept iff x is kept and floor(u_a * Z) < m_x, u_a from Philox (step, stream + 1); else the residual draw: x is
//            taken out of the kept set (Z' = Z - m_x, or Z when x is not kept) and the token is the smallest kept index != x
//            whose inclusive prefix mass, skipping x, exceeds floor(u * Z').  P(row's token = y) = m_y / Z either way.  With
//            warpers the kept set is the band they leave: a draft outside it is never accepted.
// Launch 2, one thread per group: n_accept = the number of leading rows whose flag is set (a group's last row is never
// compared), tokens = the choices of rows 0 .. n_accept, -1 behind them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spec.hpp"
#include "sample_core.hpp"

namespace {

using namespace samplecore;

template <bool BF16, bool CACHED, bool WARP>
__global__ __launch_bounds__(THREADS) void verify_sampled_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                                 const int32_t* __restrict__ draft,
                                                                 const vstar_vqa_sampling* __restrict__ params,
                                                                 const vstar_vqa_warpers* __restrict__ warpers,
                                                                 int32_t* __restrict__ choice, int32_t* __restrict__ flag) {
  __shared__ SampleSmem<CACHED> sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const vstar_vqa_sampling P = params[row];
  const int xd = draft[row];                         // -1 or in [0, vocab): checked on the host (vstar_verify_check)
  if (tid < 256) sm.hist[tid] = 0;
  __syncthreads();
  WarpedRow<BF16, CACHED, WARP> w(sm, x + (int64_t)row * ld, vocab, P.temperature);
  w.keep(P);
  if constexpr (WARP) w.warp(warpers[row]);                  // §8.10: the same kept set (a band) as the draw's
  const ChunkScan c = chunk_scan(w);
  const u64 u = philox_u24(P.seed, P.stream, P.step);        // (every thread: uniform values, no LDS round trip)
  if (xd < 0 || xd >= vocab) {                               // no draft: the plain §8.1 draw
    chunk_pick(w, c, scale_u24(c.Z, u), -1, 0, choice + row);
    if (tid == 0) flag[row] = 0;
    return;
  }
  const uint32_t kx = w.key_at(xd);
  const u64 mx = w.kept(kx) ? w.mass(kx) : 0;                // 0: not kept (or a kept token whose mass rounds to 0: never accepted)
  const u64 ua = philox_u24(P.seed, P.stream + 1, P.step);
  if (scale_u24(c.Z, ua) < mx) {                             // (uniform over the workgroup)
    if (tid == 0) { choice[row] = xd; flag[row] = 1; }
    return;
  }
  chunk_pick(w, c, scale_u24(c.Z - mx, u), xd, mx, choice + row);      // mx < Z here: mx == Z always accepts
  if (tid == 0) flag[row] = 0;
}

template <bool BF16>
__global__ __launch_bounds__(THREADS) void verify_greedy_kernel(const uint16_t* __restrict__ x, int vocab, int64_t ld,
                                                                const int32_t* __restrict__ draft, int32_t* __restrict__ choice,
                                                                int32_t* __restrict__ flag) {
  __shared__ float bv[WAVES];
  __shared__ int bi[WAVES];
  const int row = blockIdx.x, tid = threadIdx.x;
  const uint16_t* xr = x + (int64_t)row * ld;
  float best = -3.0e38f;                             // argmax_rows_lp's start value and comparisons
  int idx = 0;
  for (int i = tid; i < vocab; i += THREADS) {
    const float v = bits2f<BF16>(xr[i]);
    if (v > best) { best = v; idx = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WAVES; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    choice[row] = idx;
    flag[row] = idx == draft[row];
  }
}

__global__ void verify_finish_kernel(const int32_t* __restrict__ group_off, int n_groups, const int32_t* __restrict__ choice,
                                     const int32_t* __restrict__ flag, int32_t* __restrict__ n_accept, int32_t* __restrict__ tokens) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const int r0 = group_off[g], r1 = group_off[g + 1];
  int a = 0;
  while (r0 + a < r1 - 1 && flag[r0 + a]) ++a;       // the last row is never compared
  n_accept[g] = a;
  for (int r = r0; r < r1; ++r) tokens[r] = r - r0 <= a ? choice[r] : -1;
}

template <bool BF16>
hipError_t verify_rows(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                       const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers, int32_t* choice,
                       int32_t* flag, int32_t* n_accept, int32_t* tokens, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || !group_off || !draft || !choice || !flag || !n_accept || !tokens || n_groups <= 0 || n_groups > rows || rows > 65535 ||
      vocab <= 0 || vocab > MAX_VOCAB || ld < vocab)
    return hipErrorInvalidValue;
  if (!params)
    hipLaunchKernelGGL((verify_greedy_kernel<BF16>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, draft, choice, flag);
  else {                                             // (greedy ignores the warpers, as it ignores top-k / top-p)
    const bool cached = vocab <= CACHE;
#define VSTAR_VERIFY_LAUNCH(C, W)                                                                                                \
  hipLaunchKernelGGL((verify_sampled_kernel<BF16, C, W>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, draft, params, warpers, choice, \
                     flag)
    if (warpers) { if (cached) VSTAR_VERIFY_LAUNCH(true, true); else VSTAR_VERIFY_LAUNCH(false, true); }
    else { if (cached) VSTAR_VERIFY_LAUNCH(true, false); else VSTAR_VERIFY_LAUNCH(false, false); }
#undef VSTAR_VERIFY_LAUNCH
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(verify_finish_kernel, dim3((n_groups + 63) / 64), dim3(64), 0, s, group_off, n_groups, choice, flag, n_accept, tokens);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_verify_rows_f16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                                 const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers, int32_t* choice,
                                 int32_t* flag, int32_t* n_accept, int32_t* tokens, hipStream_t s) {
  return verify_rows<false>(x, rows, vocab, ld, group_off, n_groups, draft, params, warpers, choice, flag, n_accept, tokens, s);
}

hipError_t vstar_verify_rows_bf16(const uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* group_off, int n_groups,
                                  const int32_t* draft, const vstar_vqa_sampling* params, const vstar_vqa_warpers* warpers, int32_t* choice,
                                  int32_t* flag, int32_t* n_accept, int32_t* tokens, hipStream_t s) {
  return verify_rows<true>(x, rows, vocab, ld, group_off, n_groups, draft, params, warpers, choice, flag, n_accept, tokens, s);
}

const char* vstar_verify_check(int rows, int vocab, int n_groups, const int32_t* group_off, const int32_t* draft) {
  if (rows <= 0 || n_groups <= 0 || !group_off || !draft) return "verify: no rows / groups / drafts";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "verify: vocabulary size out of range [1, 2^22]";
  if (group_off[0] != 0 || group_off[n_groups] != rows) return "verify: the groups must cover the wanted rows exactly";
  for (int g = 0; g < n_groups; ++g) {
    const int n = group_off[g + 1] - group_off[g];
    if (group_off[g] < 0 || group_off[g + 1] > rows) return "verify: group_off exceeds the wanted rows";
    if (n < 1) return "verify: an empty group (group_off must increase)";
    if (n > VSTAR_VERIFY_MAX_GROUP) return "verify: a group of more than 16 rows (the current token + at most 15 drafts)";
    if (draft[group_off[g + 1] - 1] != -1) return "verify: the last row of a group has no draft to be compared with (draft must be -1)";
  }
  for (int r = 0; r < rows; ++r)
    if (draft[r] < -1 || draft[r] >= vocab) return "verify: a draft id is outside [0, vocab) (and not -1)";
  return nullptr;
}
