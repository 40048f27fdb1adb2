// edit.hip — the logits-edit stage: HF generate's logits processors (repetition penalty, n-gram / bad-word / EOS / suppress bans,
// prefix allow-lists) as three sorted token lists per logits row, applied in place on the device between lm_head and the tail
// that picks a token.  DESIGN.md §8.8; the arguments and the semantics are documented at the launchers (edit.hpp).
//
// One workgroup (16 waves) per row, rows independent; a row without lists returns before it touches anything.  Three phases,
// separated by workgroup barriers because they can address the same element from different threads:
//   1. one thread per penalised id: read, fp32 multiply or IEEE divide, one rounding, write
//   2. one thread per banned id: -inf
//   3. allow-list: every element of [0, vocab) decides its own membership by binary search of the sorted list (staged in LDS
//      when it has at most LDS_IDS entries, read through L2 otherwise) and only NON-members are written — members are never
//      touched, so there is no fill-then-restore and no write-write race.  Whole 16-byte vectors without a member are one store;
//      the row start need not be 16-byte aligned (scalar head and tail).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "edit.hpp"

namespace {

constexpr int THREADS = 1024;
constexpr int LDS_IDS = 8192;          // allow-lists up to this length are searched in LDS (32 KiB)
constexpr int MAX_VOCAB = 1 << 22;

template <bool BF16> __device__ __forceinline__ float bits2f(uint32_t b) {
  if constexpr (BF16) return __uint_as_float(b << 16);
  else return (float)__builtin_bit_cast(_Float16, (uint16_t)b);
}
template <bool BF16> __device__ __forceinline__ uint16_t f2bits(float f) {     // round to nearest even (torch's cast)
  if constexpr (BF16) return __builtin_bit_cast(uint16_t, (__bf16)f);
  else return __builtin_bit_cast(uint16_t, (_Float16)f);
}

// the first p in [0, n] with list[p] >= v (n: none)
__device__ __forceinline__ int lower_bound(const int32_t* list, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (list[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// phase 3: -inf into every element of xr[0, vocab) that is not in list[0, n) (sorted, strictly increasing)
template <bool BF16>
__device__ __forceinline__ void keep_only(uint16_t* xr, int vocab, const int32_t* list, int n) {
  constexpr uint16_t NEG_INF = BF16 ? 0xff80u : 0xfc00u;
  const int tid = threadIdx.x;
  // [0, head): the elements in front of the row's first 16-byte boundary; nvec whole 8-element vectors; [tail0, vocab): the rest
  int head = (int)(((16u - (uint32_t)((uintptr_t)xr & 15u)) & 15u) >> 1);
  head = head < vocab ? head : vocab;
  const int nvec = (vocab - head) >> 3;
  const int tail0 = head + (nvec << 3);
  const int nscal = head + (vocab - tail0);          // <= 7 + 7
  if (tid < nscal) {
    const int i = tid < head ? tid : tail0 + (tid - head);
    const int p = lower_bound(list, n, i);
    if (p == n || list[p] != i) xr[i] = NEG_INF;
  }
  const uint32_t w = (uint32_t)NEG_INF * 0x10001u;
  const uint4 fill = make_uint4(w, w, w, w);
  for (int v = tid; v < nvec; v += THREADS) {
    const int i0 = head + (v << 3);
    int p = lower_bound(list, n, i0);
    if (p == n || list[p] >= i0 + 8) {               // no member among the eight
      *reinterpret_cast<uint4*>(xr + i0) = fill;
      continue;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (p < n && list[p] == i0 + k) ++p;
      else xr[i0 + k] = NEG_INF;
    }
  }
}

template <bool BF16>
__global__ __launch_bounds__(THREADS) void edit_rows_kernel(uint16_t* __restrict__ x, int vocab, int64_t ld, const int32_t* __restrict__ off,
                                                            const int32_t* __restrict__ tok, const float* __restrict__ penalty) {
  __shared__ int32_t ids[LDS_IDS];
  constexpr uint16_t NEG_INF = BF16 ? 0xff80u : 0xfc00u;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int o0 = off[3 * row], o1 = off[3 * row + 1], o2 = off[3 * row + 2], o3 = off[3 * row + 3];
  if (o0 == o3) return;                              // no lists: the row is neither read nor written (uniform over the workgroup)
  uint16_t* xr = x + (int64_t)row * ld;
  if (o1 > o0) {
    const float theta = penalty[row];
    for (int i = o0 + tid; i < o1; i += THREADS) {
      const int t = tok[i];
      const float f = bits2f<BF16>(xr[t]);
      xr[t] = f2bits<BF16>(f < 0.f ? f * theta : __fdiv_rn(f, theta));
    }
  }
  __syncthreads();                                   // a banned id may also be penalised: the ban is written second
  for (int i = o1 + tid; i < o2; i += THREADS) xr[tok[i]] = NEG_INF;
  if (o3 == o2) return;
  const int n = o3 - o2;
  const bool in_lds = n <= LDS_IDS;
  if (in_lds)
    for (int i = tid; i < n; i += THREADS) ids[i] = tok[o2 + i];
  __syncthreads();                                   // phases 1 / 2 before phase 3's writes; the staged list
  if (in_lds) keep_only<BF16>(xr, vocab, ids, n);
  else keep_only<BF16>(xr, vocab, tok + o2, n);
}

template <bool BF16>
hipError_t edit_rows(uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok, const float* penalty,
                     hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!x || ((uintptr_t)x & 1) || !off || rows > 65535 || vocab <= 0 || vocab > MAX_VOCAB || ld < vocab) return hipErrorInvalidValue;
  hipLaunchKernelGGL((edit_rows_kernel<BF16>), dim3(rows), dim3(THREADS), 0, s, x, vocab, ld, off, tok, penalty);
  return hipGetLastError();
}

}  // namespace

hipError_t vstar_edit_rows_f16(uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok, const float* penalty,
                               hipStream_t s) {
  return edit_rows<false>(x, rows, vocab, ld, off, tok, penalty, s);
}

hipError_t vstar_edit_rows_bf16(uint16_t* x, int rows, int vocab, int64_t ld, const int32_t* off, const int32_t* tok, const float* penalty,
                                hipStream_t s) {
  return edit_rows<true>(x, rows, vocab, ld, off, tok, penalty, s);
}

const char* vstar_edit_check(int rows, int vocab, const int32_t* off, const int32_t* tok, const float* penalty) {
  if (rows <= 0 || !off) return "edit: no rows / offsets";
  if (vocab <= 0 || vocab > MAX_VOCAB) return "edit: vocabulary size out of range [1, 2^22]";
  if (off[0] != 0) return "edit: off[0] must be 0";
  for (int i = 0; i < 3 * rows; ++i)
    if (off[i + 1] < off[i]) return "edit: the offsets must not decrease";
  if (off[3 * rows] > 0 && !tok) return "edit: token lists without a token array";
  for (int j = 0; j < rows; ++j) {
    for (int l = 0; l < 3; ++l) {
      const int a = off[3 * j + l], b = off[3 * j + l + 1];
      for (int i = a; i < b; ++i) {
        if (tok[i] < 0 || tok[i] >= vocab) return "edit: a token id is outside [0, vocab)";
        if (i > a && tok[i] <= tok[i - 1]) return "edit: every list must be strictly increasing (sorted, no repeated id)";
      }
    }
    if (off[3 * j + 1] > off[3 * j]) {
      if (!penalty) return "edit: a penalised list without penalties";
      if (!(penalty[j] > 0.f) || !std::isfinite(penalty[j])) return "edit: the repetition penalty must be finite and > 0";
    }
  }
  return nullptr;
}
