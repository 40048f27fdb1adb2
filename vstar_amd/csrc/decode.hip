// decode.hip — kernels of the KV-cached language-model path (VQA-LLM: LLaVA/llava/model/language_model/
// llava_search_llama.py:56-113 driven by vstar_bench_eval.py:78-165; HF LlamaAttention 4.31 with past_key_values) and of the
// object-feature Perceiver resampler (LLaVA/llava/model/multimodal_projector/perceiver.py:25-121).
//
// Every launcher that touches the KV cache takes one layer's view of it (KvLayer, kernels.hpp: format, cells, scale bytes, strides)
// and the rows of the call (KvRows: per-row position / sequence / slot, per-sequence own slot / prefix slot / past length, the
// nullable ancestry table); the kernels receive the fields as separate __restrict__ parameters.
//
//   rope_kv_append       rotate-half RoPE (HF rounding points) on q,k in place at per-row absolute positions + K/V rows
//                        written into the per-slot cache [slot][head][ctx][128].
//   cached_attn_kernel   one workgroup per (new row, head): scores against the cached keys (prefix slot below `past`, own
//                        slot from there on — option scoring forks a shared question prefix without copying it), fp32
//                        softmax, probabilities rounded to the storage type like HF, PV from the cached values.
//   cached_attn_split_*  the same for decode steps of few sequences, the keys of a (row, head) cut into 8 partitions.
//   perceiver_attn       32 latents x (256 media + 32 latent) keys, 16 heads x 96 dims: one wave per (image, head, latent).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <type_traits>
#include "common.hpp"
#include "kernels.hpp"
#include "gemm_epilogue.hpp"
#include "mx.hpp"

namespace VS_NS {

namespace {

// ------------------------------------------------ embedding rows ------------------------------------------------
__global__ void embed_rows_kernel(const int32_t* __restrict__ src, const lp_t* __restrict__ table, int vocab,
                                  const lp_t* __restrict__ feats, int64_t n_feat_rows, lp_t* __restrict__ x, int R, int C) {
  const int vec = C >> 3;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * vec) return;
  const int r = (int)(idx / vec), v = (int)(idx - (int64_t)r * vec);
  const int sidx = src[r];
  lpx8 o = {0, 0, 0, 0, 0, 0, 0, 0};
  if (sidx >= 0) {
    if (sidx < vocab) o = *(const lpx8*)(table + (int64_t)sidx * C + v * 8);
  } else if (sidx != INT32_MIN) {
    const int64_t f = -(int64_t)sidx - 1;
    if (f < n_feat_rows) o = *(const lpx8*)(feats + f * C + v * 8);
  }
  *(lpx8*)(x + (int64_t)r * C + v * 8) = o;
}

// ------------------------------------------------ block-scaled fp8 KV rows ------------------------------------------------
// KV-cache formats (KvLayer::fmt, kernels.hpp) as the template parameter KVF of every kernel that touches the cache:
//   0  fp16 rows [128]: the kernels as they always were
//   1  MX e4m3: a row is 128 code bytes + 4 E8M0 bytes (one per block of 32 head-dim elements, mx.hpp's arithmetic); the cache
//      pointers then address BYTES with the same element strides, the scale bytes live at (element offset / 32) of their own array
//   2  the fp16 cache holding fp16(decoded): format 1's values through format 0's readers (the yardstick of the bit-identity tests)
// kv8_quant is the ONE place a value is quantised: every writer of formats 1 and 2 and the op-level quantiser call it with the
// block's amax, however their lane geometry reduced it.  The decoded value code x 2^(e - 127) is exact in fp32 and, for fp16 inputs
// below 63488, exactly representable in fp16 — so the two formats hold the same numbers.
__device__ __forceinline__ float kv8_scale(uint32_t e) { return __uint_as_float(e << 23); }      // 2^(e - 127); e = 0: all-zero block
__device__ __forceinline__ uint32_t kv8_quant(float x, float amax, uint32_t* e_out, float* xhat) {
  const uint32_t e = mx_e8m0(amax);
  const uint32_t c = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x * mx_inv_scale(e), 0.f, 0, false) & 0xffu;
  *e_out = e;
  // (the sign is taken from the code: a value that rounds to zero keeps its sign bit in the code, and so does the decoded row)
  *xhat = __uint_as_float(__float_as_uint(fabsf(__builtin_amdgcn_cvt_f32_fp8((int)c, 0)) * kv8_scale(e)) | ((c & 0x80u) << 24));
  return c;
}
// max over the 2^LOG2 neighbouring lanes of a block (all of them active)
template <int LOG2>
__device__ __forceinline__ float kv8_lanes_max(float v) {
#pragma unroll
  for (int o = 1 << (LOG2 - 1); o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// one element of a cached row held by one lane (the fused writers: 32 neighbouring lanes hold a block): quantise, store at element
// offset `off` of the layer's cache, return the value the row now has
template <int KVF>
__device__ __forceinline__ float kv8_put(lp_t* cache, uint8_t* scales, int64_t off, float x) {
  uint32_t e;
  float xhat;
  const uint32_t c = kv8_quant(x, kv8_lanes_max<5>(fabsf(x)), &e, &xhat);
  if constexpr (KVF == 1) {
    ((uint8_t*)cache)[off] = (uint8_t)c;
    if ((off & 31) == 0) scales[off >> 5] = (uint8_t)e;
  } else {
    cache[off] = f2lp(xhat);
  }
  return xhat;
}
// a lane's 8 consecutive elements of a cached row, as loaded / as fp32
template <int KVF> struct KvFrag { lpx8 v; };
template <> struct KvFrag<1> { uint2 c; uint32_t s; };
template <int KVF> struct KvCell { typedef lp_t type; };
template <> struct KvCell<1> { typedef uint8_t type; };
template <int KVF>
__device__ __forceinline__ KvFrag<KVF> kv_frag_zero() {
  KvFrag<KVF> f;
  if constexpr (KVF == 1) { f.c = make_uint2(0u, 0u); f.s = 0u; }
  else f.v = (lpx8){0, 0, 0, 0, 0, 0, 0, 0};
  return f;
}
// row = the cached row (kv_row), base = the layer's cache, l16 = the lane's 8-vector
template <int KVF>
__device__ __forceinline__ KvFrag<KVF> kv_frag_load(const typename KvCell<KVF>::type* row, const typename KvCell<KVF>::type* base,
                                                    const uint8_t* scales, int l16) {
  KvFrag<KVF> f;
  if constexpr (KVF == 1) {
    f.c = *(const uint2*)(row + l16 * 8);
    f.s = *(const uint32_t*)(scales + ((row - base) >> 5));       // the row's 4 scale bytes
  } else {
    f.v = *(const lpx8*)(row + l16 * 8);
  }
  return f;
}
// format 1: the 8 codes -> fp32 and ONE exact multiply by the block's power of two
__device__ __forceinline__ void kv8_frag_f32(const KvFrag<1>& f, int l16, float* x) {
  const float s = kv8_scale((f.s >> ((l16 >> 2) * 8)) & 0xffu);
  const auto p0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)f.c.x, false), p1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)f.c.x, true);
  const auto p2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)f.c.y, false), p3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)f.c.y, true);
  x[0] = p0[0] * s; x[1] = p0[1] * s; x[2] = p1[0] * s; x[3] = p1[1] * s;
  x[4] = p2[0] * s; x[5] = p2[1] * s; x[6] = p3[0] * s; x[7] = p3[1] * s;
}
template <int KVF>
__device__ __forceinline__ void kv_frag_f32(const KvFrag<KVF>& f, int l16, float* x) {
  if constexpr (KVF == 1) kv8_frag_f32(f, l16, x);
  else {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = lp2f((lp_t)f.v[e]);
  }
}

// [rows, 128] fp16 -> codes [rows, 128], E8M0 bytes [rows, 4], (nullable, may alias x) xhat: one lane per element
__global__ __launch_bounds__(256) void kv_quantize_rows_kernel(const lp_t* x, int64_t n, uint8_t* __restrict__ codes,
                                                               uint8_t* __restrict__ scales, lp_t* xhat) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;                                  // n % 128 == 0: the 32 lanes of a block stay together
  uint32_t e;
  float xh;
  const float v = lp2f(x[idx]);
  const uint32_t c = kv8_quant(v, kv8_lanes_max<5>(fabsf(v)), &e, &xh);
  codes[idx] = (uint8_t)c;
  if ((idx & 31) == 0) scales[idx >> 5] = (uint8_t)e;
  if (xhat) xhat[idx] = f2lp(xh);
}

// ------------------------------------------------ RoPE + KV-cache append ------------------------------------------------
// One output of rotate-half RoPE with HF's three rounding points: h(h(x * c) + h(y * s)).  Contraction is OFF here: with it the
// compiler narrows the sum of the two rounded products to fp16 and fuses one product into it (v_pk_fma_f16 / v_fma_f16) — that product
// is then never rounded on its own, and q / k come out one fp16 step off the reference's in some elements.
__device__ __forceinline__ lp_t rope_out(float x, float c, float y, float s) {
#pragma clang fp contract(off)
  const float xc = rlp(x * c), ys = rlp(y * s);
  return f2lp(xc + ys);
}
// One thread per (row, q|k|v, head, 8-vector of the FIRST half of the head dim); handles d0 and d0 + D/2 together.
// KVF != 0: a block of 32 is the 8-vectors of 4 neighbouring threads; the round-tripped k AND v also replace the row's k / v in
// `qkv`, which the prefill attention reads — a position has one value whoever reads it.
template <int KVF>
__global__ void rope_kv_append_kernel(lp_t* __restrict__ qkv, const lp_t* __restrict__ cos_sin, const int32_t* __restrict__ row_pos,
                                      const int32_t* __restrict__ row_slot, lp_t* __restrict__ kc, lp_t* __restrict__ vc,
                                      int64_t slot_stride, int ctx, int R, int H, uint8_t* __restrict__ ks, uint8_t* __restrict__ vs) {
  constexpr int D = 128, HALF = 64, VPH = HALF / 8;
  const int per_row = 3 * H * VPH;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)R * per_row) return;
  const int row = (int)(idx / per_row);
  int rem = (int)(idx - (int64_t)row * per_row);
  const int which = rem / (H * VPH);
  rem -= which * H * VPH;
  const int h = rem / VPH, d0 = (rem - h * VPH) * 8;
  const int pos = row_pos[row];
  if (pos < 0) return;                                   // padding row of a ragged prefill batch
  lp_t* base = qkv + (int64_t)row * (3 * H * D) + which * (H * D) + h * D;
  lpx8 o1 = *(const lpx8*)(base + d0), o2 = *(const lpx8*)(base + d0 + HALF);
  if (which < 2) {
    const lpx8 c = *(const lpx8*)(cos_sin + (int64_t)pos * D + d0);
    const lpx8 sn = *(const lpx8*)(cos_sin + (int64_t)pos * D + HALF + d0);
    const lpx8 x1 = o1, x2 = o2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float a = lp2f((lp_t)x1[e]), b = lp2f((lp_t)x2[e]);
      const float cs = lp2f((lp_t)c[e]), si = lp2f((lp_t)sn[e]);
      o1[e] = (short)rope_out(a, cs, -b, si);
      o2[e] = (short)rope_out(b, cs, a, si);
    }
    if (KVF == 0 || which == 0) {
      *(lpx8*)(base + d0) = o1;
      *(lpx8*)(base + d0 + HALF) = o2;
    }
    if (which == 0) return;
  }
  if constexpr (KVF == 0) {
    lp_t* dst = (which == 1 ? kc : vc) + (int64_t)row_slot[row] * slot_stride + ((int64_t)h * ctx + pos) * D;
    *(lpx8*)(dst + d0) = o1;
    *(lpx8*)(dst + d0 + HALF) = o2;
  } else {
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a1 = fmaxf(a1, fabsf(lp2f((lp_t)o1[e])));
      a2 = fmaxf(a2, fabsf(lp2f((lp_t)o2[e])));
    }
    a1 = kv8_lanes_max<2>(a1);
    a2 = kv8_lanes_max<2>(a2);
    uint32_t c1[8], c2[8], e1 = 0, e2 = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float h1, h2;
      c1[e] = kv8_quant(lp2f((lp_t)o1[e]), a1, &e1, &h1);
      c2[e] = kv8_quant(lp2f((lp_t)o2[e]), a2, &e2, &h2);
      o1[e] = (short)f2lp(h1);
      o2[e] = (short)f2lp(h2);
    }
    *(lpx8*)(base + d0) = o1;
    *(lpx8*)(base + d0 + HALF) = o2;
    const int64_t off = (int64_t)row_slot[row] * slot_stride + ((int64_t)h * ctx + pos) * D;
    if constexpr (KVF == 1) {
      uint8_t* dst = (uint8_t*)(which == 1 ? kc : vc) + off;
      *(uint2*)(dst + d0) = make_uint2(c1[0] | (c1[1] << 8) | (c1[2] << 16) | (c1[3] << 24), c1[4] | (c1[5] << 8) | (c1[6] << 16) | (c1[7] << 24));
      *(uint2*)(dst + d0 + HALF) = make_uint2(c2[0] | (c2[1] << 8) | (c2[2] << 16) | (c2[3] << 24), c2[4] | (c2[5] << 8) | (c2[6] << 16) | (c2[7] << 24));
      if ((d0 & 31) == 0) {
        uint8_t* sc = (which == 1 ? ks : vs) + (off >> 5);
        sc[d0 >> 5] = (uint8_t)e1;
        sc[2 + (d0 >> 5)] = (uint8_t)e2;
      }
    } else {
      lp_t* dst = (which == 1 ? kc : vc) + off;
      *(lpx8*)(dst + d0) = o1;
      *(lpx8*)(dst + d0 + HALF) = o2;
    }
  }
}

// ------------------------------------------------ attention over the KV cache ------------------------------------------------
// FUSED (decode steps: every sequence contributes exactly one new row): the workgroup also applies RoPE to its row's q and
// k, appends k and v to the cache and attends to them from LDS — rope_kv_append's work without its launch.
// ANC (beam search): key / value row j of a sequence lives in slot anc[kv_slot * ctx + j] (the KV ancestry
// table) instead of `j < past ? prefix : own`; the caller has set the entries of the rows it writes to kv_slot.
// The launchers take the layer's KvLayer and the call's KvRows and hand the kernels their fields as separate __restrict__ parameters.
//
// The three attention kernels repeat five pieces: the slot pointers of a (sequence, head), the q / k half of the RoPE + append
// prologue, the score pass, the own-key score and the PV pass.  Each exists ONCE, below — as a macro, not as a function: with every
// piece a __forceinline__ function (functors for the store of a score and the probability of a key, in three variants) each kernel
// kept its values bit for bit but not its instruction stream, and the un-fused continuation of the fp8 cache measured 0.15 % slower
// per step; textual sharing leaves all three kernels the machine code they had with the copies written out
// (profiles/kv_views_machine_code.txt).  The pieces use the kernels' common names (seq, h, pos, past, arow, tid, l16, grp, qv, mx, ...).
template <bool ANC, class T>
__device__ __forceinline__ const T* kv_row(const T* head0, const T* pre, const T* own, const int32_t* arow, int j, int past,
                                           int64_t slot_stride) {
  constexpr int D = 128;
  if constexpr (ANC) return head0 + (int64_t)arow[j] * slot_stride + (int64_t)j * D;
  else return (j < past ? pre : own) + (int64_t)j * D;
}
// head h of the sequence's own slot / of its prefix slot / of slot 0 in `cache`: p##own, p##pre, p##h0
#define KV_SLOT_PTRS(p, cache)                                                                                   \
  cell_t* p##own = (cell_t*)(cache) + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;                 \
  const cell_t* p##pre = (const cell_t*)(cache) + (int64_t)seq_prefix[seq] * slot_stride + (int64_t)h * ctx * D; \
  const cell_t* p##h0 = (const cell_t*)(cache) + (int64_t)h * ctx * D
// lane d of q (which == 0) or k (which == 1): rotate-half RoPE with HF's rounding points; q -> qs, k -> the cache (formats 1 / 2:
// kv8_put, the whole of wave 1: 32 lanes per block) and, as the value the cache now holds, own_k
#define KV_ROPE_QK()                                                                                   \
  const lp_t* base = rowp + which * (H * D);                                                           \
  const float x1 = lp2f(base[d]), x2 = lp2f(base[d + 64]);                                             \
  const float cs = lp2f(cos_sin[(int64_t)pos * D + d]), si = lp2f(cos_sin[(int64_t)pos * D + 64 + d]); \
  const lp_t o1 = rope_out(x1, cs, -x2, si), o2 = rope_out(x2, cs, x1, si);                            \
  if (which == 0) {                                                                                    \
    qs[d] = lp2f(o1);                                                                                  \
    qs[d + 64] = lp2f(o2);                                                                             \
  } else if constexpr (KVF == 0) {                                                                     \
    own_k[d] = lp2f(o1);                                                                               \
    own_k[d + 64] = lp2f(o2);                                                                          \
    kown[(int64_t)pos * D + d] = o1;                                                                   \
    kown[(int64_t)pos * D + d + 64] = o2;                                                              \
  } else {                                                                                             \
    const int64_t own_off = (int64_t)seq_kv[seq] * slot_stride + ((int64_t)h * ctx + pos) * D;         \
    own_k[d] = kv8_put<KVF>(kc, ks, own_off + d, lp2f(o1));                                            \
    own_k[d + 64] = kv8_put<KVF>(kc, ks, own_off + d + 64, lp2f(o2));                                  \
  }
// scores of the cached keys [J_LO, J_HI): 16 lanes per key, 16 key groups, 4 keys per group and pass (64 keys in flight per pass);
// STORE runs on the first lane of key j with its score sv (HF: matmul output in the storage type, then / sqrt(head_dim))
#define KV_SCORE_PASS(J_LO, J_HI, STORE)                                                                                                 \
  for (int j0 = J_LO; j0 < J_HI; j0 += 64) {                                                                                             \
    KvFrag<KVF> kv8[4];                                                                                                                  \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                                      \
      const int j = j0 + u * 16 + grp;                                                                                                   \
      kv8[u] = kv_frag_zero<KVF>();                                                                                                      \
      if (j < J_HI)                                                                                                                      \
        kv8[u] = kv_frag_load<KVF>(kv_row<ANC>(kh0, kpre, (const cell_t*)kown, arow, j, past, slot_stride), (const cell_t*)kc, ks, l16); \
    }                                                                                                                                    \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                                      \
      const int j = j0 + u * 16 + grp;                                                                                                   \
      float a = 0.f, kx[8];                                                                                                              \
      kv_frag_f32<KVF>(kv8[u], l16, kx);                                                                                                 \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) a += qv[e] * kx[e];                                                                  \
      a += __shfl_xor(a, 8, 64);                                                                                                         \
      a += __shfl_xor(a, 4, 64);                                                                                                         \
      a += __shfl_xor(a, 2, 64);                                                                                                         \
      a += __shfl_xor(a, 1, 64);                                                                                                         \
      if (j < J_HI) {                                                                                                                    \
        const float sv = rlp(rlp(a) / inv_scale);                                                                                        \
        if (l16 == 0) { STORE; }                                                                                                         \
        mx = fmaxf(mx, sv);                                                                                                              \
      }                                                                                                                                  \
    }                                                                                                                                    \
  }
// the score of the row's own key, from LDS (key group 0)
#define KV_OWN_SCORE(STORE)                                                      \
  float a = 0.f;                                                                 \
  _Pragma("unroll") for (int e = 0; e < 8; ++e) a += qv[e] * own_k[l16 * 8 + e]; \
  a += __shfl_xor(a, 8, 64);                                                     \
  a += __shfl_xor(a, 4, 64);                                                     \
  a += __shfl_xor(a, 2, 64);                                                     \
  a += __shfl_xor(a, 1, 64);                                                     \
  const float sv = rlp(rlp(a) / inv_scale);                                      \
  if (l16 == 0) { STORE; }                                                       \
  mx = fmaxf(mx, sv)
// o += P.V over the cached keys J_FIRST, J_FIRST + 16, ... < J_HI of this key group: lane = 8 output dims (16-byte V loads), 4 keys in
// flight; PROB is key j's probability, rounded to the storage type (HF .to(query.dtype))
#define KV_PV_PASS(J_FIRST, J_HI, PROB)                                                                                                 \
  for (int j0 = J_FIRST; j0 < J_HI; j0 += 64) {                                                                                         \
    KvFrag<KVF> v8[4];                                                                                                                  \
    float pr[4];                                                                                                                        \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                                     \
      const int j = j0 + u * 16;                                                                                                        \
      v8[u] = kv_frag_zero<KVF>();                                                                                                      \
      pr[u] = 0.f;                                                                                                                      \
      if (j < J_HI) {                                                                                                                   \
        v8[u] = kv_frag_load<KVF>(kv_row<ANC>(vh0, vpre, (const cell_t*)vown, arow, j, past, slot_stride), (const cell_t*)vc, vs, l16); \
        pr[u] = PROB;                                                                                                                   \
      }                                                                                                                                 \
    }                                                                                                                                   \
    _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                                                     \
      float vx[8];                                                                                                                      \
      kv_frag_f32<KVF>(v8[u], l16, vx);                                                                                                 \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) o[e] += pr[u] * vx[e];                                                              \
    }                                                                                                                                   \
  }

template <bool FUSED, bool ANC, int KVF = 0>
__global__ __launch_bounds__(256) void cached_attn_kernel(const lp_t* __restrict__ qkv, lp_t* __restrict__ kc, lp_t* __restrict__ vc,
                                                          const int32_t* __restrict__ row_seq, const int32_t* __restrict__ row_pos,
                                                          const int32_t* __restrict__ seq_kv, const int32_t* __restrict__ seq_prefix,
                                                          const int32_t* __restrict__ seq_past, const lp_t* __restrict__ cos_sin,
                                                          lp_t* __restrict__ out, int H, int ctx, int64_t slot_stride,
                                                          float inv_scale, const int32_t* __restrict__ anc,
                                                          uint8_t* __restrict__ ks, uint8_t* __restrict__ vs) {
  constexpr int D = 128;
  typedef typename KvCell<KVF>::type cell_t;  // fp16 element or code byte: same element strides
  extern __shared__ float dyn[];            // [D] q | [nk] scores/probabilities
  __shared__ float redbuf[8];
  __shared__ float part[16][D];
  __shared__ float own_k[D], own_v[D];
  const int r = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
  const int pos = row_pos[r];
  if (pos < 0) return;
  const int seq = row_seq[r];
  const int past = seq_past[seq], nk = pos + 1;
  const int nkc = FUSED ? pos : nk;         // keys that come from the cache
  KV_SLOT_PTRS(k, kc);
  KV_SLOT_PTRS(v, vc);
  const int32_t* arow = ANC ? anc + (int64_t)seq_kv[seq] * ctx : nullptr;
  float* qs = dyn;
  float* sc = dyn + D;
  const lp_t* rowp = qkv + (int64_t)r * (3 * H * D) + h * D;
  if (FUSED) {
    if (tid < 128) {                         // rotate-half RoPE with HF's rounding points: tid 0-63 q pairs, 64-127 k pairs
      const int which = tid >> 6, d = tid & 63;
      KV_ROPE_QK();
    } else {
      const int d = tid - 128;
      const lp_t v = rowp[2 * H * D + d];
      if constexpr (KVF == 0) {
        own_v[d] = lp2f(v);
        vown[(int64_t)pos * D + d] = v;
      } else {                                // the whole of waves 2 and 3
        const int64_t own_off = (int64_t)seq_kv[seq] * slot_stride + ((int64_t)h * ctx + pos) * D;
        own_v[d] = kv8_put<KVF>(vc, vs, own_off + d, lp2f(v));
      }
    }
  } else if (tid < D) {
    qs[tid] = lp2f(rowp[tid]);
  }
  __syncthreads();
  // ---- scores: 16 lanes per key, 16 key groups, 4 keys per group and pass (64 keys in flight per pass) ----
  const int l16 = tid & 15, grp = tid >> 4;
  float qv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qv[e] = qs[l16 * 8 + e];
  float mx = -3.0e38f;
  KV_SCORE_PASS(0, nkc, sc[j] = sv);
  if (FUSED && grp == 0) {                     // the row's own key, from LDS
    KV_OWN_SCORE(sc[pos] = sv);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) redbuf[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redbuf[0], redbuf[1]), fmaxf(redbuf[2], redbuf[3]));
  float sum = 0.f;
  for (int j = tid; j < nk; j += 256) {
    const float e = __expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) redbuf[4 + (tid >> 6)] = sum;
  __syncthreads();
  const float inv = 1.0f / (redbuf[4] + redbuf[5] + redbuf[6] + redbuf[7]);
  // ---- PV: group = keys j == grp (mod 16), lane = 8 output dims (16-byte V loads), 4 keys in flight; probabilities are
  // rounded to the storage type (HF .to(query.dtype)) ----
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  KV_PV_PASS(grp, nkc, rlp(sc[j] * inv));
  if (FUSED && grp == 0) {
    const float pr = rlp(sc[pos] * inv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] += pr * own_v[l16 * 8 + e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[grp][l16 * 8 + e] = o[e];
  __syncthreads();
  if (tid < D) {
    float t = 0.f;
#pragma unroll
    for (int g2 = 0; g2 < 16; ++g2) t += part[g2][tid];
    out[(int64_t)r * (H * D) + h * D + tid] = f2lp(t);
  }
}

// ------------------------------------------------ split-KV decode attention ------------------------------------------------
// A decode step of few sequences leaves cached_attn_kernel<true> on R x 32 workgroups of 256 CUs, each pulling the whole K and V
// of its head through one CU (17.8 us per layer at ~700 keys: 15 % of a batch-1 token).  Here the keys of a (row, head) are cut
// into P partitions = P workgroups.  The reference's rounding points need the GLOBAL softmax statistics before a probability is
// rounded to the storage type, so the work is two launches:
//   scores kernel  RoPE(q) (+ RoPE(k), append k / v to the cache: last partition), this partition's scores -> workspace, its
//                  local max and sum of exponentials
//   pv kernel      global max / sum from the P partials (fixed order), probabilities rounded like HF, partial P.V; the LAST
//                  partition to finish (ticket) adds the partials in partition order and writes the row — no spinning, no
//                  co-residency requirement, deterministic summation order.
// Same arithmetic per key as cached_attn_kernel; only the order of the fp32 sums differs.
constexpr int SPLIT_P = 8;

__device__ __forceinline__ void split_range(int nkc, int p, int* lo, int* hi) {
  const int span = (((nkc + SPLIT_P - 1) / SPLIT_P) + 63) & ~63;
  *lo = p * span < nkc ? p * span : nkc;
  *hi = *lo + span < nkc ? *lo + span : nkc;
}

// the workspace of cached_attention_split_ws_bytes(max_rows, H, ctx), cut up
struct SplitWs {
  float *scores, *stats, *opart;      // [rows * H] x [ctx] / [SPLIT_P][2] / [SPLIT_P][128]
  int* cnt;                           // [rows * H] tickets
  SplitWs(void* ws, int max_rows, int H, int ctx) {
    const size_t rh = (size_t)max_rows * H;
    scores = (float*)ws;
    stats = scores + rh * ctx;
    opart = stats + rh * SPLIT_P * 2;
    cnt = (int*)(opart + rh * SPLIT_P * 128);
  }
};

template <bool ANC, int KVF = 0>
__global__ __launch_bounds__(256) void cached_attn_split_scores_kernel(
    const lp_t* __restrict__ qkv, lp_t* __restrict__ kc, lp_t* __restrict__ vc, const int32_t* __restrict__ row_seq,
    const int32_t* __restrict__ row_pos, const int32_t* __restrict__ seq_kv, const int32_t* __restrict__ seq_prefix,
    const int32_t* __restrict__ seq_past, const lp_t* __restrict__ cos_sin, float* __restrict__ ws_scores, float* __restrict__ ws_stats,
    int H, int ctx, int64_t slot_stride, float inv_scale, const int32_t* __restrict__ anc, uint8_t* __restrict__ ks,
    uint8_t* __restrict__ vs) {
  constexpr int D = 128;
  typedef typename KvCell<KVF>::type cell_t;
  extern __shared__ float dyn[];            // this partition's scores (span + 1)
  __shared__ float qs[D], own_k[D], redbuf[8];
  const int r = blockIdx.x, h = blockIdx.y, p = blockIdx.z, tid = threadIdx.x;
  const int pos = row_pos[r];
  if (pos < 0) return;
  const int seq = row_seq[r];
  const int past = seq_past[seq], nkc = pos;
  KV_SLOT_PTRS(k, kc);
  cell_t* vown = (cell_t*)vc + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;
  const int32_t* arow = ANC ? anc + (int64_t)seq_kv[seq] * ctx : nullptr;
  const lp_t* rowp = qkv + (int64_t)r * (3 * H * D) + h * D;
  const bool last = p == SPLIT_P - 1;
  if (tid < 128) {                           // rotate-half RoPE with HF's rounding points: tid 0-63 q pairs, 64-127 k pairs
    const int which = tid >> 6, d = tid & 63;
    if (which == 0 || last) {
      KV_ROPE_QK();
    }
  } else if (last) {
    const int d = tid - 128;
    if constexpr (KVF == 0) {
      vown[(int64_t)pos * D + d] = rowp[2 * H * D + d];
    } else {                                  // the whole of waves 2 and 3
      const int64_t own_off = (int64_t)seq_kv[seq] * slot_stride + ((int64_t)h * ctx + pos) * D;
      kv8_put<KVF>(vc, vs, own_off + d, lp2f(rowp[2 * H * D + d]));
    }
  }
  __syncthreads();
  int j_lo, j_hi;
  split_range(nkc, p, &j_lo, &j_hi);
  float* gsc = ws_scores + ((int64_t)r * H + h) * ctx;
  const int l16 = tid & 15, grp = tid >> 4;
  float qv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) qv[e] = qs[l16 * 8 + e];
  float mx = -3.0e38f;
  KV_SCORE_PASS(j_lo, j_hi, dyn[j - j_lo] = sv; gsc[j] = sv);
  int n_loc = j_hi - j_lo;
  if (last) {                                  // the row's own key, from LDS
    if (grp == 0) {
      KV_OWN_SCORE(dyn[n_loc] = sv; gsc[pos] = sv);
    }
    n_loc += 1;
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) redbuf[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redbuf[0], redbuf[1]), fmaxf(redbuf[2], redbuf[3]));
  float sum = 0.f;
  for (int j = tid; j < n_loc; j += 256) sum += __expf(dyn[j] - mx);
  sum = wave_sum(sum);
  if ((tid & 63) == 0) redbuf[4 + (tid >> 6)] = sum;
  __syncthreads();
  if (tid == 0) {
    float* st = ws_stats + (((int64_t)r * H + h) * SPLIT_P + p) * 2;
    st[0] = mx;
    st[1] = (redbuf[4] + redbuf[5]) + (redbuf[6] + redbuf[7]);
  }
}

template <bool ANC, int KVF = 0>
__global__ __launch_bounds__(256) void cached_attn_split_pv_kernel(
    const lp_t* __restrict__ vc, const int32_t* __restrict__ row_seq, const int32_t* __restrict__ row_pos,
    const int32_t* __restrict__ seq_kv, const int32_t* __restrict__ seq_prefix, const int32_t* __restrict__ seq_past,
    const float* __restrict__ ws_scores, const float* __restrict__ ws_stats, float* __restrict__ ws_opart, int* __restrict__ ws_cnt,
    lp_t* __restrict__ out, int H, int ctx, int64_t slot_stride, const int32_t* __restrict__ anc, const uint8_t* __restrict__ vs) {
  constexpr int D = 128;
  typedef typename KvCell<KVF>::type cell_t;
  __shared__ float part[16][D];
  __shared__ int ticket;
  const int r = blockIdx.x, h = blockIdx.y, p = blockIdx.z, tid = threadIdx.x;
  const int pos = row_pos[r];
  if (pos < 0) return;
  const int seq = row_seq[r];
  const int past = seq_past[seq], nkc = pos;
  KV_SLOT_PTRS(v, vc);
  const int32_t* arow = ANC ? anc + (int64_t)seq_kv[seq] * ctx : nullptr;
  const float* st = ws_stats + ((int64_t)r * H + h) * SPLIT_P * 2;
  float M = -3.0e38f;
#pragma unroll
  for (int q = 0; q < SPLIT_P; ++q) M = fmaxf(M, st[2 * q]);
  float L = 0.f;
#pragma unroll
  for (int q = 0; q < SPLIT_P; ++q) L += st[2 * q + 1] * __expf(st[2 * q] - M);
  const float inv = 1.0f / L;
  int j_lo, j_hi;
  split_range(nkc, p, &j_lo, &j_hi);
  if (p == SPLIT_P - 1) j_hi = (j_hi == nkc) ? nkc + 1 : j_hi;       // + the row's own key / value (appended by the scores kernel)
  const float* gsc = ws_scores + ((int64_t)r * H + h) * ctx;
  const int l16 = tid & 15, grp = tid >> 4;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = 0.f;
  KV_PV_PASS(j_lo + grp, j_hi, rlp(__expf(gsc[j] - M) * inv));     // (the own key included: appended by the scores kernel)
#pragma unroll
  for (int e = 0; e < 8; ++e) part[grp][l16 * 8 + e] = o[e];
  __syncthreads();
  float* op = ws_opart + ((int64_t)r * H + h) * SPLIT_P * D;
  // Cross-workgroup hand-over WITHOUT fences: a __threadfence() here is a whole-L2 write-back + invalidate per workgroup on this
  // chip (first version of this kernel: 4.18 ms / token against 3.79 unsplit).  The partials are written with agent-scope atomic
  // stores (write-through to the coherence point, nothing left dirty in this XCD's L2), the wave waits until they are performed
  // (vmcnt(0)), then takes its ticket with an agent-scope atomic; the last workgroup reads the partials with agent-scope atomic
  // loads (never served from a stale line of its own L2).  Per-location coherence of atomics + completion of the stores before
  // the ticket is exactly the ordering needed.
  if (tid < D) {
    float t = 0.f;
#pragma unroll
    for (int g2 = 0; g2 < 16; ++g2) t += part[g2][tid];
    __hip_atomic_store(&op[p * D + tid], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) ticket = __hip_atomic_fetch_add(&ws_cnt[r * H + h], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (ticket != SPLIT_P - 1) return;
  if (tid < D) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < SPLIT_P; ++q) t += __hip_atomic_load(&op[q * D + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    out[(int64_t)r * (H * D) + h * D + tid] = f2lp(t);
  }
  if (tid == 0) __hip_atomic_store(&ws_cnt[r * H + h], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
}

// ------------------------------------------------ Perceiver attention ------------------------------------------------
// q [n*L, H*DH]; kv [n*NK, 2*H*DH] = k | v; out [n*L, H*DH].  Rounding points of the fp16 reference: q*scale, sim, sim-amax,
// softmax output and the attn·v product are each materialised in the storage type.
template <int DH>
__global__ __launch_bounds__(256) void perceiver_attn_kernel(const lp_t* __restrict__ q, const lp_t* __restrict__ kv,
                                                             lp_t* __restrict__ out, int n, int L, int NK, int H, float scale) {
  constexpr int MAXK_PER_LANE = 8;     // up to 512 keys
  __shared__ float qsh[4][DH];
  __shared__ float psh[4][64 * MAXK_PER_LANE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t wid = (int64_t)blockIdx.x * 4 + w;
  if (wid >= (int64_t)n * H * L) return;
  const int qi = (int)(wid % L), h = (int)((wid / L) % H), b = (int)(wid / ((int64_t)L * H));
  const int C = H * DH;
  const lp_t* qp = q + ((int64_t)b * L + qi) * C + h * DH;
  for (int d = lane; d < DH; d += 64) qsh[w][d] = rlp(lp2f(qp[d]) * scale);
  __builtin_amdgcn_wave_barrier();
  float sc[MAXK_PER_LANE];
  float mx = -3.0e38f;
#pragma unroll
  for (int i = 0; i < MAXK_PER_LANE; ++i) {
    const int key = i * 64 + lane;
    float s = -3.0e38f;
    if (key < NK) {
      const lp_t* kp = kv + ((int64_t)b * NK + key) * (2 * C) + h * DH;
      float a = 0.f;
#pragma unroll
      for (int d8 = 0; d8 < DH / 8; ++d8) {
        const lpx8 k8 = *(const lpx8*)(kp + d8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) a += qsh[w][d8 * 8 + e] * lp2f((lp_t)k8[e]);
      }
      s = rlp(a);
    }
    sc[i] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXK_PER_LANE; ++i) {
    const int key = i * 64 + lane;
    if (key < NK) {
      const float e = __expf(rlp(sc[i] - mx));
      sc[i] = e;
      sum += e;
    }
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
#pragma unroll
  for (int i = 0; i < MAXK_PER_LANE; ++i) {
    const int key = i * 64 + lane;
    if (key < NK) psh[w][key] = rlp(sc[i] * inv);
  }
  __builtin_amdgcn_wave_barrier();
  if (lane * 2 < DH) {
    const lp_t* vp = kv + (int64_t)b * NK * (2 * C) + C + h * DH + lane * 2;
    float o0 = 0.f, o1 = 0.f;
    for (int key = 0; key < NK; ++key) {
      const uint32_t v2 = *(const uint32_t*)(vp + (int64_t)key * (2 * C));
      const float pr = psh[w][key];
      o0 += pr * lp2f((lp_t)(v2 & 0xffff));
      o1 += pr * lp2f((lp_t)(v2 >> 16));
    }
    lp_t* op = out + ((int64_t)b * L + qi) * C + h * DH + lane * 2;
    op[0] = f2lp(o0);
    op[1] = f2lp(o1);
  }
}

// ------------------------------------------------ KV ancestry table ------------------------------------------------
// the rows a forward call writes live in their own slot
__global__ void kv_anc_mark_kernel(const int32_t* __restrict__ row_slot, const int32_t* __restrict__ row_pos, int R,
                                   int32_t* __restrict__ anc, int ctx) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int pos = row_pos[r];
  if (pos < 0) return;                                   // padding row
  anc[(int64_t)row_slot[r] * ctx + pos] = row_slot[r];
}

__global__ void kv_anc_fill_kernel(int32_t* __restrict__ row, int value, int lo, int hi) {
  const int p = lo + blockIdx.x * blockDim.x + threadIdx.x;
  if (p < hi) row[p] = value;
}

__global__ void kv_anc_gather_kernel(const int32_t* __restrict__ anc, int32_t* __restrict__ tmp, const int32_t* __restrict__ src,
                                     int lo, int w, int ctx) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (p < w) tmp[(int64_t)i * w + p] = anc[(int64_t)src[i] * ctx + lo + p];
}

__global__ void kv_anc_scatter_kernel(int32_t* __restrict__ anc, const int32_t* __restrict__ tmp, const int32_t* __restrict__ dst,
                                      int lo, int w, int ctx) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (p < w) anc[(int64_t)dst[i] * ctx + lo + p] = tmp[(int64_t)i * w + p];
}

// K / V rows [lo, lo + w) of every layer and head: dst's own rows <- the rows src's ancestry points at (16 B per thread)
// (KVF == 1: 8 code bytes per thread, and the first thread of a row moves its 4 scale bytes)
template <int KVF>
__global__ void kv_copy_rows_kernel(lp_t* __restrict__ kc, lp_t* __restrict__ vc, const int32_t* __restrict__ anc, int dst, int src,
                                    int lo, int w, int H, int ctx, int64_t slot_stride, int64_t layer_stride, int64_t n,
                                    uint8_t* __restrict__ ks, uint8_t* __restrict__ vs) {
  constexpr int D = 128;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const int v8 = (int)(idx & 15);
  int64_t rest = idx >> 4;
  const int p = lo + (int)(rest % w);
  rest /= w;
  const int h = (int)(rest % H);
  rest /= H;
  const int which = (int)(rest & 1);
  const int64_t layer = rest >> 1;
  const int from = anc[(int64_t)src * ctx + p];
  if constexpr (KVF == 1) {
    const int64_t off = layer * layer_stride + (int64_t)h * ctx * D + (int64_t)p * D;
    uint8_t* base = (uint8_t*)(which ? vc : kc) + off + v8 * 8;
    *(uint2*)(base + (int64_t)dst * slot_stride) = *(const uint2*)(base + (int64_t)from * slot_stride);
    if (v8 == 0) {
      uint8_t* sb = (which ? vs : ks) + (off >> 5);
      *(uint32_t*)(sb + (((int64_t)dst * slot_stride) >> 5)) = *(const uint32_t*)(sb + (((int64_t)from * slot_stride) >> 5));
    }
  } else {
    lp_t* base = (which ? vc : kc) + layer * layer_stride + (int64_t)h * ctx * D + (int64_t)p * D + v8 * 8;
    *(lpx8*)(base + (int64_t)dst * slot_stride) = *(const lpx8*)(base + (int64_t)from * slot_stride);
  }
}

__global__ void argmax_rows_lp_kernel(const lp_t* __restrict__ x, int cols, int64_t ld, int32_t* __restrict__ out) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int row = blockIdx.x;
  const lp_t* p = x + (int64_t)row * ld;
  float best = -3.0e38f;
  int idx = 0;
  for (int c = threadIdx.x; c < cols; c += blockDim.x) {
    const float v = lp2f(p[c]);
    if (v > best) { best = v; idx = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    out[row] = idx;
  }
}

}  // namespace

hipError_t embed_rows(const int32_t* src, const lp_t* table, int vocab, const lp_t* feats, int64_t n_feat_rows, lp_t* x, int R,
                      int C, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  const int64_t n = (int64_t)R * (C / 8);
  hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, table, vocab, feats,
                     n_feat_rows, x, R, C);
  return hipGetLastError();
}

bool kv_format_ok(const KvLayer& kv) {
#ifdef VSTAR_LP_F16
  return kv.fmt == KV_FMT_F16 || kv.fmt == KV_FMT_MXFP8_EMU || (kv.fmt == KV_FMT_MXFP8 && kv.ks && kv.vs);
#else
  return kv.fmt == KV_FMT_F16;
#endif
}

// KV_DISPATCH(fmt, CALL): CALL with the constant KVF = the runtime format fmt (the format-0 instantiation is the only one of
// the bf16 build)
#ifdef VSTAR_LP_F16
#define KV_DISPATCH(fmt, ...)                                              \
  switch (fmt) {                                                           \
    case KV_FMT_MXFP8: { constexpr int KVF = 1; __VA_ARGS__; break; }      \
    case KV_FMT_MXFP8_EMU: { constexpr int KVF = 2; __VA_ARGS__; break; }  \
    default: { constexpr int KVF = 0; __VA_ARGS__; break; }                \
  }
#else
#define KV_DISPATCH(fmt, ...) { constexpr int KVF = 0; __VA_ARGS__; }
#endif

hipError_t rope_kv_append(lp_t* qkv, const lp_t* cos_sin, const KvLayer& kv, const KvRows& rows, int R, hipStream_t s) {
  if (!kv_format_ok(kv)) return hipErrorInvalidValue;
  if (R <= 0) return hipSuccess;
  const int64_t n = (int64_t)R * 3 * kv.H * 8;
  KV_DISPATCH(kv.fmt, hipLaunchKernelGGL(rope_kv_append_kernel<KVF>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, qkv, cos_sin,
                                         rows.row_pos, rows.row_slot, (lp_t*)kv.k, (lp_t*)kv.v, kv.slot_stride, kv.ctx, R, kv.H, kv.ks,
                                         kv.vs));
  return hipGetLastError();
}

#ifdef VSTAR_LP_F16
hipError_t kv_quantize_rows(const lp_t* x, int rows, uint8_t* codes, uint8_t* scales, lp_t* xhat, hipStream_t s) {
  if (!x || !codes || !scales || rows <= 0) return hipErrorInvalidValue;
  const int64_t n = (int64_t)rows * 128;
  hipLaunchKernelGGL(kv_quantize_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, codes, scales, xhat);
  return hipGetLastError();
}
#endif

size_t cached_attention_split_ws_bytes(int max_rows, int H, int ctx) {
  const size_t rh = (size_t)max_rows * H;
  return rh * ((size_t)ctx * 4 + SPLIT_P * 2 * 4 + SPLIT_P * 128 * 4 + 4) + 256;
}

// decode steps of few sequences: P partitions per (row, head) so that the K / V streams of a head run on 8 CUs instead of one
bool cached_attention_splits(bool fused, bool have_ws, int R, int split_max_rows, int H, int max_keys) {
  static const bool split_on = [] { const char* v = getenv("VSTAR_DECODE_SPLIT_KV"); return !v || atoi(v) != 0; }();
  return split_on && fused && have_ws && R <= split_max_rows && R * H <= 128 && max_keys >= 256;
}

static thread_local int t_last_path = -1;
int cached_attention_last_path() { return t_last_path; }

template <bool ANC, int KVF>
static hipError_t cached_attention_t(const lp_t* qkv, const KvLayer& kv, const KvRows& rows, const lp_t* fused_cos_sin, lp_t* out, int R,
                                     int max_keys, hipStream_t s, void* split_ws, int split_max_rows, int decide_rows) {
  const float inv_scale = sqrtf(128.0f);
  lp_t *kc = (lp_t*)kv.k, *vc = (lp_t*)kv.v;      // (the kernels' cell type is their KVF's)
  // (decide_rows: the decision of a step of that many rows; the workspace bound is R's own either way)
  if (R <= split_max_rows &&
      cached_attention_splits(fused_cos_sin != nullptr, split_ws != nullptr, decide_rows > 0 ? decide_rows : R, split_max_rows, kv.H, max_keys)) {
    t_last_path = 2;
    const SplitWs ws(split_ws, split_max_rows, kv.H, kv.ctx);
    const int span = ((((max_keys + SPLIT_P - 1) / SPLIT_P) + 63) & ~63) + 1;
    hipLaunchKernelGGL((cached_attn_split_scores_kernel<ANC, KVF>), dim3(R, kv.H, SPLIT_P), dim3(256), (size_t)span * sizeof(float), s,
                       qkv, kc, vc, rows.row_seq, rows.row_pos, rows.seq_kv, rows.seq_prefix, rows.seq_past, fused_cos_sin, ws.scores,
                       ws.stats, kv.H, kv.ctx, kv.slot_stride, inv_scale, rows.anc, kv.ks, kv.vs);
    hipLaunchKernelGGL((cached_attn_split_pv_kernel<ANC, KVF>), dim3(R, kv.H, SPLIT_P), dim3(256), 0, s, vc, rows.row_seq, rows.row_pos,
                       rows.seq_kv, rows.seq_prefix, rows.seq_past, ws.scores, ws.stats, ws.opart, ws.cnt, out, kv.H, kv.ctx,
                       kv.slot_stride, rows.anc, kv.vs);
    return hipGetLastError();
  }
  const size_t lds = (size_t)(128 + max_keys) * sizeof(float);
  if (lds > 40 * 1024) return hipErrorInvalidValue;
  t_last_path = fused_cos_sin ? 1 : 0;
  hipLaunchKernelGGL((fused_cos_sin ? cached_attn_kernel<true, ANC, KVF> : cached_attn_kernel<false, ANC, KVF>), dim3(R, kv.H), dim3(256),
                     lds, s, qkv, kc, vc, rows.row_seq, rows.row_pos, rows.seq_kv, rows.seq_prefix, rows.seq_past, fused_cos_sin, out, kv.H,
                     kv.ctx, kv.slot_stride, inv_scale, rows.anc, kv.ks, kv.vs);
  return hipGetLastError();
}

hipError_t cached_attention(const lp_t* qkv, const KvLayer& kv, const KvRows& rows, const lp_t* fused_cos_sin, lp_t* out, int R,
                            int max_keys, hipStream_t s, void* split_ws, int split_max_rows, int decide_rows) {
  t_last_path = -1;
  if (!kv_format_ok(kv)) return hipErrorInvalidValue;
  if (R <= 0) return hipSuccess;
  hipError_t e = hipErrorInvalidValue;
  KV_DISPATCH(kv.fmt, e = rows.anc ? cached_attention_t<true, KVF>(qkv, kv, rows, fused_cos_sin, out, R, max_keys, s, split_ws, split_max_rows, decide_rows)
                                   : cached_attention_t<false, KVF>(qkv, kv, rows, fused_cos_sin, out, R, max_keys, s, split_ws, split_max_rows, decide_rows));
  return e;
}

// ---- KV ancestry table (beam search): anc[slot * ctx + p] = the slot whose cache holds position p ----
hipError_t kv_anc_mark(const int32_t* row_slot, const int32_t* row_pos, int R, int32_t* anc, int ctx, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  hipLaunchKernelGGL(kv_anc_mark_kernel, dim3((R + 255) / 256), dim3(256), 0, s, row_slot, row_pos, R, anc, ctx);
  return hipGetLastError();
}

hipError_t kv_anc_fill(int32_t* anc, int slot, int value, int lo, int hi, int ctx, hipStream_t s) {
  lo = lo < 0 ? 0 : lo;
  hi = hi > ctx ? ctx : hi;
  if (hi <= lo) return hipSuccess;
  hipLaunchKernelGGL(kv_anc_fill_kernel, dim3((hi - lo + 255) / 256), dim3(256), 0, s, anc + (int64_t)slot * ctx, value, lo, hi);
  return hipGetLastError();
}

hipError_t kv_anc_reorder(int32_t* anc, int32_t* tmp, const int32_t* d_dst, const int32_t* d_src, int n, int lo, int hi, int ctx,
                          hipStream_t s) {
  const int w = hi - lo;
  if (n <= 0 || w <= 0) return hipSuccess;
  const dim3 grid((w + 255) / 256, n);
  hipLaunchKernelGGL(kv_anc_gather_kernel, grid, dim3(256), 0, s, anc, tmp, d_src, lo, w, ctx);     // every source read ...
  hipLaunchKernelGGL(kv_anc_scatter_kernel, grid, dim3(256), 0, s, anc, tmp, d_dst, lo, w, ctx);    // ... before any destination
  return hipGetLastError();
}

hipError_t kv_copy_rows(const KvLayer& kv0, int layers, int64_t layer_stride, const int32_t* anc, int dst, int src, int lo, int hi,
                        hipStream_t s) {
  if (!kv_format_ok(kv0)) return hipErrorInvalidValue;
  if (hi <= lo) return hipSuccess;
  const int64_t n = (int64_t)2 * layers * kv0.H * (hi - lo) * 16;
  KV_DISPATCH(kv0.fmt, hipLaunchKernelGGL(kv_copy_rows_kernel<KVF>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (lp_t*)kv0.k,
                                          (lp_t*)kv0.v, anc, dst, src, lo, hi - lo, kv0.H, kv0.ctx, kv0.slot_stride, layer_stride, n,
                                          kv0.ks, kv0.vs));
  return hipGetLastError();
}

hipError_t perceiver_attention(const lp_t* q, const lp_t* kv, lp_t* out, int n, int L, int NK, int H, int DH, hipStream_t s) {
  if (DH != 96 && DH != 64 && DH != 32) return hipErrorInvalidValue;
  if (NK > 512 || n <= 0) return hipErrorInvalidValue;
  const int64_t waves = (int64_t)n * H * L;
  const dim3 grid((unsigned)((waves + 3) / 4));
  const float scale = 1.0f / sqrtf((float)DH);
  if (DH == 96) hipLaunchKernelGGL(perceiver_attn_kernel<96>, grid, dim3(256), 0, s, q, kv, out, n, L, NK, H, scale);
  else if (DH == 64) hipLaunchKernelGGL(perceiver_attn_kernel<64>, grid, dim3(256), 0, s, q, kv, out, n, L, NK, H, scale);
  else hipLaunchKernelGGL(perceiver_attn_kernel<32>, grid, dim3(256), 0, s, q, kv, out, n, L, NK, H, scale);
  return hipGetLastError();
}

hipError_t argmax_rows_lp(const lp_t* x, int rows, int cols, int64_t ld, int32_t* out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(argmax_rows_lp_kernel, dim3(rows), dim3(256), 0, s, x, cols, ld, out);
  return hipGetLastError();
}

}  // namespace VS_NS
