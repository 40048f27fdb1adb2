// decode.hip — kernels of the KV-cached language-model path (VQA-LLM: LLaVA/llava/model/language_model/
// llava_search_llama.py:56-113 driven by vstar_bench_eval.py:78-165; HF LlamaAttention 4.31 with past_key_values) and of the
// object-feature Perceiver resampler (LLaVA/llava/model/multimodal_projector/perceiver.py:25-121).
//
//   gemm_skinny_kernel   out[M<=64, N] = A · W^T for decode-sized M: HBM-bound weight streaming.  One workgroup owns 16 (or
//                        16 gate + 16 up) output columns, its 8 waves split K in an interleaved fashion so that the
//                        workgroup as a whole reads 512 contiguous bytes of every W row per step; partial sums meet in LDS.
//   rope_kv_append       rotate-half RoPE (HF rounding points) on q,k in place at per-row absolute positions + K/V rows
//                        written into the per-slot cache [slot][head][ctx][128].
//   cached_attn_kernel   one workgroup per (new row, head): scores against the cached keys (prefix slot below `past`, own
//                        slot from there on — option scoring forks a shared question prefix without copying it), fp32
//                        softmax, probabilities rounded to the storage type like HF, PV from the cached values.
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

// ------------------------------------------------ skinny GEMM ------------------------------------------------
// Operands as in the big kernels: W fragment is the MFMA A operand (16 output columns x 32 k), the activation fragment
// the B operand (16 rows x 32 k); lane (fr = lane%16, g = lane/16) loads 16 bytes at k = ks*32 + g*8 of W row / A row fr.
// The accumulator lane then owns output row fr, columns 4g..4g+3 — the layout gemm_epilogue_store expects.
constexpr int SK_WAVES = 8;
constexpr int SKR_WAVE_BYTES = 10240;      // gemm_skinny_ring_kernel: LDS ring per wave

// W8 forms (GemmParams::Wq): the lane's 8 k-elements of a W row are 8 bytes of int8.  Eight int8 -> eight fp16,
// exact and without a cvt chain: q ^ 0x80 = q + 128 as an unsigned byte u; the 16-bit pattern 0x6400 | u is the fp16 number
// 1024 + u (the ulp of [1024, 2048) is 1); one packed subtraction of 1152 leaves q.  Two bytes per v_perm_b32, two halves per v_pk_add_f16.
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;      // 8 int8 weights: what a lane loads per MFMA k-step
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;      // 16 bytes: the converted fragment, a chunk of the int8 tile image
__device__ __forceinline__ lpx8 w8_to_f16x8(u32x2 raw) {
  typedef __attribute__((ext_vector_type(2))) _Float16 h2;
  const h2 off = {(_Float16)1152.0f, (_Float16)1152.0f};
  u32x4 o;
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const unsigned x = raw[w] ^ 0x80808080u;
    const unsigned lo = __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u);   // bytes [x0, 0x64, x1, 0x64]
    const unsigned hi = __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u);   // bytes [x2, 0x64, x3, 0x64]
    o[2 * w] = __builtin_bit_cast(unsigned, __builtin_bit_cast(h2, lo) - off);
    o[2 * w + 1] = __builtin_bit_cast(unsigned, __builtin_bit_cast(h2, hi) - off);
  }
  return __builtin_bit_cast(lpx8, o);
}
// the one fp32 multiply per output column of the W8 forms: the lane's four columns start at packed row n
__device__ __forceinline__ f32x4 w8_scale_cols(f32x4 acc, const float* __restrict__ scale, int n) {
#pragma clang fp contract(off)      // a multiply of its own: never fused into the epilogue's bias / residual add
  const f32x4 sc = *(const f32x4*)(scale + n);
  return acc * sc;
}

// W4 form (GemmParams::Wq4): the lane's 8 k-elements of a W row are ONE 32-bit word of offset nibbles u = q + 8,
// element e in nibble (e >> 1) + 4 (e & 1).  With that order `x & 0x000F000F | 0x64006400` is the fp16 pair (1024 + u_e0,
// 1024 + u_e1) and a packed subtraction of 1032 leaves (q_e0, q_e1); nibbles 1 / 5 are taken unshifted, `x & 0x00F000F0 | 0x6400...`
// = 1024 + 16 u, and a packed fma by 1/16 and -72 leaves q exactly; one shift by 8 serves nibbles 2 / 6 and 3 / 7 the same way.
// Then ONE packed fp16 multiply by the group scale per pair: the MFMA operand is exactly fp16(fp16(q) * s), the dequantised weight.
__device__ __forceinline__ lpx8 w4_to_f16x8(unsigned x, lp_t scale_bits) {
  typedef __attribute__((ext_vector_type(2))) _Float16 h2;
  const _Float16 sc = __builtin_bit_cast(_Float16, scale_bits);
  const h2 s2 = {sc, sc};
  const h2 off = {(_Float16)1032.0f, (_Float16)1032.0f};
  const h2 r16 = {(_Float16)0.0625f, (_Float16)0.0625f}, m72 = {(_Float16)-72.0f, (_Float16)-72.0f};
  const unsigned y = x >> 8;
  const h2 q01 = __builtin_bit_cast(h2, (x & 0x000F000Fu) | 0x64006400u) - off;
  const h2 q23 = __builtin_elementwise_fma(__builtin_bit_cast(h2, (x & 0x00F000F0u) | 0x64006400u), r16, m72);
  const h2 q45 = __builtin_bit_cast(h2, (y & 0x000F000Fu) | 0x64006400u) - off;
  const h2 q67 = __builtin_elementwise_fma(__builtin_bit_cast(h2, (y & 0x00F000F0u) | 0x64006400u), r16, m72);
  u32x4 o;
  o[0] = __builtin_bit_cast(unsigned, q01 * s2);
  o[1] = __builtin_bit_cast(unsigned, q23 * s2);
  o[2] = __builtin_bit_cast(unsigned, q45 * s2);
  o[3] = __builtin_bit_cast(unsigned, q67 * s2);
  return __builtin_bit_cast(lpx8, o);
}

// The W4 tile-major image (GemmParams::Wq4_tiled): per workgroup, pair j of own double steps and wave w one slot per tile.
constexpr int W4_SLOT = 1024 + 64;          // 64 lanes x 4 words | 16 rows x 2 fp16 scales
__host__ __device__ __forceinline__ int w4_tile_pairs(int K) { return (((K >> 6) + SK_WAVES - 1) / SK_WAVES + 1) >> 1; }

// WQ: 0 = fp16 / bf16 weights (GemmParams::W), 8 = the W8 form (Wq), 4 = the W4 form (Wq4)
template <int EPI, bool OUT_F32, int MT, int WQ = 0>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny_kernel(const GemmParams p) {
  constexpr bool W8 = WQ == 8, W4 = WQ == 4;
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  __shared__ float red[SK_WAVES][MT][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;

  const lp_t* wp[NT];
  const int8_t* wq[NT];            // W8: the same row and k offset, one byte per element
  const uint32_t* w4[NT];          // W4: the same row and k offset, one word per 8 elements ...
  const lp_t* s4[NT];              // ... and the row's group scales (a double step of 64 lies inside one group of 128)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    wp[t] = WQ ? nullptr : p.W + (int64_t)(n0 + t * 16 + fr) * p.K + g * 8;
    wq[t] = W8 ? p.Wq + (int64_t)(n0 + t * 16 + fr) * p.K + g * 8 : nullptr;
    w4[t] = W4 ? p.Wq4 + (int64_t)(n0 + t * 16 + fr) * (p.K >> 3) + g : nullptr;
    s4[t] = W4 ? p.wq4_scale + (int64_t)(n0 + t * 16 + fr) * (p.K >> 7) : nullptr;
  }
  // W4, tile-major image (GemmParams::Wq4_tiled, or null): this wave's slots, pair j of tile t at img + (j * 8 NT + t) * W4_SLOT —
  // the lane's 16 bytes are its four words of its own double steps ds = wave + 16 j and ds + 8, the two scales follow the 1 KiB
  const char* img = (W4 && p.Wq4_tiled)
      ? (const char*)p.Wq4_tiled + ((int64_t)blockIdx.x * w4_tile_pairs(p.K) * SK_WAVES + wave) * (NT * W4_SLOT) + lane * 16 : nullptr;
  const int img_sc = 1024 + fr * 4 - lane * 16;          // from the lane's words to its row's scale pair
  const lp_t* ap[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    int row = m * 16 + fr;
    row = row < p.M ? row : p.M - 1;          // rows past M repeat the last row (their results are never stored)
    ap[m] = p.A + (int64_t)row * p.lda + g * 8;
  }
  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[t][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- optional fused RMSNorm of the A rows: row statistics first (same summation order as norm_kernel<true>) ----
  const bool fuse_norm = p.norm_w != nullptr;
  float rstd[MT];
  const lp_t* nwp = p.norm_w + g * 8;
  if (fuse_norm) {
    float* rs_sh = &red[0][0][0][0];
    for (int row = wave; row < p.M; row += SK_WAVES) {
      const lp_t* xr = p.A + (int64_t)row * p.lda;
      float sum = 0.f;
      for (int vi = lane; vi * 8 < p.K; vi += 64) {
        const lpx8 t = *(const lpx8*)(xr + vi * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = lp2f((lp_t)t[e]);
          sum += v * v;
        }
      }
      sum = wave_sum(sum);
      if (lane == 0) rs_sh[row] = rsqrtf(sum / (float)p.K + p.norm_eps);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int row = m * 16 + fr;
      rstd[m] = rs_sh[row < p.M ? row : p.M - 1];
    }
    __syncthreads();           // rs_sh aliases the reduction buffer used below
  }
  auto normed = [&](lpx8 x, lpx8 w, float rs) {
    lpx8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (short)f2lp(lp2f((lp_t)w[e]) * rlp(lp2f((lp_t)x[e]) * rs));
    return y;
  };

  // K is walked in DOUBLE steps of 64 elements (two MFMA k-steps = one whole 128-byte line of every W row), interleaved
  // over the 8 waves; UH double steps (2*UH k-steps) are in flight per wave before the first MFMA consumes them.
  // (W4: whole PAIRS of own double steps, the unit of the tile-major image; MT = 1: two pairs, 32 weight bytes per lane and tile)
  constexpr int UH = (MT == 2) ? 2 : (MT == 1 ? (W4 ? 4 : 1) : 2);
  const int nd = p.K >> 6;
  int ds = wave;
  for (; ds + (UH - 1) * SK_WAVES < nd; ds += UH * SK_WAVES) {
    lpx8 wf[2 * UH][NT], af[2 * UH][MT];
    u32x4 raw[W4 ? UH / 2 : 1][NT];          // W4: per pair the words of (ds, u = 0), (ds, 1), (ds + 8, 0), (ds + 8, 1) ...
    unsigned sc2[W4 ? UH / 2 : 1][NT];       // ... and the scales of ds (low half) and ds + 8 (high half)
    if constexpr (W4) {
#pragma unroll
      for (int pj = 0; pj < UH / 2; ++pj)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (img) {
            const char* sl = img + ((int64_t)(((ds - wave) >> 4) + pj) * (SK_WAVES * NT) + t) * W4_SLOT;
            raw[pj][t] = __builtin_nontemporal_load((const u32x4*)sl);
            sc2[pj][t] = *(const unsigned*)(sl + img_sc);
          } else {
            const int d0 = ds + 2 * pj * SK_WAVES, d1 = d0 + SK_WAVES;
            raw[pj][t][0] = __builtin_nontemporal_load(w4[t] + d0 * 8);
            raw[pj][t][1] = __builtin_nontemporal_load(w4[t] + d0 * 8 + 4);
            raw[pj][t][2] = __builtin_nontemporal_load(w4[t] + d1 * 8);
            raw[pj][t][3] = __builtin_nontemporal_load(w4[t] + d1 * 8 + 4);
            sc2[pj][t] = (unsigned)s4[t][d0 >> 1] | ((unsigned)s4[t][d1 >> 1] << 16);
          }
        }
    }
#pragma unroll
    for (int u = 0; u < 2 * UH; ++u) {
      const int k = (ds + (u >> 1) * SK_WAVES) * 64 + (u & 1) * 32;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if constexpr (W8) wf[u][t] = w8_to_f16x8(__builtin_nontemporal_load((const u32x2*)(wq[t] + k)));
        else if constexpr (W4) wf[u][t] = w4_to_f16x8(raw[W4 ? u >> 2 : 0][t][u & 3], (lp_t)(sc2[W4 ? u >> 2 : 0][t] >> (16 * ((u >> 1) & 1))));
        else wf[u][t] = __builtin_nontemporal_load((const lpx8*)(wp[t] + k));   // streamed once
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) af[u][m] = *(const lpx8*)(ap[m] + k);
    }
    if (fuse_norm) {
#pragma unroll
      for (int u = 0; u < 2 * UH; ++u) {
        const lpx8 nw = *(const lpx8*)(nwp + (ds + (u >> 1) * SK_WAVES) * 64 + (u & 1) * 32);
#pragma unroll
        for (int m = 0; m < MT; ++m) af[u][m] = normed(af[u][m], nw, rstd[m]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2 * UH; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[t][m] = mfma_16x16x32(wf[u][t], af[u][m], acc[t][m]);
  }
  for (; ds < nd; ds += SK_WAVES) {
    // (W4, image: own double step i = (ds - wave) / 8 is half i & 1 of pair i / 2)
    const int i4 = (ds - wave) >> 3;
    const char* sl = img ? img + (int64_t)(i4 >> 1) * (SK_WAVES * NT * W4_SLOT) + (i4 & 1) * 8 : nullptr;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = ds * 64 + h * 32;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        lpx8 wf;
        if constexpr (W8) wf = w8_to_f16x8(*(const u32x2*)(wq[t] + k));
        else if constexpr (W4) {
          if (img) wf = w4_to_f16x8(*(const unsigned*)(sl + t * W4_SLOT + h * 4), *(const lp_t*)(sl + t * W4_SLOT + img_sc - (i4 & 1) * 6));
          else wf = w4_to_f16x8(w4[t][k >> 3], s4[t][k >> 7]);
        }
        else wf = *(const lpx8*)(wp[t] + k);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          lpx8 a = *(const lpx8*)(ap[m] + k);
          if (fuse_norm) a = normed(a, *(const lpx8*)(nwp + k), rstd[m]);
          acc[t][m] = mfma_16x16x32(wf, a, acc[t][m]);
        }
      }
    }
  }
  // ---- cross-wave reduction (fixed order => results do not depend on scheduling); wave m finishes row tile m ----
  f32x4 s[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t) __syncthreads();
#pragma unroll
    for (int m = 0; m < MT; ++m) *(f32x4*)red[wave][m][lane] = acc[t][m];
    __syncthreads();
    if (wave < MT) {
      s[t] = *(const f32x4*)red[0][wave][lane];
#pragma unroll
      for (int w = 1; w < SK_WAVES; ++w) s[t] += *(const f32x4*)red[w][wave][lane];
    }
  }
  if (wave >= MT) return;
  const int n_out = (EPI == VSTAR_EPI_SILU_MUL) ? p.N / 2 : p.N;
  const int row = wave * 16 + fr;
  if (row >= p.M) return;
  if constexpr (W8) {
#pragma unroll
    for (int t = 0; t < NT; ++t) s[t] = w8_scale_cols(s[t], p.wq_scale, n0 + t * 16 + g * 4);
  }
  if (EPI == VSTAR_EPI_SILU_MUL) gemm_epilogue_store<EPI, OUT_F32>(p, row, n0 / 2 + g * 4, n_out, s[0], s[NT - 1]);
  else gemm_epilogue_store<EPI, OUT_F32>(p, row, n0 + g * 4, n_out, s[0], s[0]);
}

// ------------------------------------------------ skinny GEMM, M <= 8, operands through LDS rings ------------------------
// The same arithmetic as gemm_skinny_kernel<EPI, OUT_F32, 1> — the same MFMA operands in the same order per wave (wave w owns
// the 64-element double steps ds = w, w + 8, ...), the same fixed-order cross-wave reduction: BIT-IDENTICAL results — but no
// operand passes through registers on its way in.  Every wave owns a private ring of RD stages in LDS; a stage is one double
// step: the workgroup's 16 (x NT) weight rows (2 KiB each, two LDS-DMA requests of 8 rows x 128 B: whole cache lines, where
// the register loads above touch 16 rows x 64 B per request) plus ONE 1-KiB request for the activation side — rows 0..6 = the
// (up to 7) activation rows, row 7 = the RMSNorm weight slice when the norm is fused.  Requests cost no registers, so
// RD stages (9 - 10 KiB per wave, 72 - 80 KiB per workgroup, two workgroups per CU) are in flight instead of 16 KiB per
// workgroup: a decode step at batch 1 has one workgroup per CU in o_proj / down_proj, and 16 KiB in flight per CU is a third of
// what 6 TB/s x ~2 us of latency needs.  No barrier in the K loop (private rings, counted vmcnt).  Everything in the queue is an
// LDS-DMA request on purpose: register loads mixed into the counted waits returned out of order with the DMA requests
// (wrong results under load), requests of one kind retire in order.
// W8 form (GemmParams::Wq): a 16-row weight tile of one double step is 16 x 64 B = 1 KiB = ONE request (lane ->
// row lane/4, LDS slot lane%4 <- global chunk slot ^ ((row>>2)&3)), the activation piece is unchanged.  A stage is NT + 1 KiB, so
// the 10 KiB of a wave hold 5 stages (NT = 1: 10 KiB in flight, fp16: 9) or 3 (NT = 2: 9 KiB, fp16: 10 — a fourth stage would
// need 12 KiB per wave and two workgroups of 80 KiB are all the LDS a CU has).  In WEIGHT bytes, which are what HBM has to
// deliver (the activation pieces come from L2), that is 5 KiB per wave against fp16's 6 (NT = 1) and 6 against 8 (NT = 2): the
// activation piece of a double step stays 1 KiB while its weight tile halves, so a W8 ring of the same LDS holds FEWER weight
// bytes in flight than the fp16 ring, not more.  The counted queue still holds DMA requests only; the scales
// are read with ordinary loads after the last vmcnt(0), behind the reduction.
template <int EPI, bool OUT_F32, bool NORM, bool W8 = false>
__global__ __launch_bounds__(SK_WAVES * 64, 2) void gemm_skinny_ring_kernel(const GemmParams p) {
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  constexpr int WREQ = W8 ? 1 : 2;                    // DMA requests (1 KiB each) per 16-row weight tile and stage
  constexpr int WTILE = WREQ * 1024;                  // bytes of one 16-row weight tile of a stage
  constexpr int RD = W8 ? (NT == 1 ? 5 : 3) : (NT == 1 ? 3 : 2);     // ring depth (stages)
  constexpr int STAGE = NT * WTILE + 1024;            // bytes per stage: W tiles | activation piece
  constexpr int SOPS = WREQ * NT + 1;                 // DMA requests per stage and wave
  static_assert(RD * STAGE <= SKR_WAVE_BYTES && (RD + 1) * STAGE > SKR_WAVE_BYTES, "the ring fills the wave's LDS share");
  extern __shared__ __attribute__((aligned(16))) char smem[];      // [8 waves][10 KiB]; reused for the reduction
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  char* ring = smem + wave * SKR_WAVE_BYTES;

  // DMA sources of this lane: a request moves 8 rows x 128 B, lane -> row lane/8, LDS slot lane%8 <- global chunk slot ^ ((row>>1)&7)
  const int st_r = lane >> 3, st_c = lane & 7;
  const lp_t* wsrc[NT][2];
  const int8_t* wsrc8[NT];         // W8: one request per tile, 16 rows x 64 B
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = h * 8 + st_r;
      wsrc[t][h] = W8 ? nullptr : p.W + (int64_t)(n0 + t * 16 + row) * p.K + (st_c ^ ((row >> 1) & 7)) * 8;
    }
    const int row8 = lane >> 2;
    wsrc8[t] = W8 ? p.Wq + (int64_t)(n0 + t * 16 + row8) * p.K + ((lane & 3) ^ ((row8 >> 2) & 3)) * 16 : nullptr;
  }
  const lp_t* asrc;
  {
    const int cg = (st_c ^ ((st_r >> 1) & 7)) * 8;
    const int ar = st_r < p.M ? st_r : p.M - 1;
    asrc = (NORM && st_r == 7) ? p.norm_w + cg : p.A + (int64_t)ar * p.lda + cg;
  }
  // fragment reads: W row fr, chunk (u*4 + g) ^ ((fr>>1)&7); activation row min(fr, M-1) (< 8); norm weights = row 7
  const int arow = fr < p.M ? fr : p.M - 1;
  int w_rd[2], a_rd[2], n_rd[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    // W8: row fr at fr * 64, the 8 bytes of k = u*32 + g*8 are half g&1 of chunk u*2 + g/2, stored at slot chunk ^ ((fr>>2)&3)
    w_rd[u] = W8 ? fr * 64 + (((u * 2 + (g >> 1)) ^ ((fr >> 2) & 3)) * 16) + (g & 1) * 8
                 : fr * 128 + (((u * 4 + g) ^ ((fr >> 1) & 7)) * 16);
    a_rd[u] = NT * WTILE + arow * 128 + (((u * 4 + g) ^ ((arow >> 1) & 7)) * 16);
    n_rd[u] = NT * WTILE + 7 * 128 + (((u * 4 + g) ^ 3) * 16);
  }

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nd = p.K >> 6;
  const int n = (nd - wave + SK_WAVES - 1) / SK_WAVES;          // this wave's double steps: ds = wave + 8 i
  // tile-major weights (GemmParams::W_tiled): this workgroup's pieces lie back to back, [k-step][t][h] x 1 KiB, already in request order
  const bool tiled = W8 ? p.Wq_tiled != nullptr : p.W_tiled != nullptr;
  const lp_t* wt = (!W8 && tiled) ? p.W_tiled + ((int64_t)blockIdx.x * nd * (2 * NT)) * 512 + lane * 8 : nullptr;
  // (W8, GemmParams::Wq_tiled: [k-step][t] x 1 KiB)
  const int8_t* wt8 = (W8 && tiled) ? p.Wq_tiled + ((int64_t)blockIdx.x * nd * NT) * 1024 + lane * 16 : nullptr;
  auto issue = [&](int slot, int i) {
    const int ks = wave + i * SK_WAVES;
    const int k = ks * 64;
    char* st = ring + slot * STAGE;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if constexpr (W8) {
        const int8_t* src = tiled ? wt8 + ((int64_t)ks * NT + t) * 1024 : wsrc8[t] + k;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(st + t * WTILE), 16, 0, 0);
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const lp_t* src = tiled ? wt + ((int64_t)ks * (2 * NT) + t * 2 + h) * 512 : wsrc[t][h] + k;
          __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(st + t * 2048 + h * 1024), 16, 0, 0);
        }
      }
    }
    __builtin_amdgcn_global_load_lds((gptr_t)(asrc + k), (lptr_t)(st + NT * WTILE), 16, 0, 0);
  };
  // the first RD stages go out before anything else: neither the weights nor the raw activation rows depend on the statistics
  // (with the fused norm the last wave's last slot carries the row statistics first and is filled after them: two workgroups
  // of 80 KiB are all the LDS a CU has)
  const bool hold_last = NORM && wave == SK_WAVES - 1;
#pragma unroll
  for (int j = 0; j < RD; ++j)
    if (j < n && !(hold_last && j == RD - 1)) issue(j, j);
  // ---- optional fused RMSNorm: row statistics exactly as gemm_skinny_kernel computes them ----
  float rstd = 1.f;
  if (NORM) {
    float* rs_sh = (float*)(smem + (SK_WAVES - 1) * SKR_WAVE_BYTES + (RD - 1) * STAGE);
    // Round 5: the row's loads go out EIGHT AT A TIME and are consumed behind one wait.  With the ring's DMA requests already in
    // flight the compiler guards every ordinary load with `s_waitcnt vmcnt(0)`, so the one-load-per-iteration form paid a memory
    // round trip per 512 elements — eight in series for K = 4096, ~5 us of the ~10 us by which the two norm-fused GEMVs of a layer
    // exceeded their streaming time (profiles/r05_vqa_kernel_stats_*.csv).  Same loads, same summation order (vi ascending, then e):
    // out-of-range slots read a clamped address and contribute +0.
    const int nvec = p.K >> 3;
    for (int row = wave; row < p.M; row += SK_WAVES) {
      const lp_t* xr = p.A + (int64_t)row * p.lda;
      float sum = 0.f;
      for (int v0 = lane; v0 < nvec; v0 += 64 * 8) {
        lpx8 t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int vi = v0 + 64 * j;
          t[j] = *(const lpx8*)(xr + (vi < nvec ? vi : nvec - 1) * 8);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool in = v0 + 64 * j < nvec;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float v = in ? lp2f((lp_t)t[j][e]) : 0.f;
            sum += v * v;
          }
        }
      }
      sum = wave_sum(sum);
      if (lane == 0) rs_sh[row] = rsqrtf(sum / (float)p.K + p.norm_eps);
    }
    __syncthreads();
    rstd = rs_sh[arow];
    __syncthreads();
    if (hold_last && RD - 1 < n) issue(RD - 1, RD - 1);
  }
  auto normed = [&](lpx8 x, lpx8 w, float rs) {
    lpx8 y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = (short)f2lp(lp2f((lp_t)w[e]) * rlp(lp2f((lp_t)x[e]) * rs));
    return y;
  };

  auto consume = [&](int slot) {
    const char* st = ring + slot * STAGE;
    lpx8 wf[2][NT], a[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if constexpr (W8) wf[u][t] = w8_to_f16x8(*(const u32x2*)(st + t * WTILE + w_rd[u]));
        else wf[u][t] = *(const lpx8*)(st + t * WTILE + w_rd[u]);
      }
      a[u] = *(const lpx8*)(st + a_rd[u]);
      if (NORM) a[u] = normed(a[u], *(const lpx8*)(st + n_rd[u]), rstd);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma_16x16x32(wf[u][t], a[u], acc[t]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the slot is re-filled next: its reads must have returned
  };
  int i0 = 0;
  for (; i0 + 2 * RD <= n; i0 += RD) {
    // stages i0 .. i0+RD-1 are in flight; stage i0 + j has landed once at most the RD - 1 younger stages are outstanding
#pragma unroll
    for (int j = 0; j < RD; ++j) {
      static_assert(SOPS * (RD - 1) == 8 || SOPS * (RD - 1) == 6 || SOPS * (RD - 1) == 5, "add the literal below");
      if constexpr (SOPS * (RD - 1) == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");        // W8, NT = 1: 2 x 4
      else if constexpr (SOPS * (RD - 1) == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");   // fp16 NT = 1: 3 x 2; W8 NT = 2: 3 x 2
      else asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      consume(j);
      issue(j, i0 + RD + j);
    }
  }
  // tail: fewer than 2 RD stages left, the first RD of them (those that exist) are in flight
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int j = 0; j < RD; ++j)
    if (i0 + j < n) consume(j);
#pragma unroll
  for (int j = 0; j < RD; ++j)
    if (i0 + RD + j < n) issue(j, i0 + RD + j);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int j = 0; j < RD; ++j)
    if (i0 + RD + j < n) consume(j);

  // ---- cross-wave reduction in gemm_skinny_kernel's order; wave 0 finishes the (single) row tile ----
  __syncthreads();                                   // every wave is done with its ring
  float (*red)[64][4] = (float (*)[64][4])smem;       // [SK_WAVES][64][4]
  f32x4 s[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t) __syncthreads();
    *(f32x4*)red[wave][lane] = acc[t];
    __syncthreads();
    if (wave == 0) {
      s[t] = *(const f32x4*)red[0][lane];
#pragma unroll
      for (int w = 1; w < SK_WAVES; ++w) s[t] += *(const f32x4*)red[w][lane];
    }
  }
  if (wave != 0) return;
  const int n_out = (EPI == VSTAR_EPI_SILU_MUL) ? p.N / 2 : p.N;
  if (fr >= p.M) return;
  if constexpr (W8) {
#pragma unroll
    for (int t = 0; t < NT; ++t) s[t] = w8_scale_cols(s[t], p.wq_scale, n0 + t * 16 + g * 4);
  }
  if (EPI == VSTAR_EPI_SILU_MUL) gemm_epilogue_store<EPI, OUT_F32>(p, fr, n0 / 2 + g * 4, n_out, s[0], s[NT - 1]);
  else gemm_epilogue_store<EPI, OUT_F32>(p, fr, n0 + g * 4, n_out, s[0], s[0]);
}

// one thread per 16-byte chunk of the tile-major image (see GemmParams::W_tiled)
__global__ void skinny_tile_pack_kernel(const lp_t* __restrict__ W, lp_t* __restrict__ Wt, int K, int nt, int64_t n_chunks) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_chunks) return;
  const int lane = (int)(idx & 63);
  const int64_t piece = idx >> 6;
  const int per_step = 2 * nt, nd = K >> 6;
  const int req = (int)(piece % per_step);
  const int64_t r2 = piece / per_step;
  const int ks = (int)(r2 % nd);
  const int64_t wg = r2 / nd;
  const int t = req >> 1, h = req & 1;
  const int row16 = h * 8 + (lane >> 3);
  const int64_t row = wg * 16 * nt + t * 16 + row16;
  const int chunk = (lane & 7) ^ ((row16 >> 1) & 7);          // the source-side swizzle of gemm_skinny_ring_kernel's requests
  *(lpx8*)(Wt + idx * 8) = *(const lpx8*)(W + row * K + ks * 64 + chunk * 8);
}

#ifdef VSTAR_LP_F16
// ------------------------------------------------ int8 weight-only decode: quantiser, tile-major image ------------------------
// One workgroup per row of W [rows, K]: pass 1 the row's absolute maximum, pass 2 q = clamp(rint(w / s), +-127) with
// s = amax / 127 (both divides correctly rounded; s = 1 for an all-zero row, so padding rows give q = 0, s = 1).  What (nullable,
// may alias W, hence no __restrict__ on either: a thread reads its 8 elements before it writes them) = fp16(float(q) * s), the
// value the tile kernels then see.
__global__ __launch_bounds__(256) void quantize_rows_w8_kernel(const lp_t* W, int K, int8_t* __restrict__ q,
                                                               float* __restrict__ scale, lp_t* What) {
  __shared__ float part[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const lp_t* wr = W + (int64_t)row * K;
  float a = 0.f;
  for (int v = tid; v * 8 < K; v += 256) {
    const lpx8 t = *(const lpx8*)(wr + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(lp2f((lp_t)t[e])));
  }
  a = wave_max(a);
  if ((tid & 63) == 0) part[tid >> 6] = a;
  __syncthreads();
  a = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  const float sc = a == 0.f ? 1.0f : __fdiv_rn(a, 127.0f);
  if (tid == 0) scale[row] = sc;
  for (int v = tid; v * 8 < K; v += 256) {
    const lpx8 t = *(const lpx8*)(wr + v * 8);
    u32x2 packed = {0u, 0u};
    lpx8 back;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float r = rintf(__fdiv_rn(lp2f((lp_t)t[e]), sc));
      r = fminf(fmaxf(r, -127.f), 127.f);
      const int qi = (int)r;
      packed[e >> 2] |= (unsigned)(qi & 0xff) << ((e & 3) * 8);
      back[e] = (short)f2lp((float)qi * sc);
    }
    *(u32x2*)(q + (int64_t)row * K + v * 8) = packed;
    if (What) *(lpx8*)(What + (int64_t)row * K + v * 8) = back;
  }
}

// one thread per 16-byte chunk of the tile-major int8 image (see GemmParams::Wq_tiled)
__global__ void skinny_tile_pack_w8_kernel(const int8_t* __restrict__ Wq, int8_t* __restrict__ Wt, int K, int nt, int64_t n_chunks) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_chunks) return;
  const int lane = (int)(idx & 63);
  const int64_t piece = idx >> 6;
  const int nd = K >> 6;
  const int t = (int)(piece % nt);
  const int64_t r2 = piece / nt;
  const int ks = (int)(r2 % nd);
  const int64_t wg = r2 / nd;
  const int row16 = lane >> 2;
  const int64_t row = wg * 16 * nt + t * 16 + row16;
  const int chunk = (lane & 3) ^ ((row16 >> 2) & 3);          // the source-side swizzle of the W8 ring kernel's requests
  *(u32x4*)(Wt + idx * 16) = *(const u32x4*)(Wq + row * K + ks * 64 + chunk * 16);
}

// ------------------------------------------------ int4 group-scaled weight-only decode: quantiser ------------------------
// One workgroup per row of W [rows, K], K % 128 == 0.  A thread holds 8 consecutive elements = one word of the image; the 16
// threads of a 128-element group are 16 consecutive lanes of one wave (K / 8 is a multiple of 16, so a group is wholly inside the
// loop or wholly outside).  Pass 1: the group's absolute maximum over those lanes, s = min(fp16(a / 7), 9352), 1 when that is 0.
// Pass 2, from the same registers: q = clamp(rint(w / s), +-7), the word of offset nibbles (element e in nibble (e >> 1) +
// 4 (e & 1)), and What = fp16(q) * s as one fp16 multiply — the product w4_to_f16x8 feeds the MFMAs.  What may alias W (no
// __restrict__ on either): a thread reads its 8 elements before it writes them and nobody else reads them.
__global__ __launch_bounds__(256) void quantize_groups_w4_kernel(const lp_t* W, int K, uint32_t* __restrict__ q,
                                                                 lp_t* __restrict__ scale, lp_t* What) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const lp_t* wr = W + (int64_t)row * K;
  for (int v = tid; v * 8 < K; v += 256) {
    const lpx8 t = *(const lpx8*)(wr + v * 8);
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(lp2f((lp_t)t[e])));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 16));
    _Float16 sh = (_Float16)__fdiv_rn(a, 7.0f);
    if (sh > (_Float16)9352.0f) sh = (_Float16)9352.0f;
    if (sh == (_Float16)0.0f) sh = (_Float16)1.0f;
    const float sc = (float)sh;
    if ((tid & 15) == 0) scale[(int64_t)row * (K >> 7) + (v >> 4)] = __builtin_bit_cast(unsigned short, sh);
    unsigned word = 0u;
    lpx8 back;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float r = rintf(__fdiv_rn(lp2f((lp_t)t[e]), sc));
      r = fminf(fmaxf(r, -7.f), 7.f);
      const int qi = (int)r;
      word |= (unsigned)(qi + 8) << (4 * ((e >> 1) + 4 * (e & 1)));
      back[e] = (short)__builtin_bit_cast(unsigned short, (_Float16)((_Float16)qi * sh));
    }
    q[(int64_t)row * (K >> 3) + v] = word;
    if (What) *(lpx8*)(What + (int64_t)row * K + v * 8) = back;
  }
}

// one thread per lane of a slot of the tile-major int4 image (see GemmParams::Wq4_tiled): its four words, and (lanes 0..15) its row's
// two scales.  Halves past the end of K (a wave with an odd count of double steps, or none) hold q = 0 (u = 8) and s = 1; the
// kernel never reads them.
__global__ void skinny_tile_pack_w4_kernel(const uint32_t* __restrict__ q, const lp_t* __restrict__ scale, char* __restrict__ Wt,
                                           int K, int nt, int64_t n_threads) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_threads) return;
  const int lane = (int)(idx & 63), fr = lane & 15, g = lane >> 4;
  const int64_t slot = idx >> 6;
  const int nd = K >> 6, npair = w4_tile_pairs(K);
  const int t = (int)(slot % nt);
  const int64_t r = slot / nt;
  const int w = (int)(r % SK_WAVES);
  const int64_t r2 = r / SK_WAVES;
  const int j = (int)(r2 % npair);
  const int64_t wg = r2 / npair;
  const int64_t row = wg * 16 * nt + t * 16 + fr;
  u32x4 words;
  unsigned sc = 0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int ds = w + 16 * j + 8 * h;
    const bool in = ds < nd;
    words[2 * h] = in ? q[row * (K >> 3) + ds * 8 + g] : 0x88888888u;
    words[2 * h + 1] = in ? q[row * (K >> 3) + ds * 8 + 4 + g] : 0x88888888u;
    sc |= (unsigned)(in ? scale[row * (K >> 7) + (ds >> 1)] : (lp_t)0x3C00) << (16 * h);
  }
  char* sl = Wt + slot * W4_SLOT;
  *(u32x4*)(sl + lane * 16) = words;
  if (g == 0) *(unsigned*)(sl + 1024 + fr * 4) = sc;
}
#endif

template <int EPI, bool OUT_F32, bool W8 = false>
hipError_t launch_skinny_ring(const GemmParams& p0, hipStream_t s) {
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  constexpr int lds = SK_WAVES * SKR_WAVE_BYTES;
  GemmParams p = p0;
  if (p.N % (16 * NT)) p.W_tiled = nullptr, p.Wq_tiled = nullptr;    // whole 16 NT-row tiles only
  const int blocks = (p.N + 16 * NT - 1) / (16 * NT);
  static bool attr_done[2] = {false, false};                   // (per instantiation: the W8 forms keep their own)
  const int nm = p.norm_w ? 1 : 0;
  if (!attr_done[nm]) {
    const void* k = nm ? (const void*)gemm_skinny_ring_kernel<EPI, OUT_F32, true, W8> : (const void*)gemm_skinny_ring_kernel<EPI, OUT_F32, false, W8>;
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_done[nm] = true;
  }
  if (nm) hipLaunchKernelGGL((gemm_skinny_ring_kernel<EPI, OUT_F32, true, W8>), dim3(blocks), dim3(SK_WAVES * 64), lds, s, p);
  else hipLaunchKernelGGL((gemm_skinny_ring_kernel<EPI, OUT_F32, false, W8>), dim3(blocks), dim3(SK_WAVES * 64), lds, s, p);
  return hipGetLastError();
}

template <int EPI, bool OUT_F32, int WQ = 0>
hipError_t launch_skinny(const GemmParams& p0, hipStream_t s) {
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  GemmParams p = p0;
  if (p.N % (16 * NT)) p.Wq4_tiled = nullptr;                   // whole 16 NT-row tiles only, like the ring's images
  const int blocks = (p.N + 16 * NT - 1) / (16 * NT);
  const int mt = (p.M + 15) / 16;
  // M <= 8 (decode steps of up to 8 sequences; 7 with the fused norm): the LDS-ring variant, bit-identical (VSTAR_SKINNY_RING=0: the register-streaming kernel, A/B and tests);
  // the W rows it reads are padded to 256, so whole 16-row tiles exist for every workgroup
  static const bool ring = [] { const char* e = getenv("VSTAR_SKINNY_RING"); return !e || atoi(e) != 0; }();
  // (WQ == 4: there is no W4 ring, the register kernel below serves every M <= 64 — bit-identical)
  if constexpr (WQ != 4)
    if (ring && p.M <= (p.norm_w ? 7 : 8) && p.K >= 512 && p.tile_force != -1) return launch_skinny_ring<EPI, OUT_F32, WQ == 8>(p, s);   // tile_force -1: tests
  switch (mt) {
    case 1: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 1, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    case 2: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 2, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    case 3: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 3, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    case 4: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 4, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

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
// KV-cache formats (KvFormat, kernels.hpp) as the template parameter KVF of every kernel that touches the cache:
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
      o1[e] = (short)f2lp(rlp(a * cs) + rlp(-b * si));
      o2[e] = (short)f2lp(rlp(b * cs) + rlp(a * si));
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
template <bool ANC, class T>
__device__ __forceinline__ const T* kv_row(const T* head0, const T* pre, const T* own, const int32_t* arow, int j, int past,
                                           int64_t slot_stride) {
  constexpr int D = 128;
  if constexpr (ANC) return head0 + (int64_t)arow[j] * slot_stride + (int64_t)j * D;
  else return (j < past ? pre : own) + (int64_t)j * D;
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
  cell_t* kown = (cell_t*)kc + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* kpre = (const cell_t*)kc + (int64_t)seq_prefix[seq] * slot_stride + (int64_t)h * ctx * D;
  cell_t* vown = (cell_t*)vc + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* vpre = (const cell_t*)vc + (int64_t)seq_prefix[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* kh0 = (const cell_t*)kc + (int64_t)h * ctx * D;
  const cell_t* vh0 = (const cell_t*)vc + (int64_t)h * ctx * D;
  const int32_t* arow = ANC ? anc + (int64_t)seq_kv[seq] * ctx : nullptr;
  float* qs = dyn;
  float* sc = dyn + D;
  const lp_t* rowp = qkv + (int64_t)r * (3 * H * D) + h * D;
  if (FUSED) {
    if (tid < 128) {                         // rotate-half RoPE with HF's rounding points: tid 0-63 q pairs, 64-127 k pairs
      const int which = tid >> 6, d = tid & 63;
      const lp_t* base = rowp + which * (H * D);
      const float x1 = lp2f(base[d]), x2 = lp2f(base[d + 64]);
      const float cs = lp2f(cos_sin[(int64_t)pos * D + d]), si = lp2f(cos_sin[(int64_t)pos * D + 64 + d]);
      const lp_t o1 = f2lp(rlp(x1 * cs) + rlp(-x2 * si)), o2 = f2lp(rlp(x2 * cs) + rlp(x1 * si));
      if (which == 0) {
        qs[d] = lp2f(o1);
        qs[d + 64] = lp2f(o2);
      } else if constexpr (KVF == 0) {
        own_k[d] = lp2f(o1);
        own_k[d + 64] = lp2f(o2);
        kown[(int64_t)pos * D + d] = o1;
        kown[(int64_t)pos * D + d + 64] = o2;
      } else {                                // the whole of wave 1: 32 lanes per block
        const int64_t own_off = (int64_t)seq_kv[seq] * slot_stride + ((int64_t)h * ctx + pos) * D;
        own_k[d] = kv8_put<KVF>(kc, ks, own_off + d, lp2f(o1));
        own_k[d + 64] = kv8_put<KVF>(kc, ks, own_off + d + 64, lp2f(o2));
      }
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
  for (int j0 = 0; j0 < nkc; j0 += 64) {
    KvFrag<KVF> kv8[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 16 + grp;
      kv8[u] = kv_frag_zero<KVF>();
      if (j < nkc)
        kv8[u] = kv_frag_load<KVF>(kv_row<ANC>(kh0, kpre, (const cell_t*)kown, arow, j, past, slot_stride), (const cell_t*)kc, ks, l16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 16 + grp;
      float a = 0.f, kx[8];
      kv_frag_f32<KVF>(kv8[u], l16, kx);
#pragma unroll
      for (int e = 0; e < 8; ++e) a += qv[e] * kx[e];
      a += __shfl_xor(a, 8, 64);
      a += __shfl_xor(a, 4, 64);
      a += __shfl_xor(a, 2, 64);
      a += __shfl_xor(a, 1, 64);
      if (j < nkc) {
        const float sv = rlp(rlp(a) / inv_scale);    // HF: matmul output in the storage type, then / sqrt(head_dim)
        if (l16 == 0) sc[j] = sv;
        mx = fmaxf(mx, sv);
      }
    }
  }
  if (FUSED && grp == 0) {                     // the row's own key, from LDS
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a += qv[e] * own_k[l16 * 8 + e];
    a += __shfl_xor(a, 8, 64);
    a += __shfl_xor(a, 4, 64);
    a += __shfl_xor(a, 2, 64);
    a += __shfl_xor(a, 1, 64);
    const float sv = rlp(rlp(a) / inv_scale);
    if (l16 == 0) sc[pos] = sv;
    mx = fmaxf(mx, sv);
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
  for (int j0 = grp; j0 < nkc; j0 += 64) {
    KvFrag<KVF> v8[4];
    float pr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 16;
      v8[u] = kv_frag_zero<KVF>();
      pr[u] = 0.f;
      if (j < nkc) {
        v8[u] = kv_frag_load<KVF>(kv_row<ANC>(vh0, vpre, (const cell_t*)vown, arow, j, past, slot_stride), (const cell_t*)vc, vs, l16);
        pr[u] = rlp(sc[j] * inv);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float vx[8];
      kv_frag_f32<KVF>(v8[u], l16, vx);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += pr[u] * vx[e];
    }
  }
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
  cell_t* kown = (cell_t*)kc + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* kpre = (const cell_t*)kc + (int64_t)seq_prefix[seq] * slot_stride + (int64_t)h * ctx * D;
  cell_t* vown = (cell_t*)vc + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* kh0 = (const cell_t*)kc + (int64_t)h * ctx * D;
  const int32_t* arow = ANC ? anc + (int64_t)seq_kv[seq] * ctx : nullptr;
  const lp_t* rowp = qkv + (int64_t)r * (3 * H * D) + h * D;
  const bool last = p == SPLIT_P - 1;
  if (tid < 128) {                           // rotate-half RoPE with HF's rounding points: tid 0-63 q pairs, 64-127 k pairs
    const int which = tid >> 6, d = tid & 63;
    if (which == 0 || last) {
      const lp_t* base = rowp + which * (H * D);
      const float x1 = lp2f(base[d]), x2 = lp2f(base[d + 64]);
      const float cs = lp2f(cos_sin[(int64_t)pos * D + d]), si = lp2f(cos_sin[(int64_t)pos * D + 64 + d]);
      const lp_t o1 = f2lp(rlp(x1 * cs) + rlp(-x2 * si)), o2 = f2lp(rlp(x2 * cs) + rlp(x1 * si));
      if (which == 0) {
        qs[d] = lp2f(o1);
        qs[d + 64] = lp2f(o2);
      } else if constexpr (KVF == 0) {
        own_k[d] = lp2f(o1);
        own_k[d + 64] = lp2f(o2);
        kown[(int64_t)pos * D + d] = o1;
        kown[(int64_t)pos * D + d + 64] = o2;
      } else {                                // the whole of wave 1: 32 lanes per block
        const int64_t own_off = (int64_t)seq_kv[seq] * slot_stride + ((int64_t)h * ctx + pos) * D;
        own_k[d] = kv8_put<KVF>(kc, ks, own_off + d, lp2f(o1));
        own_k[d + 64] = kv8_put<KVF>(kc, ks, own_off + d + 64, lp2f(o2));
      }
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
  for (int j0 = j_lo; j0 < j_hi; j0 += 64) {
    KvFrag<KVF> kv8[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 16 + grp;
      kv8[u] = kv_frag_zero<KVF>();
      if (j < j_hi)
        kv8[u] = kv_frag_load<KVF>(kv_row<ANC>(kh0, kpre, (const cell_t*)kown, arow, j, past, slot_stride), (const cell_t*)kc, ks, l16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 16 + grp;
      float a = 0.f, kx[8];
      kv_frag_f32<KVF>(kv8[u], l16, kx);
#pragma unroll
      for (int e = 0; e < 8; ++e) a += qv[e] * kx[e];
      a += __shfl_xor(a, 8, 64);
      a += __shfl_xor(a, 4, 64);
      a += __shfl_xor(a, 2, 64);
      a += __shfl_xor(a, 1, 64);
      if (j < j_hi) {
        const float sv = rlp(rlp(a) / inv_scale);    // HF: matmul output in the storage type, then / sqrt(head_dim)
        if (l16 == 0) { dyn[j - j_lo] = sv; gsc[j] = sv; }
        mx = fmaxf(mx, sv);
      }
    }
  }
  int n_loc = j_hi - j_lo;
  if (last) {                                  // the row's own key, from LDS
    if (grp == 0) {
      float a = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) a += qv[e] * own_k[l16 * 8 + e];
      a += __shfl_xor(a, 8, 64);
      a += __shfl_xor(a, 4, 64);
      a += __shfl_xor(a, 2, 64);
      a += __shfl_xor(a, 1, 64);
      const float sv = rlp(rlp(a) / inv_scale);
      if (l16 == 0) { dyn[n_loc] = sv; gsc[pos] = sv; }
      mx = fmaxf(mx, sv);
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
  const cell_t* vown = (const cell_t*)vc + (int64_t)seq_kv[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* vpre = (const cell_t*)vc + (int64_t)seq_prefix[seq] * slot_stride + (int64_t)h * ctx * D;
  const cell_t* vh0 = (const cell_t*)vc + (int64_t)h * ctx * D;
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
  for (int j0 = j_lo + grp; j0 < j_hi; j0 += 64) {
    KvFrag<KVF> v8[4];
    float pr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + u * 16;
      v8[u] = kv_frag_zero<KVF>();
      pr[u] = 0.f;
      if (j < j_hi) {
        v8[u] = kv_frag_load<KVF>(kv_row<ANC>(vh0, vpre, vown, arow, j, past, slot_stride), (const cell_t*)vc, vs, l16);
        pr[u] = rlp(__expf(gsc[j] - M) * inv);     // probabilities rounded to the storage type (HF .to(query.dtype))
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float vx[8];
      kv_frag_f32<KVF>(v8[u], l16, vx);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += pr[u] * vx[e];
    }
  }
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

bool gemm_skinny_eligible(const GemmParams& p) {
  return p.M > 0 && p.M <= 64 && p.a_group <= 0 && p.c_group <= 0 && p.K % 64 == 0 && (p.lda % 8) == 0;
}

hipError_t skinny_pack_tiles(const lp_t* W, lp_t* Wt, int n_rows, int K, int nt, hipStream_t s) {
  if (n_rows <= 0 || K <= 0 || K % 64 || (nt != 1 && nt != 2) || n_rows % (16 * nt)) return hipErrorInvalidValue;
  const int64_t n_chunks = (int64_t)n_rows * K / 8;
  hipLaunchKernelGGL(skinny_tile_pack_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, s, W, Wt, K, nt, n_chunks);
  return hipGetLastError();
}

#ifdef VSTAR_LP_F16
hipError_t quantize_rows_w8(const lp_t* W, int rows, int K, int8_t* q, float* scale, lp_t* What, hipStream_t s) {
  if (!W || !q || !scale || rows <= 0 || K <= 0 || K % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantize_rows_w8_kernel, dim3(rows), dim3(256), 0, s, W, K, q, scale, What);
  return hipGetLastError();
}

hipError_t skinny_pack_tiles_w8(const int8_t* Wq, int8_t* Wt, int n_rows, int K, int nt, hipStream_t s) {
  if (n_rows <= 0 || K <= 0 || K % 64 || (nt != 1 && nt != 2) || n_rows % (16 * nt)) return hipErrorInvalidValue;
  const int64_t n_chunks = (int64_t)n_rows * K / 16;
  hipLaunchKernelGGL(skinny_tile_pack_w8_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, s, Wq, Wt, K, nt, n_chunks);
  return hipGetLastError();
}

size_t skinny_tiles_w4_bytes(int n_rows, int K, int nt) {
  return (size_t)(n_rows / (16 * nt)) * w4_tile_pairs(K) * SK_WAVES * nt * W4_SLOT;
}

hipError_t skinny_pack_tiles_w4(const uint32_t* q, const lp_t* scale, void* Wt, int n_rows, int K, int nt, hipStream_t s) {
  if (!q || !scale || !Wt || n_rows <= 0 || K <= 0 || K % 128 || (nt != 1 && nt != 2) || n_rows % (16 * nt)) return hipErrorInvalidValue;
  const int64_t n_threads = (int64_t)(skinny_tiles_w4_bytes(n_rows, K, nt) / W4_SLOT) * 64;
  hipLaunchKernelGGL(skinny_tile_pack_w4_kernel, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, s, q, scale, (char*)Wt, K, nt,
                     n_threads);
  return hipGetLastError();
}

hipError_t quantize_groups_w4(const lp_t* W, int rows, int K, uint32_t* q, lp_t* scale, lp_t* What, hipStream_t s) {
  if (!W || !q || !scale || rows <= 0 || K <= 0 || K % 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(quantize_groups_w4_kernel, dim3(rows), dim3(256), 0, s, W, K, q, scale, What);
  return hipGetLastError();
}
#endif

hipError_t gemm_skinny_lp(const GemmParams& p, int epilogue, bool out_f32, hipStream_t s) {
  if (!gemm_skinny_eligible(p)) return hipErrorInvalidValue;
  if (p.Wq4) {             // int4 group-scaled weights (GemmParams::Wq4): fp16 build, 16-bit output, whole groups of 128
#ifdef VSTAR_LP_F16
    if (p.Wq || !p.wq4_scale || out_f32 || p.K % 128) return hipErrorInvalidValue;
    switch (epilogue) {
      case VSTAR_EPI_NONE: return launch_skinny<VSTAR_EPI_NONE, false, 4>(p, s);
      case VSTAR_EPI_QUICK_GELU: return launch_skinny<VSTAR_EPI_QUICK_GELU, false, 4>(p, s);
      case VSTAR_EPI_GELU: return launch_skinny<VSTAR_EPI_GELU, false, 4>(p, s);
      case VSTAR_EPI_RELU: return launch_skinny<VSTAR_EPI_RELU, false, 4>(p, s);
      case VSTAR_EPI_SILU_MUL: return launch_skinny<VSTAR_EPI_SILU_MUL, false, 4>(p, s);
    }
#endif
    return hipErrorInvalidValue;
  }
  if (p.Wq) {              // int8 weights (GemmParams::Wq): fp16 build, 16-bit output
#ifdef VSTAR_LP_F16
    if (!p.wq_scale || out_f32) return hipErrorInvalidValue;
    switch (epilogue) {
      case VSTAR_EPI_NONE: return launch_skinny<VSTAR_EPI_NONE, false, 8>(p, s);
      case VSTAR_EPI_QUICK_GELU: return launch_skinny<VSTAR_EPI_QUICK_GELU, false, 8>(p, s);
      case VSTAR_EPI_GELU: return launch_skinny<VSTAR_EPI_GELU, false, 8>(p, s);
      case VSTAR_EPI_RELU: return launch_skinny<VSTAR_EPI_RELU, false, 8>(p, s);
      case VSTAR_EPI_SILU_MUL: return launch_skinny<VSTAR_EPI_SILU_MUL, false, 8>(p, s);
    }
#endif
    return hipErrorInvalidValue;
  }
#define SK_CASE(E)                                                                   \
  case E:                                                                            \
    return out_f32 ? launch_skinny<E, true>(p, s) : launch_skinny<E, false>(p, s);
  switch (epilogue) {
    SK_CASE(VSTAR_EPI_NONE)
    SK_CASE(VSTAR_EPI_QUICK_GELU)
    SK_CASE(VSTAR_EPI_GELU)
    SK_CASE(VSTAR_EPI_RELU)
    SK_CASE(VSTAR_EPI_SILU_MUL)
  }
#undef SK_CASE
  return hipErrorInvalidValue;
}

hipError_t embed_rows(const int32_t* src, const lp_t* table, int vocab, const lp_t* feats, int64_t n_feat_rows, lp_t* x, int R,
                      int C, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  const int64_t n = (int64_t)R * (C / 8);
  hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, table, vocab, feats,
                     n_feat_rows, x, R, C);
  return hipGetLastError();
}

// a valid KvFormat of this build: formats beyond fp16 exist in the fp16 instantiation only, KV_FMT_MXFP8 needs its scale arrays
static bool kv_format_ok(const KvFormat& f) {
#ifdef VSTAR_LP_F16
  return f.fmt == KV_FMT_F16 || f.fmt == KV_FMT_MXFP8_EMU || (f.fmt == KV_FMT_MXFP8 && f.ks && f.vs);
#else
  return f.fmt == KV_FMT_F16;
#endif
}

// KV_DISPATCH(fmt, CALL): CALL with the constant KVF = the runtime format fmt (the format-0 instantiation is the only one of
// the bf16 build)
#ifdef VSTAR_LP_F16
#define KV_DISPATCH(fmt, CALL)                          \
  switch (fmt) {                                        \
    case KV_FMT_MXFP8: { constexpr int KVF = 1; CALL; break; }      \
    case KV_FMT_MXFP8_EMU: { constexpr int KVF = 2; CALL; break; }  \
    default: { constexpr int KVF = 0; CALL; break; }    \
  }
#else
#define KV_DISPATCH(fmt, CALL) { constexpr int KVF = 0; CALL; }
#endif

hipError_t rope_kv_append(lp_t* qkv, const lp_t* cos_sin, const int32_t* row_pos, const int32_t* row_slot, lp_t* kc, lp_t* vc,
                          int64_t slot_stride, int ctx, int R, int H, hipStream_t s, const KvFormat& kvf) {
  if (!kv_format_ok(kvf)) return hipErrorInvalidValue;
  if (R <= 0) return hipSuccess;
  const int64_t n = (int64_t)R * 3 * H * 8;
  KV_DISPATCH(kvf.fmt, hipLaunchKernelGGL(rope_kv_append_kernel<KVF>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, qkv, cos_sin,
                                          row_pos, row_slot, kc, vc, slot_stride, ctx, R, H, kvf.ks, kvf.vs));
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

template <bool ANC, int KVF>
static hipError_t cached_attention_t(const lp_t* qkv, lp_t* kc, lp_t* vc, const int32_t* row_seq, const int32_t* row_pos,
                                     const int32_t* seq_kv, const int32_t* seq_prefix, const int32_t* seq_past, const lp_t* fused_cos_sin,
                                     lp_t* out, int R, int H, int ctx, int64_t slot_stride, int max_keys, hipStream_t s, void* split_ws,
                                     int split_max_rows, const int32_t* anc, uint8_t* ks, uint8_t* vs) {
  static const bool split_on = [] { const char* v = getenv("VSTAR_DECODE_SPLIT_KV"); return !v || atoi(v) != 0; }();
  // decode steps of few sequences: P partitions per (row, head) so that the K / V streams of a head run on 8 CUs instead of one
  if (split_on && fused_cos_sin && split_ws && R <= split_max_rows && R * H <= 128 && max_keys >= 256) {
    const size_t rh = (size_t)split_max_rows * H;
    float* ws_scores = (float*)split_ws;
    float* ws_stats = ws_scores + rh * ctx;
    float* ws_opart = ws_stats + rh * SPLIT_P * 2;
    int* ws_cnt = (int*)(ws_opart + rh * SPLIT_P * 128);
    const int span = ((((max_keys + SPLIT_P - 1) / SPLIT_P) + 63) & ~63) + 1;
    hipLaunchKernelGGL((cached_attn_split_scores_kernel<ANC, KVF>), dim3(R, H, SPLIT_P), dim3(256), (size_t)span * sizeof(float), s, qkv,
                       kc, vc, row_seq, row_pos, seq_kv, seq_prefix, seq_past, fused_cos_sin, ws_scores, ws_stats, H, ctx, slot_stride,
                       sqrtf(128.0f), anc, ks, vs);
    hipLaunchKernelGGL((cached_attn_split_pv_kernel<ANC, KVF>), dim3(R, H, SPLIT_P), dim3(256), 0, s, vc, row_seq, row_pos, seq_kv,
                       seq_prefix, seq_past, ws_scores, ws_stats, ws_opart, ws_cnt, out, H, ctx, slot_stride, anc, vs);
    return hipGetLastError();
  }
  const size_t lds = (size_t)(128 + max_keys) * sizeof(float);
  if (lds > 40 * 1024) return hipErrorInvalidValue;
  if (fused_cos_sin)
    hipLaunchKernelGGL((cached_attn_kernel<true, ANC, KVF>), dim3(R, H), dim3(256), lds, s, qkv, kc, vc, row_seq, row_pos, seq_kv,
                       seq_prefix, seq_past, fused_cos_sin, out, H, ctx, slot_stride, sqrtf(128.0f), anc, ks, vs);
  else
    hipLaunchKernelGGL((cached_attn_kernel<false, ANC, KVF>), dim3(R, H), dim3(256), lds, s, qkv, kc, vc, row_seq, row_pos, seq_kv,
                       seq_prefix, seq_past, fused_cos_sin, out, H, ctx, slot_stride, sqrtf(128.0f), anc, ks, vs);
  return hipGetLastError();
}

hipError_t cached_attention(const lp_t* qkv, lp_t* kc, lp_t* vc, const int32_t* row_seq, const int32_t* row_pos,
                            const int32_t* seq_kv, const int32_t* seq_prefix, const int32_t* seq_past, const lp_t* fused_cos_sin,
                            lp_t* out, int R, int H, int ctx, int64_t slot_stride, int max_keys, hipStream_t s, void* split_ws,
                            int split_max_rows, const int32_t* anc, const KvFormat& kvf) {
  if (!kv_format_ok(kvf)) return hipErrorInvalidValue;
  if (R <= 0) return hipSuccess;
  hipError_t e = hipErrorInvalidValue;
  if (anc) {
    KV_DISPATCH(kvf.fmt, e = (cached_attention_t<true, KVF>(qkv, kc, vc, row_seq, row_pos, seq_kv, seq_prefix, seq_past, fused_cos_sin,
                                                            out, R, H, ctx, slot_stride, max_keys, s, split_ws, split_max_rows, anc,
                                                            kvf.ks, kvf.vs)));
  } else {
    KV_DISPATCH(kvf.fmt, e = (cached_attention_t<false, KVF>(qkv, kc, vc, row_seq, row_pos, seq_kv, seq_prefix, seq_past, fused_cos_sin,
                                                             out, R, H, ctx, slot_stride, max_keys, s, split_ws, split_max_rows, nullptr,
                                                             kvf.ks, kvf.vs)));
  }
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

hipError_t kv_copy_rows(lp_t* kc, lp_t* vc, const int32_t* anc, int dst, int src, int lo, int hi, int layers, int H, int ctx,
                        int64_t slot_stride, int64_t layer_stride, hipStream_t s, const KvFormat& kvf) {
  if (!kv_format_ok(kvf)) return hipErrorInvalidValue;
  if (hi <= lo) return hipSuccess;
  const int64_t n = (int64_t)2 * layers * H * (hi - lo) * 16;
  KV_DISPATCH(kvf.fmt, hipLaunchKernelGGL(kv_copy_rows_kernel<KVF>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kc, vc, anc, dst,
                                          src, lo, hi - lo, H, ctx, slot_stride, layer_stride, n, kvf.ks, kvf.vs));
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
