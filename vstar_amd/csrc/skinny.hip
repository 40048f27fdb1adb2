// skinny.hip — the weight-streaming GEMV family of the decode path (M <= 64 rows; kernels.hpp: gemm_skinny_lp): HBM-bound, the
// weights are read once per call in the format GemmParams::dw names (SkinnyWeights: fp16 / bf16, int8 per row, int4 in groups of 128).
//
//   gemm_skinny_kernel       out[M<=64, N] = A · W^T for decode-sized M: HBM-bound weight streaming.  One workgroup owns 16 (or
//                            16 gate + 16 up) output columns, its 8 waves split K in an interleaved fashion so that the
//                            workgroup as a whole reads 512 contiguous bytes of every W row per step; partial sums meet in LDS.
//   gemm_skinny_ring_kernel  the same arithmetic for M <= 8 with the operands moved through per-wave LDS rings by LDS-DMA requests.
//   skinny_tile_pack_*       the tile-major images of the three weight formats; quantize_rows_w8 / quantize_groups_w4: the quantisers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <type_traits>
#include "common.hpp"
#include "kernels.hpp"
#include "gemm_epilogue.hpp"

namespace VS_NS {

namespace {

// ------------------------------------------------ skinny GEMM ------------------------------------------------
// Operands as in the big kernels: W fragment is the MFMA A operand (16 output columns x 32 k), the activation fragment
// the B operand (16 rows x 32 k); lane (fr = lane%16, g = lane/16) loads 16 bytes at k = ks*32 + g*8 of W row / A row fr.
// The accumulator lane then owns output row fr, columns 4g..4g+3 — the layout gemm_epilogue_store expects.
constexpr int SK_WAVES = 8;
constexpr int SKR_WAVE_BYTES = 10240;      // gemm_skinny_ring_kernel: LDS ring per wave

// W8 forms (SKINNY_W_INT8): the lane's 8 k-elements of a W row are 8 bytes of int8.  Eight int8 -> eight fp16,
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

// W4 form (SKINNY_W_INT4G128): the lane's 8 k-elements of a W row are ONE 32-bit word of offset nibbles u = q + 8,
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

// The W4 tile-major image (SKINNY_W_INT4G128's `tiled`): per workgroup, pair j of own double steps and wave w one slot per tile.
constexpr int W4_SLOT = 1024 + 64;          // 64 lanes x 4 words | 16 rows x 2 fp16 scales
__host__ __device__ __forceinline__ int w4_tile_pairs(int K) { return (((K >> 6) + SK_WAVES - 1) / SK_WAVES + 1) >> 1; }

// WQ = GemmParams::dw.fmt: 0 = fp16 / bf16 weights (GemmParams::W), 8 = the W8 form, 4 = the W4 form
template <int EPI, bool OUT_F32, int MT, int WQ = 0>
__global__ __launch_bounds__(SK_WAVES * 64) void gemm_skinny_kernel(const GemmParams p) {
  constexpr bool W8 = WQ == 8, W4 = WQ == 4;
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  __shared__ float red[SK_WAVES][MT][64][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  // the typed views of the weight descriptor (GemmParams::dw) this instantiation reads
  const int8_t* dw_q8 = nullptr; const float* dw_s8 = nullptr;
  const uint32_t* dw_q4 = nullptr; const uint16_t* dw_s4 = nullptr; const void* dw_img4 = nullptr;
  if constexpr (W8) { dw_q8 = (const int8_t*)p.dw.q; dw_s8 = (const float*)p.dw.scale; }
  if constexpr (W4) { dw_q4 = (const uint32_t*)p.dw.q; dw_s4 = (const uint16_t*)p.dw.scale; dw_img4 = p.dw.tiled; }

  const lp_t* wp[NT];
  const int8_t* wq[NT];            // W8: the same row and k offset, one byte per element
  const uint32_t* w4[NT];          // W4: the same row and k offset, one word per 8 elements ...
  const lp_t* s4[NT];              // ... and the row's group scales (a double step of 64 lies inside one group of 128)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    wp[t] = WQ ? nullptr : p.W + (int64_t)(n0 + t * 16 + fr) * p.K + g * 8;
    wq[t] = W8 ? dw_q8 + (int64_t)(n0 + t * 16 + fr) * p.K + g * 8 : nullptr;
    w4[t] = W4 ? dw_q4 + (int64_t)(n0 + t * 16 + fr) * (p.K >> 3) + g : nullptr;
    s4[t] = W4 ? dw_s4 + (int64_t)(n0 + t * 16 + fr) * (p.K >> 7) : nullptr;
  }
  // W4, tile-major image (dw.tiled, or null): this wave's slots, pair j of tile t at img + (j * 8 NT + t) * W4_SLOT —
  // the lane's 16 bytes are its four words of its own double steps ds = wave + 16 j and ds + 8, the two scales follow the 1 KiB
  const char* img = (W4 && dw_img4)
      ? (const char*)dw_img4 + ((int64_t)blockIdx.x * w4_tile_pairs(p.K) * SK_WAVES + wave) * (NT * W4_SLOT) + lane * 16 : nullptr;
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
    for (int t = 0; t < NT; ++t) s[t] = w8_scale_cols(s[t], dw_s8, n0 + t * 16 + g * 4);
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
// W8 form (SKINNY_W_INT8): a 16-row weight tile of one double step is 16 x 64 B = 1 KiB = ONE request (lane ->
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
  // the typed views of the weight descriptor (GemmParams::dw) this instantiation reads
  const int8_t* dw_q8 = nullptr; const float* dw_s8 = nullptr; const int8_t* dw_img8 = nullptr; const lp_t* dw_img = nullptr;
  if constexpr (W8) { dw_q8 = (const int8_t*)p.dw.q; dw_s8 = (const float*)p.dw.scale; dw_img8 = (const int8_t*)p.dw.tiled; }
  else dw_img = (const lp_t*)p.dw.tiled;

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
    wsrc8[t] = W8 ? dw_q8 + (int64_t)(n0 + t * 16 + row8) * p.K + ((lane & 3) ^ ((row8 >> 2) & 3)) * 16 : nullptr;
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
  // tile-major weights (dw.tiled): this workgroup's pieces lie back to back, [k-step][t][h] x 1 KiB, already in request order
  const bool tiled = W8 ? dw_img8 != nullptr : dw_img != nullptr;
  const lp_t* wt = (!W8 && tiled) ? dw_img + ((int64_t)blockIdx.x * nd * (2 * NT)) * 512 + lane * 8 : nullptr;
  // (W8, dw.tiled: [k-step][t] x 1 KiB)
  const int8_t* wt8 = (W8 && tiled) ? dw_img8 + ((int64_t)blockIdx.x * nd * NT) * 1024 + lane * 16 : nullptr;
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
    for (int t = 0; t < NT; ++t) s[t] = w8_scale_cols(s[t], dw_s8, n0 + t * 16 + g * 4);
  }
  if (EPI == VSTAR_EPI_SILU_MUL) gemm_epilogue_store<EPI, OUT_F32>(p, fr, n0 / 2 + g * 4, n_out, s[0], s[NT - 1]);
  else gemm_epilogue_store<EPI, OUT_F32>(p, fr, n0 + g * 4, n_out, s[0], s[0]);
}

// one thread per 16-byte chunk of the tile-major image (see SKINNY_W_F16)
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

// one thread per 16-byte chunk of the tile-major int8 image (see SKINNY_W_INT8)
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

// one thread per lane of a slot of the tile-major int4 image (see SKINNY_W_INT4G128): its four words, and (lanes 0..15) its row's
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

thread_local int t_last_kernel = 0;          // gemm_skinny_last_kernel()

template <int EPI, bool OUT_F32, bool W8 = false>
hipError_t launch_skinny_ring(const GemmParams& p0, hipStream_t s) {
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  constexpr int lds = SK_WAVES * SKR_WAVE_BYTES;
  GemmParams p = p0;
  if (p.N % (16 * NT)) p.dw.tiled = nullptr;                  // whole 16 NT-row tiles only
  const int blocks = (p.N + 16 * NT - 1) / (16 * NT);
  static bool attr_done[2] = {false, false};                   // (per instantiation: the W8 forms keep their own)
  const int nm = p.norm_w ? 1 : 0;
  if (!attr_done[nm]) {
    const void* k = nm ? (const void*)gemm_skinny_ring_kernel<EPI, OUT_F32, true, W8> : (const void*)gemm_skinny_ring_kernel<EPI, OUT_F32, false, W8>;
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    attr_done[nm] = true;
  }
  t_last_kernel = 2;
  if (nm) hipLaunchKernelGGL((gemm_skinny_ring_kernel<EPI, OUT_F32, true, W8>), dim3(blocks), dim3(SK_WAVES * 64), lds, s, p);
  else hipLaunchKernelGGL((gemm_skinny_ring_kernel<EPI, OUT_F32, false, W8>), dim3(blocks), dim3(SK_WAVES * 64), lds, s, p);
  return hipGetLastError();
}

template <int EPI, bool OUT_F32, int WQ = 0>
hipError_t launch_skinny(const GemmParams& p0, hipStream_t s) {
  constexpr int NT = (EPI == VSTAR_EPI_SILU_MUL) ? 2 : 1;
  GemmParams p = p0;
  if (p.N % (16 * NT)) p.dw.tiled = nullptr;                    // whole 16 NT-row tiles only, like the ring's images
  const int blocks = (p.N + 16 * NT - 1) / (16 * NT);
  const int mt = (p.M + 15) / 16;
  // M <= 8 (decode steps of up to 8 sequences; 7 with the fused norm): the LDS-ring variant, bit-identical (VSTAR_SKINNY_RING=0: the register-streaming kernel, A/B and tests);
  // the W rows it reads are padded to 256, so whole 16-row tiles exist for every workgroup
  static const bool ring = [] { const char* e = getenv("VSTAR_SKINNY_RING"); return !e || atoi(e) != 0; }();
  // (WQ == 4: there is no W4 ring, the register kernel below serves every M <= 64 — bit-identical)
  if constexpr (WQ != 4)
    if (ring && p.M <= (p.norm_w ? 7 : 8) && p.K >= 512 && p.tile_force != -1) return launch_skinny_ring<EPI, OUT_F32, WQ == 8>(p, s);   // tile_force -1: tests
  if (mt >= 1 && mt <= 4) t_last_kernel = 1;
  switch (mt) {
    case 1: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 1, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    case 2: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 2, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    case 3: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 3, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    case 4: hipLaunchKernelGGL((gemm_skinny_kernel<EPI, OUT_F32, 4, WQ>), dim3(blocks), dim3(SK_WAVES * 64), 0, s, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
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

// the one epilogue switch: WQ != 0 (fp16 build only) has 16-bit output alone
template <int WQ>
static hipError_t skinny_dispatch(const GemmParams& p, int epilogue, bool out_f32, hipStream_t s) {
#define SK_CASE(E)                                                                                     \
  case E:                                                                                              \
    if constexpr (WQ != 0) return launch_skinny<E, false, WQ>(p, s);                                   \
    else return out_f32 ? launch_skinny<E, true>(p, s) : launch_skinny<E, false>(p, s);
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

int gemm_skinny_last_kernel() { return t_last_kernel; }

hipError_t gemm_skinny_lp(const GemmParams& p, int epilogue, bool out_f32, hipStream_t s) {
  t_last_kernel = 0;
  if (!gemm_skinny_eligible(p)) return hipErrorInvalidValue;
  const SkinnyWeights& dw = p.dw;
  if (dw.fmt == SKINNY_W_F16) return skinny_dispatch<0>(p, epilogue, out_f32, s);
#ifdef VSTAR_LP_F16
  // the quantised formats: fp16 build, both images' row-major parts present, 16-bit output; int4 streams whole groups of 128
  if (!dw.q || !dw.scale || out_f32) return hipErrorInvalidValue;
  if (dw.fmt == SKINNY_W_INT8) return skinny_dispatch<8>(p, epilogue, false, s);
  if (dw.fmt == SKINNY_W_INT4G128 && p.K % 128 == 0) return skinny_dispatch<4>(p, epilogue, false, s);
#endif
  return hipErrorInvalidValue;
}

}  // namespace VS_NS
