// kernels.hpp — host-side launch interface of the gfx950 kernels (internal; the public ABI is include/vstar_hip.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "../../include/vstar_hip.h"
#include "common.hpp"

namespace VS_NS {

// What the weight-streaming GEMV (gemm_skinny_lp, skinny.hip) streams as its weight operand: one format tag and the format's
// three device images.
enum {
  // fp16 / bf16 weights: GemmParams::W is read, q and scale are null.
  // tiled (gemm_skinny_ring_kernel only (round 5), or null): a TILE-MAJOR copy of W for the decode GEMV — [N / (16 NT)][K / 64][2 NT]
  // pieces of 1 KiB, each in the lane order of the LDS-DMA request that fetches it (skinny_pack_tiles): a workgroup then streams ONE
  // sequential region of HBM instead of 16 / 32 row streams 2 K bytes apart (tools/probes/stream_layout_probe.hip: gate|up 5.4 -> 7.0 TB/s)
  SKINNY_W_F16 = 0,
  // gemm_skinny_kernel / gemm_skinny_ring_kernel, fp16 build: int8 weights with fp16 activations (W8A16).
  // The weight operand is q [ceil(N/256)*256, K] int8, K-contiguous like W, and scale [ceil(N/256)*256] fp32 one scale per packed
  // row: every MFMA sees fp16(q) (exact: |q| <= 127) in place of W, and the reduced accumulator of column n is multiplied once by
  // scale[n] before gemm_epilogue_store.  W is then not read.
  // tiled (ring kernel, or null): the TILE-MAJOR int8 image, [N / (16 NT)][K / 64][NT] pieces of 1 KiB.  A piece is ONE LDS-DMA
  // request (16 rows x 64 B, where fp16 needs two of 8 rows x 128 B): lane l carries 16 bytes of row l / 4, namely chunk
  // (l % 4) ^ ((row / 4) % 4) of that row's 64 bytes, so that LDS holds row r at r * 64 with its 16-byte chunks swizzled by
  // (r / 4) % 4 and the 8-byte fragment reads of rows r, r + 4, r + 8, r + 12 fall into different banks (skinny_pack_tiles_w8).
  SKINNY_W_INT8 = 8,
  // gemm_skinny_kernel only, fp16 build: int4 group-scaled weights with fp16 activations (W4A16, groups of 128).
  // The weight operand is q [ceil(N/256)*256, K / 8] 32-bit words (eight offset nibbles u = q + 8 each: element e of a word in
  // nibble (e >> 1) + 4 (e & 1)) and scale [ceil(N/256)*256, K / 128] fp16 bits, one scale per row and 128 k (K % 128 == 0).
  // Every MFMA sees fp16(fp16(q) * s), ONE fp16 multiply per weight in registers, in place of W: the kernel is bit-identical to the
  // fp16 kernel on the dequantised weights, there is no post-scale.  W is then not read.
  // tiled (or null): the TILE-MAJOR image, read INSTEAD of q / scale: [N / (16 NT)][pairs][8 waves][NT] slots of 1088 B,
  // pairs = ceil(ceil(K / 64 / 8) / 2).  Slot (j, w, t) belongs to wave w: lane l = fr + 16 g holds at l * 16 its four words of its
  // OWN two consecutive double steps ds = w + 16 j and ds + 8 of row fr of tile t — (ds, k-step 0), (ds, 1), (ds + 8, 0), (ds + 8, 1)
  // — so a wave fetches them with ONE fully coalesced 1-KiB load where the row-major words cost four loads of 16 rows x 16 B; the
  // 64 bytes behind them are the rows' scale pairs (s[ds / 2], s[(ds + 8) / 2]) at 1024 + fr * 4 (skinny_pack_tiles_w4).  Wave
  // ownership of the double steps, and with it the MFMA order, is unchanged.
  SKINNY_W_INT4G128 = 4
};
struct SkinnyWeights { int fmt; const void* q; const void* scale; const void* tiled; };

// Row maps let a GEMM read/write a strided sub-sequence without a gather pass:
//   mapped(r) = (r / group) * gstride + off + r % group      (group <= 0: identity)
struct GemmParams {
  const lp_t* A; int64_t lda; int a_group; int64_t a_gstride; int64_t a_off;
  const lp_t* W;          // [ceil(N/256)*256, K] K-contiguous rows (nn.Linear layout), zero padded; K % 64 == 0
  const lp_t* bias;       // [N] or null
  const lp_t* res; int64_t ldr;   // residual, laid out like C (same row map), or null
  void* C; int64_t ldc; int c_group; int64_t c_gstride; int64_t c_off;
  int M, N, K;
  int debug_flags;   // diagnostics only: bit0 = skip the epilogue's global stores, bit1 = skip the whole epilogue, bit2 = gemm256 without its direct (in-register) epilogue
  // gemm_skinny_lp only: when norm_w != null the rows of A are RMS-normalised on the fly (LlamaRMSNorm: fp32 statistics,
  // rlp(x * rstd), then rlp(norm_w * that)) — bit-identical to rmsnorm_lp followed by the GEMM, one launch less
  const lp_t* norm_w; float norm_eps;
  // gemm256 only (bf16/fp16 output, VSTAR_EPI_NONE): rotate-half RoPE fused into the epilogue of the q|k columns
  // (col < rope_cols, heads of 128): out = rlp(x*cos) + rlp(-/+ partner*sin) with position = row % rope_S and the table
  // rope_cs [rope_S, 128] = cos(64)|sin(64) — the rounding points of rope_kernel, one pass over q,k less
  const lp_t* rope_cs; int rope_S; int rope_cols;
  int rope_R0, rope_Lc;   // grouped sequences (see attn_forward): position of row r >= rope_R0 is rope_Lc + ((r - rope_R0) & 31); 0 = off
  // shared system-prompt prefix (engine.hip::llm_forward): rows [0, rope_tail) are sequences of rope_S rows that START at position
  // rope_pos0 (their first rope_pos0 positions live once, in the rows from rope_tail on: position = row - rope_tail); 0 = off
  int rope_pos0, rope_tail;
  // gemm256 only: W8A8 mode (BASELINE config 5).  a_scale != null => A and W point at OCP fp8 e4m3 bytes (lda / K count
  // fp8 elements, K % 256 == 0), a_scale [M] and w_scale [N] are the per-row / per-output-channel dequantisation factors:
  // C = epilogue((A_q · W_q^T) * a_scale[m] * w_scale[n]).  One v_mfma_scale_f32_16x16x128_f8f6f4 (scales 1.0) replaces two
  // 16x16x32 bf16 MFMAs on the same LDS bytes, i.e. twice the K per K-tile at the same LDS/DMA traffic.
  const float* a_scale; const float* w_scale;
  // RMSNorm folded into the linears (bf16 kernels, llm_forward): `row_scale` [buffer rows] multiplies the accumulators of row r by
  // row_scale[mapped A row r] before bias / activation / RoPE — with the norm's weight folded into W's columns this IS
  // Linear(RMSNorm(x)) without the normalised copy of x.  `sumsq_out` (VSTAR_EPI_NONE, bf16 output): the epilogue also writes,
  // per output row and 64-column span, the sum of squares of the STORED bf16 values to sumsq_out[crow * sumsq_ld + col / 64] —
  // the statistics of the next RMSNorm, produced where the residual stream is written.  Both kernels add in the same fixed
  // order (4+4 columns, pairs of 8-column chunks, 16-column fragments pairwise), so the partials are bit-identical.
  const float* row_scale; float* sumsq_out; int sumsq_ld;
  // LayerNorm folded into the ViT linears (round 4): with stats_sum != 0 the epilogue ALSO writes the plain sum of every span to
  // sumsq_out[crow * sumsq_ld + stats_sum + col / 64] (stats_sum = the number of 64-column spans of a row), same fixed tree; the
  // consumer's row_scale is then 1 / sqrt(var + eps) with var = E[x^2] - E[x]^2 (ln_rstd_partials), its weights are
  // W diag(g) with every row CENTRED over k (ln_fold_weights) — sum_k x_k (w_k - mean w) = sum_k (x_k - mean x) w_k, so no shift
  // term is needed — and its bias is W b_ln + c
  int stats_sum;
  // kernel choice: 0 = the dispatcher decides, 128 / 256 = force that tile (256 fails with hipErrorInvalidValue when the shape
  // is not gemm256_eligible).  Process-wide default for 0 calls: environment VSTAR_GEMM_TILE (A/B runs).
  int tile_force;
  // variant of the 128-row family: 0 = the dispatcher decides (shape, CU count, process default VSTAR_GEMM128_STAGES), 2 / 5 / 6 / 7
  // = that variant for THIS call (GemmPlan::mode values; op-level tests).  Non-zero implies tile_force = 128 (no 256^2 kernel, no
  // ragged-round split); any other value, or a request next to tile_force 256 / GEMM_TILE_4W, rope_cs, a_scale, a_mx or c_mx, fails
  // with hipErrorInvalidValue — never re-routed
  int stages_force;
  // gemm4w only, W8A8 with block-scaled activations (mx.hpp; round 6).  a_mx != null: A holds fp8 bytes whose E8M0
  // block scales (one per row and 32 k, tile-major: mx_scale_offset with m128 = M / 128) are applied inside the MFMA; w_scale as above.
  // c_mx != null (VSTAR_EPI_SILU_MUL): the epilogue writes SiLU(gate) * up as fp8 bytes to (uint8_t*)C (ldc in bytes) and the block
  // scales to c_mx (same layout, consumer K = N / 2) instead of 16-bit values — bit-identical to storing them and running
  // quantize_rows_mx over the result.  Both fail with hipErrorInvalidValue outside gemm4w's domain (gemm_mx_supported).
  const uint8_t* a_mx; uint8_t* c_mx;
  // ... and VSTAR_EPI_NONE with c_mx != null (o_proj / down_proj: residual stream out): C receives the 16-bit rows as usual AND c8
  // [M, ldc8] their block-scaled fp8 copy (scales to c_mx) — the next linear's A operand, whose RMSNorm is folded: its weight into that
  // linear's W, its 1 / rms applied as a_scale (allowed next to a_mx) from the sum-of-squares partials this epilogue writes (sumsq_out).
  uint8_t* c8; int64_t ldc8;
  // gemm_skinny_lp only (the tile kernels never read it): what the skinny kernels stream instead of / next to W
  SkinnyWeights dw;
};
bool gemm_mx_supported(const GemmParams& p, int epilogue);
hipError_t gemm_lp(const GemmParams& p, int epilogue, bool out_f32, hipStream_t s);
// GemmParams::tile_force / gemm_last_tile() value of the 4-wave / AGPR 256 x 256 kernel (gemm4w.hip; "256, 4 waves")
constexpr int GEMM_TILE_4W = 2564;
// whether unforced calls inside gemm4w's domain take it (VSTAR_GEMM4W overrides)
#ifndef GEMM4W_DEFAULT
#define GEMM4W_DEFAULT 1
#endif
// compute units of the current device, rounded down to a multiple of 8 (>= 8); cached per process
int gemm_device_cus();
// What gemm_lp does with a call, as a value.  tile: 0 = nothing to launch, 128 = the 128-row family, 256 = the 8-wave 256^2 kernel,
// GEMM_TILE_4W, 384 = split launch (the leading split_rows rows on the 256^2 kernel `lead` = 256 / GEMM_TILE_4W, the rest on the
// 128-row family).  mode: the variant of the 128-row part — 2 = double buffer, 5 / 6 / 7 = loader-wave ring on the 128 x 128 /
// 128 x 64 / 128 x 256 tile — else 0.  status != hipSuccess: gemm_lp refuses the call, everything else is 0.
struct GemmPlan { hipError_t status; int tile, mode, split_rows, lead; };
// The dispatcher's decision for a device with `cus` compute units: a pure function of its arguments and of the process-wide
// environment defaults — no HIP call, no state, no pointer is dereferenced (vstar_op_gemm_plan: host-only tests of the kernel choice).
GemmPlan gemm_plan(const GemmParams& p, int epilogue, bool out_f32, int cus);
// tile / mode of the plan the last gemm_lp call of THIS thread executed, 0 / 0 when it refused the call (observability for the
// op-level tests: a dispatcher change must not silently move a test onto the other kernel)
int gemm_last_tile();
int gemm_launched_mode();
bool gemm256_eligible(const GemmParams& p);   // true: gemm_lp runs the 256^2 kernel (the only one that honours rope_cs)

// decode-sized GEMM (skinny.hip): M <= 64, identity row maps; same operands/epilogues as gemm_lp
bool gemm_skinny_eligible(const GemmParams& p);
hipError_t gemm_skinny_lp(const GemmParams& p, int epilogue, bool out_f32, hipStream_t s);
// which kernel the last gemm_skinny_lp call of THIS thread launched: 1 = gemm_skinny_kernel (registers), 2 = gemm_skinny_ring_kernel,
// 0 = it refused the call (observability for the op-level tests, like gemm_last_tile())
int gemm_skinny_last_kernel();
// Wt <- tile-major image of the packed row-major W [n_rows][K] for gemm_skinny_ring_kernel (nt = 2 for SiLU(gate)*up weights whose
// rows interleave gate / up in blocks of 16, else 1); n_rows % (16 nt) == 0, K % 64 == 0; Wt holds n_rows * K elements
hipError_t skinny_pack_tiles(const lp_t* W, lp_t* Wt, int n_rows, int K, int nt, hipStream_t s);
#ifdef VSTAR_LP_F16
// ---- int8 weight-only decode (W8A16; fp16 build only: the in-register int8 -> fp16 conversion is exact there) ----
// Per row n of W [rows, K] (fp16): a = max|W[n,:]|, s = a / 127 (one correctly rounded fp32 divide; 1 when a == 0),
// q = clamp(rint(float(W) / s), -127, 127).  What (nullable, may alias W): fp16(float(q) * s).  One workgroup per row.
hipError_t quantize_rows_w8(const lp_t* W, int rows, int K, int8_t* q, float* scale, lp_t* What, hipStream_t s);
// the tile-major int8 image (SKINNY_W_INT8's `tiled`) of the row-major Wq [n_rows][K]; n_rows % (16 nt) == 0, K % 64 == 0
hipError_t skinny_pack_tiles_w8(const int8_t* Wq, int8_t* Wt, int n_rows, int K, int nt, hipStream_t s);
// ---- int4 group-scaled weight-only decode (W4A16; fp16 build only) ----
// Per row n of W [rows, K] (fp16, K % 128 == 0) and group j of 128 k: a = max|W[n, 128 j ..]|, s = min(fp16(float(a) / 7.0f), 9352),
// 1 when that is 0; q = clamp(rint(float(W) / float(s)), -7, 7).  q [rows, K / 8] words (SKINNY_W_INT4G128's `q`), scale [rows, K / 128]
// fp16.  What (nullable, may alias W): fp16(q) * s, one fp16 multiply.  One workgroup per row.
hipError_t quantize_groups_w4(const lp_t* W, int rows, int K, uint32_t* q, lp_t* scale, lp_t* What, hipStream_t s);
// the tile-major int4 image (SKINNY_W_INT4G128's `tiled`) of the row-major q [n_rows][K / 8] and scale [n_rows][K / 128];
// n_rows % (16 nt) == 0, K % 128 == 0; Wt holds skinny_tiles_w4_bytes(n_rows, K, nt) bytes
size_t skinny_tiles_w4_bytes(int n_rows, int K, int nt);
hipError_t skinny_pack_tiles_w4(const uint32_t* q, const lp_t* scale, void* Wt, int n_rows, int K, int nt, hipStream_t s);
#endif

// ---- KV-cached language model + Perceiver resampler (decode.hip) ----
// One layer of the KV cache: K and V as [slot][H][ctx][128] cells, slot_stride cells apart, in the format `fmt`
// (beyond KV_FMT_F16: fp16 build only).
//   KV_FMT_F16        a cell is an lp_t.
//   KV_FMT_MXFP8      a cell is an e4m3 code BYTE — k / v then address bytes with the same element strides — and ks / vs hold the
//                     E8M0 bytes [slot][H][ctx][4] of this layer, one per block of 32 head-dim elements (mx.hpp), at
//                     (cell offset / 32) of their own arrays.
//   KV_FMT_MXFP8_EMU  lp_t cells, every writer storing the round-tripped row: format 1's values through format 0's readers.
enum { KV_FMT_F16 = 0, KV_FMT_MXFP8 = 1, KV_FMT_MXFP8_EMU = 2 };
struct KvLayer {
  int fmt = KV_FMT_F16;
  void *k = nullptr, *v = nullptr;             // cells, untyped: the format decides
  uint8_t *ks = nullptr, *vs = nullptr;        // KV_FMT_MXFP8 only, else null
  int64_t slot_stride = 0;                     // H * ctx * 128
  int H = 0, ctx = 0;
};
// a valid view for this build: formats beyond fp16 exist in the fp16 instantiation only, KV_FMT_MXFP8 needs its scale arrays
bool kv_format_ok(const KvLayer& kv);
// The rows of one call (device arrays): row r is position row_pos[r] (< 0: a padding row, skipped) of sequence row_seq[r] and is
// stored in slot row_slot[r]; sequence i writes slot seq_kv[i] and reads keys [0, seq_past[i]) from slot seq_prefix[i], the rest
// from its own.  anc (nullable): the KV ancestry table of beam search, see kv_anc_mark below.
struct KvRows {
  const int32_t *row_seq = nullptr, *row_pos = nullptr, *row_slot = nullptr;
  const int32_t *seq_kv = nullptr, *seq_prefix = nullptr, *seq_past = nullptr;
  const int32_t* anc = nullptr;
};
// x[r,:] = src[r] >= 0 ? table[src[r]] : (src[r] == INT32_MIN ? 0 : feats[-(src[r]+1)])
hipError_t embed_rows(const int32_t* src, const lp_t* table, int vocab, const lp_t* feats, int64_t n_feat_rows, lp_t* x, int R,
                      int C, hipStream_t s);
// in-place RoPE on q,k of qkv [R, 3*H*128] at rows.row_pos (padding rows are skipped) and K/V rows appended to the cache of slot
// rows.row_slot[r]
hipError_t rope_kv_append(lp_t* qkv, const lp_t* cos_sin, const KvLayer& kv, const KvRows& rows, int R, hipStream_t s);
// causal attention of R new rows against the cache: keys [0, seq_past) come from seq_prefix's slot, the rest from seq_kv's
// (rows.anc given: through the ancestry table).
// fused_cos_sin != null (only when every sequence has exactly ONE new row): the kernel also does rope_kv_append's work for
// its row (RoPE on q,k, K/V appended to the cache) — qkv then holds the raw projection.
// decide_rows > 0: the split-KV decision is the one a step of decide_rows rows would get (the batched cue decode asks for a one-row
// step's, so that a sequence's sums run in the order of its solo decode whatever R is); the workspace must still hold R rows.
hipError_t cached_attention(const lp_t* qkv, const KvLayer& kv, const KvRows& rows, const lp_t* fused_cos_sin, lp_t* out, int R,
                            int max_keys, hipStream_t s, void* split_ws = nullptr, int split_max_rows = 0, int decide_rows = 0);
// whether cached_attention takes the split-KV pair for such a call (fused: fused_cos_sin given; have_ws: split_ws given) — the ONE
// place the decision is taken (VSTAR_DECODE_SPLIT_KV=0 turns the path off), for the dispatcher and for the op-level door
bool cached_attention_splits(bool fused, bool have_ws, int R, int split_max_rows, int H, int max_keys);
// which kernels the last cached_attention call of THIS thread launched: 0 = un-fused, 1 = fused, 2 = fused split-KV pair, -1 = nothing
// (observability for the op-level tests, like gemm_last_tile())
int cached_attention_last_path();
// KV ancestry table of beam search (anc: [slots, ctx] int32, entry (slot, p) = the slot whose cache holds position p of the
// sequence in `slot`; cached_attention reads K/V through it when KvRows::anc is given).  mark: entry (row_slot[r], row_pos[r]) =
// row_slot[r] for every row; fill: slot's entries [lo, hi) = value; reorder: entries [lo, hi) of dst[i] = those of src[i], every
// source read before any destination is written (tmp: n * (hi - lo) ints); copy_rows: K/V rows [lo, hi) of every layer of
// `dst` = the rows src's entries point at (a physical copy) — kv0 is layer 0's view, layer i lies i * layer_stride cells behind it.
hipError_t kv_anc_mark(const int32_t* row_slot, const int32_t* row_pos, int R, int32_t* anc, int ctx, hipStream_t s);
hipError_t kv_anc_fill(int32_t* anc, int slot, int value, int lo, int hi, int ctx, hipStream_t s);
hipError_t kv_anc_reorder(int32_t* anc, int32_t* tmp, const int32_t* d_dst, const int32_t* d_src, int n, int lo, int hi, int ctx,
                          hipStream_t s);
hipError_t kv_copy_rows(const KvLayer& kv0, int layers, int64_t layer_stride, const int32_t* anc, int dst, int src, int lo, int hi,
                        hipStream_t s);
#ifdef VSTAR_LP_F16
// x [rows, 128] fp16 -> e4m3 codes [rows, 128], E8M0 bytes [rows, 4] and (nullable, may alias x) xhat = fp16(decoded): the device
// function every KV_FMT_MXFP8 writer quantises with
hipError_t kv_quantize_rows(const lp_t* x, int rows, uint8_t* codes, uint8_t* scales, lp_t* xhat, hipStream_t s);
#endif
// workspace of the split-KV decode path (scores, partial statistics / outputs, tickets) for up to max_rows new rows per step;
// must be zero-filled once
size_t cached_attention_split_ws_bytes(int max_rows, int H, int ctx);
// q [n*L, H*DH], kv [n*NK, 2*H*DH] (k | v) -> out [n*L, H*DH]
hipError_t perceiver_attention(const lp_t* q, const lp_t* kv, lp_t* out, int n, int L, int NK, int H, int DH, hipStream_t s);
// argmax over 16-bit logits rows: the first column holding the largest NUMBER. Unlike argmax_rows (below) it does not rank NaN: a NaN
// never wins, and a row of only NaN and / or values <= -3e38 (-inf) returns 0 — always an index in [0, cols)
hipError_t argmax_rows_lp(const lp_t* x, int rows, int cols, int64_t ld, int32_t* out, hipStream_t s);

// ---- W8A8 (quant.hip): per-row symmetric fp8 e4m3 quantisation, scale = absmax / 448 ----
hipError_t quantize_rows_fp8(const lp_t* x, int64_t ldx, uint8_t* q, int64_t ldq, float* scale, int rows, int cols,
                             hipStream_t s);
// LlamaRMSNorm whose 16-bit output row is quantised on the way out (cols <= 4096)
hipError_t rmsnorm_quant_fp8(const lp_t* x, const lp_t* gamma, uint8_t* q, float* scale, int rows, int cols, float eps,
                             hipStream_t s);
// LayerNorm (layernorm_lp with act = 0 and no row index) whose 16-bit output row is quantised on the way out (cols <= 4096): the same
// bytes and scales as layernorm_lp followed by quantize_rows_fp8 with ld = cols
hipError_t layernorm_quant_fp8(const lp_t* x, const lp_t* gamma, const lp_t* beta, uint8_t* q, float* scale, int rows, int cols,
                               float eps, hipStream_t s);

// block-scaled twin (mx.hpp): x [rows, cols] 16-bit -> fp8 bytes q [rows, ldq] + E8M0 scales (tile-major, rows % 128 == 0, cols % 128 == 0)
hipError_t quantize_rows_mx(const lp_t* x, int64_t ldx, uint8_t* q, int64_t ldq, uint8_t* scales, int rows, int cols, hipStream_t s);

// ---- norms (norm.hip) ----
// y[r] = LN(x[row_index ? row_index[r] : r]) ; act: 0 none, 1 exact GELU after the affine (LayerNorm2d+GELU)
hipError_t layernorm_lp(const lp_t* x, const lp_t* gamma, const lp_t* beta, lp_t* y, int rows, int cols,
                          float eps, const int32_t* row_index, int act, hipStream_t s);
// r[row] = rsqrt(mean(x[row]^2) + eps) (LlamaRMSNorm's fp32 statistics) — from x itself, or from the 64-column partial sums a GEMM
// epilogue wrote (GemmParams::sumsq_out); the two agree bit for bit (same summation tree).  cols % 64 == 0.
hipError_t rms_rstd_rows(const lp_t* x, int rows, int cols, float eps, float* r, hipStream_t s);
hipError_t rms_rstd_partials(const float* partials, int ld, int rows, int cols, float eps, float* r, hipStream_t s);
// LayerNorm twins: r[row] = 1 / sqrt(E[x^2] - E[x]^2 + eps) from the rows themselves / from the epilogue's partials (sumsq spans
// at [0, cols/64), sum spans at [cols/64, 2 cols/64) of each partial row); same summation trees, bit-identical to each other
hipError_t ln_rstd_rows(const lp_t* x, int rows, int cols, float eps, float* r, hipStream_t s);
hipError_t ln_rstd_partials(const float* partials, int ld, int rows, int cols, float eps, float* r, hipStream_t s);
// Folds LayerNorm(g, b_ln) into the packed Linear (W [n_rows, K] K-contiguous, bias [n_rows] or null) that consumes it, in place:
// bias[n] = sum_k W[n,k] b_ln[k] + bias[n] (fp32, from the unscaled W), then W[n,:] = W[n,:] * g - mean_k(W[n,:] * g)
hipError_t ln_fold_weights(lp_t* W, lp_t* bias, const lp_t* g, const lp_t* b_ln, int n_rows, int K, hipStream_t s);
// W[n, k] = round(W[n, k] * w[k]) for n < rows: folds a norm weight into the columns of a packed Linear; fill_lp: v[i] = value
hipError_t scale_cols_lp(lp_t* W, const lp_t* w, int64_t rows, int K, hipStream_t s);
hipError_t fill_lp(lp_t* v, int64_t n, float value, hipStream_t s);
hipError_t rmsnorm_lp(const lp_t* x, const lp_t* gamma, lp_t* y, int rows, int cols, float eps,
                        const int32_t* row_index, hipStream_t s);

// ---- attention (attention.hip) ----
// qkv: [B*S, 3*H*D] (q | k | v).  attn_prepare: in-place rotate-half RoPE on q,k (no-op when cos_sin == null)
// Grouped sequences (grp_R0 > 0; causal D = 128 only): rows [0, grp_Lc) of every sequence are a shared prefix, rows [grp_R0, S) are
// independent 32-row suffix blocks that attend to the prefix and causally to themselves; RoPE positions of a suffix block restart
// at grp_Lc.  grp_R0 % 128 == 0, (S - grp_R0) % 32 == 0.
hipError_t attn_prepare(lp_t* qkv, const lp_t* cos_sin /*[S, D] = cos(D/2)|sin(D/2), or null*/, int B, int S, int H, int D,
                        hipStream_t s, int grp_R0 = 0, int grp_Lc = 0);
hipError_t attn_forward(const lp_t* qkv, lp_t* out, int B, int S, int H, int D, int causal, float scale, hipStream_t s,
                        int grp_R0 = 0, int grp_Lc = 0);
// causal D = 128 with the output written block-scaled (mx.hpp): fp8 bytes out8 [B*S, H*128] + E8M0 scales (m128 = B*S / 128; B*S % 128
// == 0) — bit-identical to attn_forward followed by quantize_rows_mx
hipError_t attn_forward_mx(const lp_t* qkv, uint8_t* out8, uint8_t* scales, int B, int S, int H, float scale, hipStream_t s,
                           int grp_R0 = 0, int grp_Lc = 0);
// generic small attention for the SAM head: q[B,Nq,H*D] k[B,Nk,H*D] v[B,Nk,H*D] -> out[B,Nq,H*D]; D <= 32, fp32 math
hipError_t small_attention(const lp_t* q, const lp_t* k, const lp_t* v, lp_t* out, int B, int Nq, int Nk, int H,
                           int D, hipStream_t s);

// ---- elementwise / layout (elementwise.hip) ----
// pix [B,3,I,I] -> A [B*P, Kpad], k = c*ps*ps + ky*ps + kx, zero padded to Kpad
hipError_t im2col_patch(const lp_t* pix, lp_t* A, int B, int I, int ps, int Kpad, hipStream_t s);
// tokens[b,0]=cls+pos[0]; tokens[b,1+p]=patch[b,p]+pos[1+p]   (bf16 add)
hipError_t vit_assemble_tokens(const lp_t* patch, const lp_t* cls, const lp_t* pos, lp_t* tokens, int B, int P,
                               int C, hipStream_t s);
// LLaMA input embeddings for the text positions of the spliced sequence (image rows are written by the projector GEMM)
hipError_t llm_embed_text(const int32_t* ids, int L, int img_col, int P, const lp_t* table, int vocab, lp_t* x, int B,
                          int C, hipStream_t s);
// out[r, :] = a[r, :] + b[(r % b_rows), :]   (bf16 add; b broadcast over groups of b_rows)
hipError_t add_bcast(const lp_t* a, const lp_t* b, lp_t* out, int64_t rows, int cols, int64_t b_rows, hipStream_t s);
// out[(n * rows_per + p), :] = a[((n / rep) * rows_per + p), :] + b[0, :]  for n < n_out : every block of rows_per rows repeated rep times
hipError_t add_bcast_repeat(const lp_t* a, const lp_t* b, lp_t* out, int n_out, int rep, int rows_per, int cols, hipStream_t s);
// dst[(r * rep_stride + i) * ld + 0..cols) = src[i * ld + 0..cols) for r < nrep, i < nrows (one block of rows copied to the head of
// every sequence); cols % 8 == 0
hipError_t bcast_rows(const lp_t* src, lp_t* dst, int nrep, int64_t rep_stride, int nrows, int cols, int64_t ld, hipStream_t s);
// OWL-ViT: y[b,p,:] = x[b,1+p,:] * x[b,0,:]  (x = post_layernorm output, [B,N,C]) -> [B,N-1,C]
hipError_t owl_cls_mul(const lp_t* x, lp_t* y, int B, int N, int C, hipStream_t s);
// gather rows: y[r,:] = x[idx[r],:]
hipError_t gather_rows(const lp_t* x, const int32_t* idx, lp_t* y, int rows, int cols, hipStream_t s);
// argmax over fp32 logits rows (cols >= 1): the FIRST column holding the maximum, where NaN ranks above every number — torch.argmax's
// rule, so a row with NaN returns the column of its first NaN and every row returns an index in [0, cols)
hipError_t argmax_rows(const float* x, int rows, int cols, int ld, int32_t* out, int out_stride, hipStream_t s);

// ---- heads (heads.hip) ----
// class head: emb [R, ldc] fp32 = dense0(512) | shift | scale ; query [B, Q] bf16; rows_per_crop = 2304
// img_div: record b reads the image rows of crop b / img_div (several queries per crop: grouped scoring); 1 = one query per crop
hipError_t owl_class_logits(const float* emb, int ld, int Q, const lp_t* query, float* out, int out_stride_crop,
                            int B, int rows_per_crop, hipStream_t s, int img_div = 1);
// box head final: raw [R, 4] fp32 (dense2 out incl. bias) + grid bias -> sigmoid -> out[b*stride + p*4 ..]
hipError_t owl_box_finish(const float* raw, int ld, float* out, int out_stride_crop, int B, int grid, hipStream_t s, int img_div = 1);
// SAM upscaling: bilinear x2 (align_corners=False, fp32 -> bf16) fused with 3x3 im2col (zero pad):
// src [B, h, w, C] channels-last -> A [B*(2h)*(2w), 9*C], k = (ky*3+kx)*C + c
hipError_t upsample2x_im2col3x3(const lp_t* src, lp_t* A, int B, int h, int w, int C, hipStream_t s);
// masks[b, pix] = sum_c hyper[b,c] * up[b,pix,c]  (bf16 in, fp32 accumulate, bf16-rounded like the reference matmul) -> fp32
hipError_t hyper_mask(const lp_t* hyper, const lp_t* up, float* out, int out_stride_crop, int B, int npix, int C,
                      hipStream_t s);
// bilinear resize (align_corners=False) of fp32 [hin,win] -> [hout,wout], then clamp(min=0) unless clamp_min0 == 0
hipError_t resize_bilinear_clamp(const float* in, int hin, int win, float* out, int hout, int wout, hipStream_t s, int clamp_min0 = 1);

// min / max / total / rectangle sums of clamp(bilinear(lowres -> hout x wout), 0) for n maps in ONE launch (device arrays: lowres
// [n][hin*win], hw [n][2] = (hout, wout), rects [n][32], n_rects [n], out [n][3 + 8] doubles, mm_scratch [n][2])
hipError_t heat_stats_batch(const float* lowres, int hin, int win, const int* hw, const int* rects, const int* n_rects, int n,
                            int64_t max_pixels, double* out, unsigned* mm_scratch, hipStream_t s);

// ---- GPU-side crop preprocessing (preprocess.hip) ----
struct PreJob {            // one (crop, target) pair; jobs are stored as [crop][0 = CLIP, 1 = OWL-ViT]
  int x0, y0, cw, ch;      // crop box inside the resident image
  int in_w, in_h;          // resampled extent (CLIP: the padded square side; OWL: cw, ch)
  int out;                 // output side (I or 768)
  int hb_off, hc_off, hks; // horizontal bounds / coefficients offsets (int32 units) and kernel size
  int vb_off, vc_off, vks;
  int img_w;               // row pitch (pixels) of the image this crop is cut from
  int64_t temp_off;        // byte offset of this job's uint8 intermediate [in_h][out][3]
  int64_t out_off;         // element offset into the bf16 pixel buffer [3][out][out]
  const uint8_t* img;      // the resident image (slot) this crop is cut from
};
void pil_bicubic_coeffs(int in_size, int out_size, std::vector<int32_t>* bounds, std::vector<int32_t>* coeffs, int* ksize);
void clip_norm_lut(lp_t* lut);
hipError_t preprocess_launch(const PreJob* jobs, const int32_t* tables, uint8_t* temp,
                             const lp_t* lut, lp_t* out, int which, int B, int out_size, int max_in_h, hipStream_t s);

}  // namespace VS_NS
using namespace VS_NS;
