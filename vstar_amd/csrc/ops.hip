// ops.hip — the operator-level entry points ("doors") of the bf16 half of libvstar_hip.so: vstar_op_* (include/vstar_hip.h).  A door
// runs ONE launcher (or a short fixed sequence) on buffers the caller owns, so that a single kernel can be tested against a reference;
// none of them takes an engine handle.  Built once, as bf16; the fp16 doors are vqa_ops.hip, and what both share is op_doors.hpp.
#ifdef VSTAR_LP_F16
#error "ops.hip is the bf16 instantiation: build without -DVSTAR_LP_F16"
#endif
#include <algorithm>
#include "op_doors.hpp"
#include "mx.hpp"                 // (after common.hpp, which names VS_NS)
#include "gemm_epilogue.hpp"      // gemm_map_row: the doors check extents with the kernels' own row map

// The kernel requests of `epilogue`, for every GEMM door: VSTAR_EPI_TILE4W / TILE256 / TILE128 (the first of them that is set) ->
// GemmParams::tile_force, the VSTAR_EPI_VARIANT field -> stages_force.  false (message set, nothing to launch): a variant outside
// {0, 2, 5, 6, 7}, or a variant of the 128-row family next to a request for a 256 x 256 kernel.
static bool op_gemm_flags(int epilogue, GemmParams* p) {
  p->tile_force = (epilogue & VSTAR_EPI_TILE4W) ? GEMM_TILE_4W : (epilogue & VSTAR_EPI_TILE256) ? 256 : (epilogue & VSTAR_EPI_TILE128) ? 128 : 0;
  const int v = (epilogue & VSTAR_EPI_VARIANT_MASK) >> 12;
  p->stages_force = v;
  if (v == 0) return true;
  if (v != 2 && v != 5 && v != 6 && v != 7) {
    tls_error() = "VSTAR_EPI_VARIANT(" + std::to_string(v) + "): the variants of the 128-row family are 2, 5, 6 and 7";
    return false;
  }
  if (epilogue & (VSTAR_EPI_TILE256 | VSTAR_EPI_TILE4W)) {
    tls_error() = "VSTAR_EPI_VARIANT with VSTAR_EPI_TILE256 / VSTAR_EPI_TILE4W: the variants belong to the 128-row family";
    return false;
  }
  return true;
}

static int gemm_debug_env() { const char* e = getenv("VSTAR_GEMM_DEBUG"); return e ? atoi(e) : 0; }

// What vstar_op_gemm and vstar_op_gemm_norm share: the operands and extents (the door has set its own fields of *p), the debug flags
// and the refusals, in the doors' order — both tile overrides, the door's own rule (`own`, null = none), the kernel requests, the
// forced 256 x 256 kernel outside its domain (each door words that one its own way: `tile256`).  false: message set, refuse.
static bool op_gemm_params(GemmParams* p, const uint16_t* A, int64_t lda, const uint16_t* W, const uint16_t* bias, const uint16_t* residual,
                           int64_t ldr, void* C, int64_t ldc, int M, int N, int K, int epilogue, const char* own, const char* tile256) {
  p->A = A; p->lda = lda; p->W = W; p->bias = bias; p->res = residual; p->ldr = ldr; p->C = C; p->ldc = ldc;
  p->M = M; p->N = N; p->K = K;
  p->debug_flags = gemm_debug_env();
  if ((epilogue & VSTAR_EPI_TILE128) && (epilogue & VSTAR_EPI_TILE256)) { tls_error() = "both tile overrides set"; return false; }
  if (own) { tls_error() = own; return false; }
  if (!op_gemm_flags(epilogue, p)) return false;
  if (p->tile_force == 256 && !gemm256_eligible(*p)) { tls_error() = tile256; return false; }
  return true;
}

// The W8A8 bench doors: one launch, then `iters` timed launches between two events (*gemm_ms = ms / iters); all of it skipped after a
// failure.  The caller synchronises.
static hipError_t op_gemm_timed(hipError_t e, const GemmParams& p, int epilogue, hipStream_t s, int iters, float* gemm_ms) {
  if (e == hipSuccess) e = gemm_lp(p, epilogue, false, s);
  if (e == hipSuccess && iters > 0 && gemm_ms) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0, s);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = gemm_lp(p, epilogue, false, s);
    hipEventRecord(e1, s);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *gemm_ms = ms / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  return e;
}

// the RoPE position the three fused-RoPE sites (gemm256.hip, gemm256_direct_epilogue.hpp) and rope_kernel derive for row r
static int64_t op_rope_pos(int64_t r, int S, int R0, int Lc, int pos0, int tail) {
  int64_t pos = r % S;
  if (R0 > 0 && pos >= R0) pos = Lc + ((pos - R0) & 31);
  if (tail > 0) pos = r >= tail ? r - tail : pos + pos0;
  return pos;
}
// the domain of grouped sequences (attn_forward / attn_forward_mx), as messages; empty = fine
static std::string op_group_domain(int S, int R0, int Lc) {
  if (R0 < 0 || Lc < 0) return "grp_R0 / grp_Lc negative";
  if (R0 == 0) return Lc ? "grp_Lc without grp_R0" : "";
  if (R0 % 128) return "grp_R0 % 128 != 0 (a suffix region starts on a 128-row query block)";
  if (Lc <= 0 || Lc > R0) return "0 < grp_Lc <= grp_R0 does not hold";
  if (R0 > S) return "grp_R0 > S";
  if ((S - R0) % 32) return "(S - grp_R0) % 32 != 0 (suffix blocks are 32 rows)";
  return "";
}

extern "C" {

// ---- GEMM, norms and attention on the caller's stream; a failure reads "HIP: ..." ----
int vstar_op_gemm(void* stream, const uint16_t* A, int64_t lda, const uint16_t* W, const uint16_t* bias,
                  const uint16_t* residual, int64_t ldr, void* C, int64_t ldc, int out_f32, int M, int N, int K,
                  int epilogue) {
  GemmParams p{};
  if (!op_gemm_params(&p, A, lda, W, bias, residual, ldr, C, ldc, M, N, K, epilogue, nullptr,
                      "VSTAR_EPI_TILE256: shape outside the 256x256 kernel's domain (M >= 1024, N >= 256, K % 128 == 0)"))
    return VSTAR_ERR_INVALID;
  hipError_t e = gemm_lp(p, epilogue & 0xff, out_f32 != 0, (hipStream_t)stream);
  return (epilogue & VSTAR_EPI_NOSYNC) ? op_result(e, "HIP") : op_sync_stream(e, stream);
}
int vstar_op_gemm_norm(void* stream, const uint16_t* A, int64_t lda, const uint16_t* W, const uint16_t* bias,
                       const uint16_t* residual, int64_t ldr, void* C, int64_t ldc, int M, int N, int K, int epilogue,
                       const float* row_scale, float* sumsq_out, int sumsq_ld) {
  GemmParams p{};
  p.row_scale = row_scale; p.sumsq_out = sumsq_out; p.sumsq_ld = sumsq_ld;
  const bool bad_sums = sumsq_out && ((epilogue & 0xff) != VSTAR_EPI_NONE || N % 64);
  if (!op_gemm_params(&p, A, lda, W, bias, residual, ldr, C, ldc, M, N, K, epilogue, bad_sums ? "sumsq_out: VSTAR_EPI_NONE and N % 64 == 0 only" : nullptr,
                      "VSTAR_EPI_TILE256: shape outside the 256x256 kernel's domain"))
    return VSTAR_ERR_INVALID;
  return op_sync_stream(gemm_lp(p, epilogue & 0xff, false, (hipStream_t)stream), stream);
}
int vstar_op_rms_rstd(void* stream, const uint16_t* x, const float* partials, int ld, int rows, int cols, float eps, float* r) {
  return op_sync_stream(x ? rms_rstd_rows(x, rows, cols, eps, r, (hipStream_t)stream)
                          : rms_rstd_partials(partials, ld, rows, cols, eps, r, (hipStream_t)stream), stream);
}
int vstar_op_ln_fold(void* stream, uint16_t* W, uint16_t* bias, const uint16_t* g, const uint16_t* b_ln, int n_rows, int K) {
  return op_sync_stream(ln_fold_weights(W, bias, g, b_ln, n_rows, K, (hipStream_t)stream), stream);
}
int vstar_op_gemm_last_tile(void) { return gemm_last_tile(); }
int vstar_op_gemm_last_mode(void) { return gemm_launched_mode(); }
int vstar_op_gemm_plan(int M, int N, int K, int epilogue, int has_residual, int fused_rope, int cus) {
  if (M <= 0 || N <= 0 || K <= 0 || cus <= 0) { tls_error() = "vstar_op_gemm_plan: bad argument"; return VSTAR_ERR_INVALID; }
  // gemm_plan dereferences nothing: a residual / a RoPE table only has to be there (non-null, aligned)
  static const lp_t* const some = (const lp_t*)(uintptr_t)0x10000;
  GemmParams p{};
  p.lda = K; p.M = M; p.N = N; p.K = K;
  const int n_out = (epilogue & 0xff) == VSTAR_EPI_SILU_MUL ? N / 2 : N;
  p.ldc = n_out;
  if (has_residual) { p.res = some; p.ldr = n_out; }
  if (fused_rope) { p.rope_cs = some; p.rope_S = 640; p.rope_cols = N * 2 / 3; }
  if (!op_gemm_flags(epilogue, &p)) return VSTAR_ERR_INVALID;
  if (p.stages_force && fused_rope) { tls_error() = "vstar_op_gemm_plan: VSTAR_EPI_VARIANT with fused RoPE (256 x 256 kernels only)"; return VSTAR_ERR_INVALID; }
  const GemmPlan pl = gemm_plan(p, epilogue & 0xff, false, cus);
  if (pl.status != hipSuccess) { tls_error() = std::string("vstar_op_gemm_plan: ") + hipGetErrorString(pl.status); return VSTAR_ERR_INVALID; }
  return pl.tile * 10 + pl.mode;
}
int vstar_op_layernorm(void* stream, const uint16_t* x, const uint16_t* g, const uint16_t* b, uint16_t* y, int rows,
                       int cols, float eps) {
  return op_sync_stream(layernorm_lp(x, g, b, y, rows, cols, eps, nullptr, 0, (hipStream_t)stream), stream);
}
int vstar_op_rmsnorm(void* stream, const uint16_t* x, const uint16_t* g, uint16_t* y, int rows, int cols, float eps) {
  return op_sync_stream(rmsnorm_lp(x, g, y, rows, cols, eps, nullptr, (hipStream_t)stream), stream);
}

// ---- W8A8 at op level: the operands are quantised into scratch here, then op_gemm_timed ----
int vstar_op_gemm_fp8(void* stream, const uint16_t* A, const uint16_t* W, const uint16_t* bias, const uint16_t* res, uint16_t* C,
                      int M, int N, int K, int epilogue, int iters, float* gemm_ms) {
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) { tls_error() = "bad argument"; return VSTAR_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  const int Npad = (N + 255) / 256 * 256;
  const int n_out = (epilogue & 0xff) == VSTAR_EPI_SILU_MUL ? N / 2 : N;
  hipError_t e = hipSuccess;
  OpBuf<uint8_t> Aq(e, (size_t)M * K), Wq(e, (size_t)Npad * K);
  OpBuf<float> sa(e, M), sw(e, Npad);
  if (e == hipSuccess) e = quantize_rows_fp8(A, K, Aq, K, sa, M, K, s);
  if (e == hipSuccess) e = quantize_rows_fp8(W, K, Wq, K, sw, Npad, K, s);
  GemmParams p{};
  p.A = (const lp_t*)Aq.p; p.lda = K; p.W = (const lp_t*)Wq.p; p.bias = bias; p.res = res; p.ldr = n_out; p.C = C; p.ldc = n_out;
  p.M = M; p.N = N; p.K = K; p.a_scale = sa; p.w_scale = sw;
  // VSTAR_EPI_TILE256 / VSTAR_EPI_TILE4W OR-ed into `epilogue`: force the 8-wave / the 4-wave W8A8 kernel (round 6; bit-identity tests)
  p.tile_force = (epilogue & VSTAR_EPI_TILE4W) ? GEMM_TILE_4W : (epilogue & VSTAR_EPI_TILE256) ? 256 : 0;
  if (e == hipSuccess && !gemm256_eligible(p)) e = hipErrorInvalidValue;      // shape not accepted by the W8A8 kernel
  return op_sync_stream(op_gemm_timed(e, p, epilogue & 0xff, s, iters, gemm_ms), stream);
}
// ---- block-scaled W8A8 (mx.hpp), op level ----
size_t vstar_op_mx_scale_bytes(int rows, int cols) { return (rows % 128 || cols % 128) ? 0 : mx_scale_bytes(rows, cols); }
int64_t vstar_op_mx_scale_offset(int row, int k_block, int rows) { return mx_scale_offset(row, k_block, rows >> 7); }
int vstar_op_quantize_mx(void* stream, const uint16_t* X, uint8_t* q, uint8_t* scales, int rows, int cols) {
  return op_sync_stream(quantize_rows_mx(X, cols, q, cols, scales, rows, cols, (hipStream_t)stream), stream);
}
int vstar_op_gemm_mx(void* stream, const uint8_t* Aq, const uint8_t* a_scales, const float* row_scale, const uint16_t* W, const uint16_t* res,
                     uint16_t* C, uint8_t* C8, uint8_t* c_scales, float* sumsq, int M, int N, int K, int epilogue, int iters, float* gemm_ms) {
  if (!Aq || !a_scales || !W || (!C && !C8) || M <= 0 || N <= 0 || K <= 0) { tls_error() = "bad argument"; return VSTAR_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  const int Npad = (N + 255) / 256 * 256;
  const int n_out = epilogue == VSTAR_EPI_SILU_MUL ? N / 2 : N;
  hipError_t e = hipSuccess;
  OpBuf<uint8_t> Wq(e, (size_t)Npad * K);
  OpBuf<float> sw(e, Npad);
  if (e == hipSuccess) e = quantize_rows_fp8(W, K, Wq, K, sw, Npad, K, s);
  GemmParams p{};
  p.A = (const lp_t*)Aq; p.lda = K; p.W = (const lp_t*)Wq.p; p.res = res; p.ldr = n_out; p.M = M; p.N = N; p.K = K;
  p.w_scale = sw; p.a_mx = a_scales; p.a_scale = row_scale;
  if (epilogue == VSTAR_EPI_SILU_MUL && C8) { p.C = C8; p.ldc = n_out; p.c_mx = c_scales; }       // fp8 out only
  else { p.C = C; p.ldc = n_out; p.c8 = C8; p.ldc8 = n_out; p.c_mx = C8 ? c_scales : nullptr; p.sumsq_out = C8 ? sumsq : nullptr; p.sumsq_ld = n_out / 64; }
  if (e == hipSuccess && !gemm_mx_supported(p, epilogue)) e = hipErrorInvalidValue;      // shape not accepted by the block-scaled W8A8 kernel
  return op_sync_stream(op_gemm_timed(e, p, epilogue, s, iters, gemm_ms), stream);
}
int vstar_op_gemm_fp8_mxout(void* stream, const uint16_t* A, const uint16_t* W, uint8_t* C8, uint8_t* c_scales, int M, int N, int K, int iters,
                            float* gemm_ms) {
  if (!A || !W || !C8 || !c_scales || M <= 0 || N <= 0 || K <= 0) { tls_error() = "bad argument"; return VSTAR_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  const int Npad = (N + 255) / 256 * 256;
  hipError_t e = hipSuccess;
  OpBuf<uint8_t> Aq(e, (size_t)M * K), Wq(e, (size_t)Npad * K);
  OpBuf<float> sa(e, M), sw(e, Npad);
  if (e == hipSuccess) e = quantize_rows_fp8(A, K, Aq, K, sa, M, K, s);
  if (e == hipSuccess) e = quantize_rows_fp8(W, K, Wq, K, sw, Npad, K, s);
  GemmParams p{};
  p.A = (const lp_t*)Aq.p; p.lda = K; p.W = (const lp_t*)Wq.p; p.C = C8; p.ldc = N / 2;
  p.M = M; p.N = N; p.K = K; p.a_scale = sa; p.w_scale = sw; p.c_mx = c_scales;
  if (e == hipSuccess && !gemm_mx_supported(p, VSTAR_EPI_SILU_MUL)) e = hipErrorInvalidValue;      // shape not accepted by the block-scaled W8A8 kernel
  return op_sync_stream(op_gemm_timed(e, p, VSTAR_EPI_SILU_MUL, s, iters, gemm_ms), stream);
}
int vstar_op_attention_mx(void* stream, const uint16_t* qkv, uint8_t* out8, uint8_t* scales, int B, int S, int H) {
  return op_sync_stream(attn_forward_mx(qkv, out8, scales, B, S, H, 1.0f / sqrtf(128.0f), (hipStream_t)stream), stream);
}

// ---- doors of the prefill-side features (row maps, fused RoPE, LayerNorm sums, grouped attention): every extent is checked on the
// host, with the kernels' own gemm_map_row, before anything is launched ----
int vstar_op_gemm_ex(void* stream, const vstar_gemm_ex* g) {
  static const char* const door = "vstar_op_gemm_ex";
  if (!g || !g->dev_A || !g->dev_W || !g->dev_C) return op_refuse(door, "null argument");
  if (g->M <= 0 || g->N <= 0 || g->K <= 0 || g->K % 64) return op_refuse(door, "M, N, K > 0 and K % 64 == 0 required");
  const int flags = g->epilogue & ~0xff, epi = g->epilogue & 0xff;
  if (flags & ~(VSTAR_EPI_TILE128 | VSTAR_EPI_TILE256 | VSTAR_EPI_TILE4W | VSTAR_EPI_VARIANT_MASK)) return op_refuse(door, "unknown bits in `epilogue` (VSTAR_EPI_NOSYNC is not taken)");
  if (epi > VSTAR_EPI_SILU_MUL) return op_refuse(door, "unknown epilogue");
  const int tiles = flags & ~VSTAR_EPI_VARIANT_MASK;
  if ((tiles & (tiles - 1)) != 0) return op_refuse(door, "more than one tile override set");
  GemmParams p{};
  if (!op_gemm_flags(g->epilogue, &p)) return op_refuse(door, std::string(tls_error()));
  const int forced = p.tile_force;
  if (p.stages_force && g->dev_rope_cs) return op_refuse(door, "rope_cs with VSTAR_EPI_VARIANT: the 128-row kernels have no fused RoPE");
  const int n_out = epi == VSTAR_EPI_SILU_MUL ? g->N / 2 : g->N;
  if (epi == VSTAR_EPI_SILU_MUL && g->N % 32) return op_refuse(door, "VSTAR_EPI_SILU_MUL: N % 32 == 0 required");
  if (g->lda < g->K || g->ldc < n_out || (g->dev_residual && g->ldr < n_out)) return op_refuse(door, "a leading dimension is shorter than its row");
  if (g->w_rows < ((int64_t)g->N + 255) / 256 * 256) return op_refuse(door, "W needs ceil(N / 256) * 256 rows");
  p.A = g->dev_A; p.lda = g->lda; p.a_group = g->a_group; p.a_gstride = g->a_gstride; p.a_off = g->a_off;
  p.W = g->dev_W; p.bias = g->dev_bias; p.res = g->dev_residual; p.ldr = g->ldr;
  p.C = g->dev_C; p.ldc = g->ldc; p.c_group = g->c_group; p.c_gstride = g->c_gstride; p.c_off = g->c_off;
  p.M = g->M; p.N = g->N; p.K = g->K;
  p.row_scale = g->dev_row_scale; p.sumsq_out = g->dev_sumsq_out; p.sumsq_ld = g->sumsq_ld; p.stats_sum = g->stats_sum;
  p.rope_cs = g->dev_rope_cs; p.rope_S = g->rope_S; p.rope_cols = g->rope_cols; p.rope_R0 = g->rope_R0; p.rope_Lc = g->rope_Lc;
  p.rope_pos0 = g->rope_pos0; p.rope_tail = g->rope_tail;
  p.debug_flags = gemm_debug_env();
  // ---- row maps: every mapped row of the call (rows of a ragged tile are clamped to M - 1 by the kernels, so [0, M) is all of them) ----
  const bool a_map = p.a_group > 0, c_map = p.c_group > 0;
  if ((a_map || c_map) && forced == GEMM_TILE_4W) return op_refuse(door, "VSTAR_EPI_TILE4W with a row map (the 4-wave kernel addresses rows by tile)");
  if (a_map && (p.a_gstride < 0 || p.a_off < 0)) return op_refuse(door, "negative A row map");
  if (c_map && p.c_off < 0) return op_refuse(door, "negative C row map");
  if (c_map && p.M > p.c_group && p.c_gstride < p.c_group) return op_refuse(door, "C row map sends two rows to one (c_gstride < c_group)");
  int64_t a_max = 0, c_max = 0;
  for (int r = 0; r < p.M; ++r) {
    a_max = std::max(a_max, gemm_map_row(r, p.a_group, p.a_gstride, p.a_off));
    c_max = std::max(c_max, gemm_map_row(r, p.c_group, p.c_gstride, p.c_off));
  }
  if (a_max >= g->a_rows) return op_refuse(door, "mapped A row " + std::to_string(a_max) + " outside a_rows = " + std::to_string(g->a_rows) + " (A, row_scale)");
  if (c_max >= g->c_rows) return op_refuse(door, "mapped C row " + std::to_string(c_max) + " outside c_rows = " + std::to_string(g->c_rows) + " (C, residual, sumsq_out)");
  // ---- statistics ----
  if (p.stats_sum && !p.sumsq_out) return op_refuse(door, "stats_sum without sumsq_out");
  if (p.sumsq_out) {
    if (epi != VSTAR_EPI_NONE || p.N % 64) return op_refuse(door, "sumsq_out: VSTAR_EPI_NONE and N % 64 == 0 only");
    const int spans = p.N / 64;
    if (p.stats_sum < 0 || (p.stats_sum && p.stats_sum < spans)) return op_refuse(door, "stats_sum must be 0 or >= N / 64 (the sums would land on the sums of squares)");
    if (p.sumsq_ld < (p.stats_sum ? p.stats_sum + spans : spans)) return op_refuse(door, "sumsq_ld shorter than the partials of a row");
  }
  // ---- fused RoPE ----
  if (!p.rope_cs && (p.rope_S || p.rope_cols || p.rope_R0 || p.rope_Lc || p.rope_pos0 || p.rope_tail)) return op_refuse(door, "rope_* set without rope_cs");
  if (p.rope_cs) {
    if (forced == 128) return op_refuse(door, "rope_cs with VSTAR_EPI_TILE128: the 128-row kernels have no fused RoPE");
    if (epi != VSTAR_EPI_NONE) return op_refuse(door, "rope_cs with an epilogue other than VSTAR_EPI_NONE");
    if (p.sumsq_out) return op_refuse(door, "rope_cs with sumsq_out (the in-register epilogue's spans of a RoPE tile are not 64 consecutive columns)");
    if (((uintptr_t)p.rope_cs & 15)) return op_refuse(door, "rope_cs must be 16-byte aligned");
    if (p.rope_S <= 0 || p.rope_cols <= 0 || p.rope_cols % 256 || p.rope_cols > p.N) return op_refuse(door, "rope_S > 0 and 0 < rope_cols <= N, rope_cols % 256 == 0 required");
    if (p.rope_R0 < 0 || p.rope_Lc < 0 || p.rope_pos0 < 0 || p.rope_tail < 0) return op_refuse(door, "negative rope_* argument");
    if (p.rope_R0 > 0 && p.rope_tail > 0) return op_refuse(door, "rope_R0 together with rope_tail (grouped and shared-prefix positions exclude each other)");
    if (p.rope_R0 == 0 && p.rope_Lc) return op_refuse(door, "rope_Lc without rope_R0");
    if (p.rope_tail == 0 && p.rope_pos0) return op_refuse(door, "rope_pos0 without rope_tail");
    if (p.rope_R0 > 0 && (p.rope_Lc <= 0 || p.rope_Lc > p.rope_R0)) return op_refuse(door, "0 < rope_Lc <= rope_R0 does not hold");
    if (!gemm256_eligible(p)) return op_refuse(door, "rope_cs: shape outside the 256 x 256 kernels' domain (M >= 1024, N >= 256, K % 128 == 0), the only ones with fused RoPE");
    int64_t pos_max = 0;
    for (int r = 0; r < p.M; ++r) pos_max = std::max(pos_max, op_rope_pos(r, p.rope_S, p.rope_R0, p.rope_Lc, p.rope_pos0, p.rope_tail));
    if (pos_max >= g->rope_rows) return op_refuse(door, "RoPE position " + std::to_string(pos_max) + " outside rope_rows = " + std::to_string(g->rope_rows));
  }
  if (forced == 256 && !gemm256_eligible(p)) return op_refuse(door, "VSTAR_EPI_TILE256: shape outside the 256 x 256 kernel's domain (M >= 1024, N >= 256, K % 128 == 0)");
  if (forced == GEMM_TILE_4W && !(gemm256_eligible(p) && gemm_mx_supported(p, epi))) return op_refuse(door, "VSTAR_EPI_TILE4W: call outside the 4-wave kernel's domain");
  hipError_t e = gemm_lp(p, epi, false, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return op_refuse(door, "the dispatcher refused the call (alignment of A / W, lda % 8)");
  return op_sync_stream(e, stream);
}
int vstar_op_rope(void* stream, uint16_t* qkv, int64_t qkv_rows, const uint16_t* cos_sin, int table_rows, int B, int S, int H, int D,
                  int grp_R0, int grp_Lc) {
  static const char* const door = "vstar_op_rope";
  if (!qkv || !cos_sin || B <= 0 || S <= 0 || H <= 0) return op_refuse(door, "bad argument");
  if (D != 64 && D != 128) return op_refuse(door, "D must be 64 or 128");
  if (grp_R0 < 0 || grp_Lc < 0 || (grp_R0 == 0 && grp_Lc) || (grp_R0 > 0 && (grp_Lc <= 0 || grp_Lc > grp_R0))) return op_refuse(door, "0 < grp_Lc <= grp_R0 does not hold");
  if (qkv_rows < (int64_t)B * S) return op_refuse(door, "qkv_rows < B * S");
  int64_t pos_max = 0;
  for (int r = 0; r < S; ++r) pos_max = std::max(pos_max, op_rope_pos(r, S, grp_R0, grp_Lc, 0, 0));
  if (pos_max >= table_rows) return op_refuse(door, "RoPE position " + std::to_string(pos_max) + " outside table_rows = " + std::to_string(table_rows));
  return op_sync_stream(attn_prepare(qkv, cos_sin, B, S, H, D, (hipStream_t)stream, grp_R0, grp_Lc), stream);
}
int vstar_op_attention_grouped(void* stream, const uint16_t* qkv, int64_t qkv_rows, uint16_t* out, int64_t out_rows, int B, int S, int H,
                               int grp_R0, int grp_Lc) {
  static const char* const door = "vstar_op_attention_grouped";
  if (!qkv || !out || B <= 0 || S <= 0 || H <= 0) return op_refuse(door, "bad argument");
  const std::string why = op_group_domain(S, grp_R0, grp_Lc);
  if (!why.empty()) return op_refuse(door, why);
  if (qkv_rows < (int64_t)B * S || out_rows < (int64_t)B * S) return op_refuse(door, "qkv_rows / out_rows < B * S");
  return op_sync_stream(attn_forward(qkv, out, B, S, H, 128, 1, 1.0f / sqrtf(128.0f), (hipStream_t)stream, grp_R0, grp_Lc), stream);
}
int vstar_op_attention_mx_grouped(void* stream, const uint16_t* qkv, int64_t qkv_rows, uint8_t* out8, int64_t out_rows, uint8_t* scales, int B,
                                  int S, int H, int grp_R0, int grp_Lc) {
  static const char* const door = "vstar_op_attention_mx_grouped";
  if (!qkv || !out8 || !scales || B <= 0 || S <= 0 || H <= 0) return op_refuse(door, "bad argument");
  if ((int64_t)B * S % 128) return op_refuse(door, "B * S % 128 != 0 (the scale layout is per 128-row block)");
  const std::string why = op_group_domain(S, grp_R0, grp_Lc);
  if (!why.empty()) return op_refuse(door, why);
  if (qkv_rows < (int64_t)B * S || out_rows < (int64_t)B * S) return op_refuse(door, "qkv_rows / out_rows < B * S");
  return op_sync_stream(attn_forward_mx(qkv, out8, scales, B, S, H, 1.0f / sqrtf(128.0f), (hipStream_t)stream, grp_R0, grp_Lc), stream);
}

size_t vstar_op_attention_workspace(int B, int S, int H, int D) {
  (void)B; (void)H;
  return (size_t)S * D * 2 + 256;     // the RoPE cos|sin table only: V is transposed inside the kernel (no V^T buffer)
}
int vstar_op_attention(void* stream, uint16_t* qkv, uint16_t* out, void* ws, size_t ws_bytes, int B, int S, int H, int D,
                       int causal, float rope_theta) {
  if (ws_bytes < vstar_op_attention_workspace(B, S, H, D)) { tls_error() = "attention workspace too small"; return VSTAR_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  lp_t* cs = nullptr;
  if (rope_theta > 0.f) {
    cs = (lp_t*)ws;
    std::vector<lp_t> tab((size_t)S * D);
    for (int p = 0; p < S; ++p)
      for (int i = 0; i < D / 2; ++i) {
        const float inv = 1.0f / powf(rope_theta, (float)(2 * i) / (float)D);
        tab[(size_t)p * D + i] = f2lp(cosf((float)p * inv));
        tab[(size_t)p * D + D / 2 + i] = f2lp(sinf((float)p * inv));
      }
    hipError_t e = hipMemcpy(cs, tab.data(), tab.size() * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) return op_result(e, "HIP");
  }
  hipError_t e = attn_prepare(qkv, cs, B, S, H, D, s);
  if (e == hipSuccess) e = attn_forward(qkv, out, B, S, H, D, causal, 1.0f / sqrtf((float)D), s);
  return op_sync_stream(e, stream);
}

// ---- doors of the small kernels (heads / layout / norm / fp8 rows / SAM attention): ONE launcher each, then synchronise ----
int vstar_op_owl_class_logits(void* stream, const float* emb, int ld, int Q, const uint16_t* query, float* out, int out_stride_crop,
                              int B, int rows_per_crop, int img_div) {
  return op_sync_stream(owl_class_logits(emb, ld, Q, query, out, out_stride_crop, B, rows_per_crop, (hipStream_t)stream, img_div), stream);
}
int vstar_op_owl_box_finish(void* stream, const float* raw, int ld, float* out, int out_stride_crop, int B, int grid, int img_div) {
  return op_sync_stream(owl_box_finish(raw, ld, out, out_stride_crop, B, grid, (hipStream_t)stream, img_div), stream);
}
int vstar_op_upsample2x_im2col3x3(void* stream, const uint16_t* src, uint16_t* A, int B, int h, int w, int C) {
  return op_sync_stream(upsample2x_im2col3x3(src, A, B, h, w, C, (hipStream_t)stream), stream);
}
int vstar_op_hyper_mask(void* stream, const uint16_t* hyper, const uint16_t* up, float* out, int out_stride_crop, int B, int npix,
                        int C) {
  return op_sync_stream(hyper_mask(hyper, up, out, out_stride_crop, B, npix, C, (hipStream_t)stream), stream);
}
int vstar_op_im2col_patch(void* stream, const uint16_t* pix, uint16_t* A, int B, int I, int ps, int Kpad) {
  return op_sync_stream(im2col_patch(pix, A, B, I, ps, Kpad, (hipStream_t)stream), stream);
}
int vstar_op_vit_assemble_tokens(void* stream, const uint16_t* patch, const uint16_t* cls, const uint16_t* pos, uint16_t* tokens,
                                 int B, int P, int C) {
  return op_sync_stream(vit_assemble_tokens(patch, cls, pos, tokens, B, P, C, (hipStream_t)stream), stream);
}
int vstar_op_llm_embed_text(void* stream, const int32_t* ids, int L, int img_col, int P, const uint16_t* table, int vocab,
                            uint16_t* x, int B, int C) {
  return op_sync_stream(llm_embed_text(ids, L, img_col, P, table, vocab, x, B, C, (hipStream_t)stream), stream);
}
int vstar_op_add_bcast(void* stream, const uint16_t* a, const uint16_t* b, uint16_t* out, int64_t rows, int cols, int64_t b_rows) {
  return op_sync_stream(add_bcast(a, b, out, rows, cols, b_rows, (hipStream_t)stream), stream);
}
int vstar_op_add_bcast_repeat(void* stream, const uint16_t* a, const uint16_t* b, uint16_t* out, int n_out, int rep, int rows_per,
                              int cols) {
  return op_sync_stream(add_bcast_repeat(a, b, out, n_out, rep, rows_per, cols, (hipStream_t)stream), stream);
}
int vstar_op_bcast_rows(void* stream, const uint16_t* src, uint16_t* dst, int nrep, int64_t rep_stride, int nrows, int cols,
                        int64_t ld) {
  return op_sync_stream(bcast_rows(src, dst, nrep, rep_stride, nrows, cols, ld, (hipStream_t)stream), stream);
}
int vstar_op_owl_cls_mul(void* stream, const uint16_t* x, uint16_t* y, int B, int N, int C) {
  return op_sync_stream(owl_cls_mul(x, y, B, N, C, (hipStream_t)stream), stream);
}
int vstar_op_gather_rows(void* stream, const uint16_t* x, const int32_t* idx, uint16_t* y, int rows, int cols) {
  return op_sync_stream(gather_rows(x, idx, y, rows, cols, (hipStream_t)stream), stream);
}
int vstar_op_argmax_rows(void* stream, const float* x, int rows, int cols, int ld, int32_t* out, int out_stride) {
  return op_sync_stream(argmax_rows(x, rows, cols, ld, out, out_stride, (hipStream_t)stream), stream);
}
int vstar_op_layernorm_ex(void* stream, const uint16_t* x, const uint16_t* g, const uint16_t* b, uint16_t* y, int rows, int cols,
                          float eps, const int32_t* row_index, int act) {
  return op_sync_stream(layernorm_lp(x, g, b, y, rows, cols, eps, row_index, act, (hipStream_t)stream), stream);
}
int vstar_op_rmsnorm_ex(void* stream, const uint16_t* x, const uint16_t* g, uint16_t* y, int rows, int cols, float eps,
                        const int32_t* row_index) {
  return op_sync_stream(rmsnorm_lp(x, g, y, rows, cols, eps, row_index, (hipStream_t)stream), stream);
}
int vstar_op_ln_rstd(void* stream, const uint16_t* x, const float* partials, int ld, int rows, int cols, float eps, float* r) {
  if (!x && !partials) { tls_error() = "vstar_op_ln_rstd: x and partials are both NULL"; return VSTAR_ERR_INVALID; }
  return op_sync_stream(x ? ln_rstd_rows(x, rows, cols, eps, r, (hipStream_t)stream)
                          : ln_rstd_partials(partials, ld, rows, cols, eps, r, (hipStream_t)stream), stream);
}
int vstar_op_scale_cols(void* stream, uint16_t* W, const uint16_t* w, int64_t rows, int K) {
  return op_sync_stream(scale_cols_lp(W, w, rows, K, (hipStream_t)stream), stream);
}
int vstar_op_fill(void* stream, uint16_t* v, int64_t n, float value) {
  return op_sync_stream(fill_lp(v, n, value, (hipStream_t)stream), stream);
}
int vstar_op_quantize_rows_fp8(void* stream, const uint16_t* x, int64_t ldx, uint8_t* q, int64_t ldq, float* scale, int rows,
                               int cols) {
  return op_sync_stream(quantize_rows_fp8(x, ldx, q, ldq, scale, rows, cols, (hipStream_t)stream), stream);
}
int vstar_op_layernorm_quant_fp8(void* stream, const uint16_t* x, const uint16_t* gamma, const uint16_t* beta, uint8_t* q, float* scale,
                                 int rows, int cols, float eps) {
  return op_sync_stream(layernorm_quant_fp8(x, gamma, beta, q, scale, rows, cols, eps, (hipStream_t)stream), stream);
}
int vstar_op_rmsnorm_quant_fp8(void* stream, const uint16_t* x, const uint16_t* gamma, uint8_t* q, float* scale, int rows, int cols,
                               float eps) {
  return op_sync_stream(rmsnorm_quant_fp8(x, gamma, q, scale, rows, cols, eps, (hipStream_t)stream), stream);
}
int vstar_op_small_attention(void* stream, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, int B, int Nq,
                             int Nk, int H, int D) {
  return op_sync_stream(small_attention(q, k, v, out, B, Nq, Nk, H, D, (hipStream_t)stream), stream);
}

// ---- op-level doors of the bf16 DECODE kernels (decode.hip / skinny.hip as this library's VSM engine runs them;
// tests/test_bf16_decode_gpu.py): the checks and bodies are op_doors.hpp's, the ones the fp16 doors of vqa_ops.hip instantiate ----
int vstar_op_rope_kv_append(void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                            const vstar_vqa_kv_rows* rows) {
  return door_rope_kv_append("vstar_op_rope_kv_append", dev_qkv, dev_cos_sin, table_rows, kv, rows);
}
int vstar_op_cached_attention(void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                              const vstar_vqa_kv_rows* rows, int max_keys, int path, int repeat, void* dev_out, int* path_ran) {
  return door_cached_attention("vstar_op_cached_attention", dev_qkv, dev_cos_sin, table_rows, kv, rows, max_keys, path, repeat, dev_out, path_ran);
}
int vstar_op_embed_rows(const int32_t* host_src, int R, const void* dev_table, int vocab, const void* dev_feats, int64_t n_feat_rows,
                        void* dev_x, int C) {
  return door_embed_rows("vstar_op_embed_rows", host_src, R, dev_table, vocab, dev_feats, n_feat_rows, dev_x, C);
}
int vstar_op_argmax_rows_lp(const void* dev_x, int rows, int cols, int64_t ld, int32_t* host_out) {
  return door_argmax_rows("vstar_op_argmax_rows_lp", dev_x, rows, cols, ld, host_out);
}
int vstar_op_gemm_skinny(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K, int epilogue,
                         int kernel, int out_f32, const void* norm_w, float norm_eps, int layout, int* kernel_ran) {
  const char* door = "vstar_op_gemm_skinny";
  const bool silu = epilogue == VSTAR_EPI_SILU_MUL;
  const int nt = silu ? 2 : 1;
  if (!A || !W || !C || !kernel_ran) return op_refuse(door, "A, W, C and kernel_ran are required");
  if (M < 1 || M > 64) return op_refuse(door, "M must lie in [1, 64]: the weight-streaming kernels' domain");
  if (N < 1 || K < 64 || K % 64) return op_refuse(door, "N >= 1, K >= 64 and K % 64 == 0");
  if (epilogue < VSTAR_EPI_NONE || epilogue > VSTAR_EPI_SILU_MUL) return op_refuse(door, "epilogue must be one of the five VSTAR_EPI_* values");
  if (silu && N % 2) return op_refuse(door, "VSTAR_EPI_SILU_MUL needs an even N (gate | up)");
  if (kernel != 1 && kernel != 3) return op_refuse(door, "kernel must be 1 (dispatch) or 3 (register kernel)");
  if ((out_f32 != 0 && out_f32 != 1) || (layout != 0 && layout != 1)) return op_refuse(door, "out_f32 and layout must be 0 or 1");
  if (layout == 1 && N % (16 * nt)) return op_refuse(door, "the tile-major layout needs whole 16-row (SiLU-mul: 32-row) tiles");
  *kernel_ran = 0;
  GemmParams p = op_dense_gemm(A, W, bias, res, C, M, N, K, epilogue, norm_w, norm_eps);
  if (kernel == 3) p.tile_force = -1;      // the register-streaming kernel even where the LDS-ring variant would run
  hipError_t e = hipSuccess;
  OpBuf<lp_t> tiles(e, (size_t)N * K, layout == 1);
  if (layout == 1 && e == hipSuccess) e = skinny_pack_tiles((const lp_t*)W, tiles.p, N, K, nt, nullptr);
  p.dw = SkinnyWeights{SKINNY_W_F16, nullptr, nullptr, tiles.p};
  if (e == hipSuccess) e = gemm_skinny_lp(p, epilogue, out_f32 != 0, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) *kernel_ran = gemm_skinny_last_kernel();
  return op_result(e, door);
}

}  // extern "C"
