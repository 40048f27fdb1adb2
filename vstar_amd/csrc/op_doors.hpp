// op_doors.hpp — what the op-level doors share: the helpers every door reports through (op_refuse, op_result, the two
// synchronise-then-report forms), device scratch (OpBuf), the dense GemmParams fill of the skinny / fp16 GEMM doors, and the
// dtype-generic checks and bodies of the decode-side doors (decode.hip).  Lives in VS_NS like the kernels it drives, so ops.hip (bf16:
// vstar_op_*) and vqa_ops.hip (fp16, -DVSTAR_LP_F16: vstar_vqa_op_*) instantiate the SAME text; `fn` is the door's exported name, the
// prefix of every message.  The structs vstar_vqa_kv_view / vstar_vqa_kv_rows are declared in include/vstar_hip.h.
#pragma once
#include <string>
#include <vector>
#include "kernels.hpp"
#include "engine_base.hpp"

namespace VS_NS {

// Device scratch of an op-level wrapper: n elements allocated on construction (none when !wanted), freed on scope exit.  `e` is the
// wrapper's one error: every step is skipped once it holds a failure, so the first failure is what it reports.
template <class T>
struct OpBuf {
  hipError_t& e;
  T* p = nullptr;
  size_t bytes;
  OpBuf(hipError_t& err, size_t n, bool wanted = true) : e(err), bytes(n * sizeof(T)) {
    if (wanted && e == hipSuccess) e = hipMalloc(&p, bytes);
  }
  OpBuf(const OpBuf&) = delete;
  ~OpBuf() { if (p) hipFree(p); }
  void upload(const T* host) { if (p && e == hipSuccess) e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice); }
  void download(T* host) { if (p && host && e == hipSuccess) e = hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost); }
  operator T*() const { return p; }
};

// a refused call: VSTAR_ERR_INVALID, message "<fn>: <why>"
inline int op_refuse(const char* fn, const std::string& why) {
  tls_error() = std::string(fn) + ": " + why;
  return VSTAR_ERR_INVALID;
}

// the return code of a door whose device work ended in `e`; a failure's message is "<prefix>: <HIP's text>", prefix being the door's
// name or, at the doors that predate the names, the fixed "HIP"
inline int op_result(hipError_t e, const char* prefix) {
  if (e == hipSuccess) return VSTAR_OK;
  tls_error() = std::string(prefix) + ": " + hipGetErrorString(e);
  return VSTAR_ERR_HIP;
}
// synchronise, then report: the caller's stream (the doors that take one) / the device (the doors that launch on the null stream)
inline int op_sync_stream(hipError_t e, void* stream, const char* prefix = "HIP") {
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  return op_result(e, prefix);
}
inline int op_sync_device(hipError_t e, const char* fn) {
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return op_result(e, fn);
}

// the dense A[M,K] · W[N,K]^T -> C[M,n_out] call of the skinny / fp16 GEMM doors: n_out = N / 2 under VSTAR_EPI_SILU_MUL, else N
inline GemmParams op_dense_gemm(const void* A, const void* W, const void* bias, const void* res, void* C, int M, int N, int K, int epilogue,
                                const void* norm_w, float norm_eps) {
  GemmParams p{};
  const int n_out = epilogue == VSTAR_EPI_SILU_MUL ? N / 2 : N;
  p.A = (const lp_t*)A; p.lda = K; p.W = (const lp_t*)W; p.bias = (const lp_t*)bias; p.res = (const lp_t*)res; p.ldr = n_out;
  p.C = C; p.ldc = n_out; p.M = M; p.N = N; p.K = K;
  p.norm_w = (const lp_t*)norm_w; p.norm_eps = norm_eps;
  return p;
}

// ---- op-level doors of the decode-side kernels: every index array is a HOST array, checked here against the extents before
// anything is allocated or launched ----
// the rules of vstar_vqa_kv_view / vstar_vqa_kv_rows (include/vstar_hip.h); path < 0: the append door (no attention rules).
// Returns the violated rule, or null.
inline const char* kv_op_check(const vstar_vqa_kv_view* kv, const vstar_vqa_kv_rows* rw, int table_rows, int max_keys, int path) {
  if (!kv || !rw) return "null view or rows";
  if (kv->fmt < 0 || kv->fmt > 2) return "fmt must be 0, 1 or 2";
  if (kv->heads < 1 || kv->heads > 256 || kv->ctx < 1 || kv->ctx > (1 << 20) || kv->slots < 1 || kv->slots > 4096)
    return "heads in [1, 256], ctx in [1, 2^20], slots in [1, 4096]";
  if (!kv->dev_k || !kv->dev_v) return "dev_k and dev_v are required";
  if (kv->fmt == 1 && (!kv->dev_ks || !kv->dev_vs)) return "format 1 needs dev_ks and dev_vs";
  {
    KvLayer l;
    l.fmt = kv->fmt; l.ks = (uint8_t*)kv->dev_ks; l.vs = (uint8_t*)kv->dev_vs;
    if (!kv_format_ok(l)) return "fmt must be 0: the bf16 build has format 0 only (kv_format_ok)";
  }
  if (rw->R < 1 || rw->R > 65535 || rw->n_seq < 1 || rw->n_seq > 65535) return "R and n_seq in [1, 65535]";
  if (!rw->row_seq || !rw->row_pos || !rw->row_slot || !rw->seq_kv || !rw->seq_prefix || !rw->seq_past) return "null index array";
  if (table_rows < 1) return "table_rows must be >= 1";
  const int pos_end = kv->ctx < table_rows ? kv->ctx : table_rows;
  for (int i = 0; i < rw->n_seq; ++i) {
    if (rw->seq_kv[i] < 0 || rw->seq_kv[i] >= kv->slots || rw->seq_prefix[i] < 0 || rw->seq_prefix[i] >= kv->slots)
      return "seq_kv and seq_prefix must lie in [0, slots)";
    if (rw->seq_past[i] < 0) return "seq_past must be >= 0";
  }
  for (int r = 0; r < rw->R; ++r) {
    if (rw->row_pos[r] < -1 || rw->row_pos[r] >= pos_end) return "row_pos must lie in [-1, min(ctx, table_rows))";
    if (rw->row_slot[r] < 0 || rw->row_slot[r] >= kv->slots) return "row_slot must lie in [0, slots)";
    if (rw->row_seq[r] < 0 || rw->row_seq[r] >= rw->n_seq) return "row_seq must lie in [0, n_seq)";
    if (rw->row_pos[r] >= 0 && rw->seq_past[rw->row_seq[r]] > rw->row_pos[r]) return "seq_past must be <= row_pos of the sequence's rows";
  }
  if (rw->anc)
    for (int64_t i = 0; i < (int64_t)kv->slots * kv->ctx; ++i)
      if (rw->anc[i] < 0 || rw->anc[i] >= kv->slots) return "anc entries must lie in [0, slots)";
  if (path < 0) return nullptr;
  if (path > 2) return "path must be 0, 1 or 2";
  if (max_keys < 1 || max_keys > kv->ctx) return "max_keys must lie in [1, ctx]";
  for (int r = 0; r < rw->R; ++r)
    if (rw->row_pos[r] + 1 > max_keys) return "row_pos + 1 must be <= max_keys";
  if (path >= 1) {
    if (rw->R != rw->n_seq) return "fused paths: exactly one row per sequence";
    std::vector<char> seen_seq((size_t)rw->n_seq, 0), seen_slot((size_t)kv->slots, 0);
    for (int r = 0; r < rw->R; ++r) {
      if (rw->row_pos[r] < 0) return "fused paths: no padding rows";
      if (seen_seq[(size_t)rw->row_seq[r]]++) return "fused paths: exactly one row per sequence";
      if (rw->row_slot[r] != rw->seq_kv[rw->row_seq[r]]) return "fused paths: row_slot must be the sequence's seq_kv";
    }
    for (int i = 0; i < rw->n_seq; ++i)
      if (seen_slot[(size_t)rw->seq_kv[i]]++) return "fused paths: seq_kv must be pairwise distinct";
  }
  if (path <= 1 && (size_t)(128 + max_keys) * sizeof(float) > 40 * 1024) return "(128 + max_keys) * 4 must be <= 40 KiB on paths 0 and 1";
  if (path == 2 && !cached_attention_splits(true, true, rw->R, rw->R, kv->heads, max_keys))
    return "path 2 outside the split-KV domain (R * heads <= 128, max_keys >= 256, VSTAR_DECODE_SPLIT_KV not 0)";
  return nullptr;
}

// the host index arrays of a checked call on the device, and the kernels' views of them
struct KvOpArgs {
  OpBuf<int32_t> row_seq, row_pos, row_slot, seq_kv, seq_prefix, seq_past, anc;
  KvLayer layer;
  KvRows rows;
  KvOpArgs(hipError_t& e, const vstar_vqa_kv_view& kv, const vstar_vqa_kv_rows& rw)
      : row_seq(e, rw.R), row_pos(e, rw.R), row_slot(e, rw.R), seq_kv(e, rw.n_seq), seq_prefix(e, rw.n_seq), seq_past(e, rw.n_seq),
        anc(e, (size_t)kv.slots * kv.ctx, rw.anc != nullptr) {
    row_seq.upload(rw.row_seq); row_pos.upload(rw.row_pos); row_slot.upload(rw.row_slot);
    seq_kv.upload(rw.seq_kv); seq_prefix.upload(rw.seq_prefix); seq_past.upload(rw.seq_past);
    if (rw.anc) anc.upload(rw.anc);
    layer.fmt = kv.fmt; layer.k = kv.dev_k; layer.v = kv.dev_v;
    layer.ks = kv.fmt == 1 ? (uint8_t*)kv.dev_ks : nullptr; layer.vs = kv.fmt == 1 ? (uint8_t*)kv.dev_vs : nullptr;
    layer.slot_stride = (int64_t)kv.heads * kv.ctx * 128; layer.H = kv.heads; layer.ctx = kv.ctx;
    rows.row_seq = row_seq; rows.row_pos = row_pos; rows.row_slot = row_slot;
    rows.seq_kv = seq_kv; rows.seq_prefix = seq_prefix; rows.seq_past = seq_past; rows.anc = anc;
  }
};

inline int door_rope_kv_append(const char* fn, void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                               const vstar_vqa_kv_rows* rows) {
  const char* bad = !dev_qkv || !dev_cos_sin ? "qkv and cos_sin are required" : kv_op_check(kv, rows, table_rows, 0, -1);
  if (bad) return op_refuse(fn, bad);
  hipError_t e = hipSuccess;
  KvOpArgs a(e, *kv, *rows);
  if (e == hipSuccess) e = rope_kv_append((lp_t*)dev_qkv, (const lp_t*)dev_cos_sin, a.layer, a.rows, rows->R, nullptr);
  return op_sync_device(e, fn);
}

inline int door_cached_attention(const char* fn, void* dev_qkv, const void* dev_cos_sin, int table_rows, const vstar_vqa_kv_view* kv,
                                 const vstar_vqa_kv_rows* rows, int max_keys, int path, int repeat, void* dev_out, int* path_ran) {
  const char* bad = !dev_qkv || !dev_out || !path_ran ? "qkv, out and path_ran are required"
                    : path < 0                        ? "path must be 0, 1 or 2"
                    : path >= 1 && !dev_cos_sin       ? "the fused paths need cos_sin"
                    : repeat < 1 || repeat > 16       ? "repeat must lie in [1, 16]"
                                                      : kv_op_check(kv, rows, table_rows, max_keys, path);
  if (bad) return op_refuse(fn, bad);
  *path_ran = -1;
  hipError_t e = hipSuccess;
  KvOpArgs a(e, *kv, *rows);
  OpBuf<char> ws(e, cached_attention_split_ws_bytes(rows->R, kv->heads, kv->ctx), path == 2);
  if (ws.p && e == hipSuccess) e = hipMemset(ws.p, 0, ws.bytes);
  for (int i = 0; i < repeat && e == hipSuccess; ++i) {
    e = cached_attention((const lp_t*)dev_qkv, a.layer, a.rows, path >= 1 ? (const lp_t*)dev_cos_sin : nullptr, (lp_t*)dev_out, rows->R,
                         max_keys, nullptr, ws.p, path == 2 ? rows->R : 0);
    if (e == hipSuccess && cached_attention_last_path() != path) {      // the door checked the dispatcher's own predicate
      hipDeviceSynchronize();
      *path_ran = cached_attention_last_path();
      tls_error() = std::string(fn) + ": the dispatcher took another path than the one asked for";
      return VSTAR_ERR_STATE;
    }
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) *path_ran = cached_attention_last_path();
  return op_result(e, fn);
}

inline int door_embed_rows(const char* fn, const int32_t* host_src, int R, const void* dev_table, int vocab, const void* dev_feats,
                           int64_t n_feat_rows, void* dev_x, int C) {
  if (!host_src || !dev_table || !dev_x || R < 1 || R > (1 << 20) || vocab < 1 || C < 8 || C % 8 || n_feat_rows < 0 ||
      (n_feat_rows > 0 && !dev_feats)) {
    tls_error() = std::string(fn) + ": bad argument (src, table and x not null, 1 <= R <= 2^20, vocab >= 1, C % 8 == 0, feats with n_feat_rows > 0)";
    return VSTAR_ERR_INVALID;
  }
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_src(e, R);
  d_src.upload(host_src);
  if (e == hipSuccess) e = embed_rows(d_src, (const lp_t*)dev_table, vocab, (const lp_t*)dev_feats, n_feat_rows, (lp_t*)dev_x, R, C, nullptr);
  return op_sync_device(e, fn);
}

inline int door_argmax_rows(const char* fn, const void* dev_x, int rows, int cols, int64_t ld, int32_t* host_out) {
  if (!dev_x || !host_out || rows < 1 || rows > (1 << 20) || cols < 1 || ld < cols) {
    tls_error() = std::string(fn) + ": bad argument (x and out not null, 1 <= rows <= 2^20, 1 <= cols <= ld)";
    return VSTAR_ERR_INVALID;
  }
  hipError_t e = hipSuccess;
  OpBuf<int32_t> d_out(e, rows);
  if (e == hipSuccess) e = argmax_rows_lp((const lp_t*)dev_x, rows, cols, ld, d_out, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  d_out.download(host_out);
  return op_result(e, fn);
}

}  // namespace VS_NS
