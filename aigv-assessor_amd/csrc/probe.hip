// The score-row attention probe of the C ABI (include/aigv_amd.h): aigv_score_attention_arm / _arm_tokens / _arm_values, what an armed
// aigv_llm_prefill / aigv_llm_extend launches per layer (probe_plan / probe_layer, called from passes.hip) and the context-free
// aigv_op_attention_probe / _probe_tokens / _probe_values.
// Host-side C++ only; the kernel is attnprobe.hip.
#include <cmath>

#include "ctx.h"

using namespace aigv;

// rows (packed indices of a pass whose sequences are cu[0..B]) -> the kernel's row table: sequence, its first row, its cached keys
static const char* fill_rows(ProbeArgs& a, const int32_t* rows, int n_rows, const int32_t* cu, int B, const int32_t* off_host) {
  if (n_rows < 1 || n_rows > AIGV_MAX_PROBE_ROWS) return "the number of probe rows is outside 1..AIGV_MAX_PROBE_ROWS (64)";
  a.n_rows = n_rows;
  for (int i = 0; i < n_rows; ++i) {
    if (rows[i] < 0 || rows[i] >= cu[B]) return "a probe row lies outside the pass";
    int b = 0;
    while (cu[b + 1] <= rows[i]) ++b;
    a.tab.r[i] = ProbeRow{rows[i], cu[b], b, off_host ? off_host[b] : 0};
  }
  return nullptr;
}

namespace aigv {

int probe_plan(aigv_ctx* c, const char* op, const int32_t* cu, int B, const int32_t* off_host, ProbeArgs* out) {
  const aigv_config& k = c->cfg;
  const int D = c->head_dim, g = c->g;
  const auto& pb = c->probe;
  if (pb.n_seg < 1 || pb.n_seg > AIGV_MAX_ATTN_SEGMENTS)
    return fail(c, AIGV_ERR_ARG, "%s: score attention armed with %d segments, outside 1..%d", op, pb.n_seg, AIGV_MAX_ATTN_SEGMENTS);
  if (pb.n_rows < 1 || pb.n_rows > AIGV_MAX_PROBE_ROWS)
    return fail(c, AIGV_ERR_ARG, "%s: score attention armed with %d rows, outside 1..%d", op, pb.n_rows, AIGV_MAX_PROBE_ROWS);
  if (!pb.seg_new || !pb.out) return fail(c, AIGV_ERR_ARG, "%s: score attention armed without a segment table or an output", op);
  if (off_host && !pb.seg_cached) return fail(c, AIGV_ERR_ARG, "%s: score attention over cached keys needs seg_cached (armed with NULL)", op);
  ProbeArgs a{};
  a.q = c->l_qkv; a.ldq = c->qkv_out;
  a.n_heads = k.llm_heads; a.n_kv_heads = k.llm_kv_heads;
  a.q_group_stride = (g + 2) * D;
  a.post_div = sqrtf((float)D);
  a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
  a.seg_new = pb.seg_new; a.seg_cached = off_host ? pb.seg_cached : nullptr; a.ld_cached = off_host ? pb.ld_cached : 0;
  a.n_seg = pb.n_seg;
  a.out = pb.out; a.out_row_stride = (size_t)k.llm_layers * k.llm_heads * pb.n_seg;
  a.tok = pb.tok; a.ld_tok = pb.ld_tok; a.tok_row_stride = (size_t)k.llm_layers * k.llm_heads * (size_t)std::max(pb.ld_tok, 0);
  a.val = pb.val; a.val_row_stride = (size_t)k.llm_layers * k.llm_heads * (size_t)(pb.n_seg + 1) * D;   // (v: per layer, probe_layer)
  if (const char* m = fill_rows(a, pb.rows, pb.n_rows, cu, B, off_host)) return fail(c, AIGV_ERR_ARG, "%s: score attention: %s (the pass has %d rows)", op, m, cu[B]);
  if (pb.tok || pb.ld_tok) {   // the dense rows: refused here, in front of the pass's first layer (aigv_probe_check repeats it per launch)
    if (!pb.tok || pb.ld_tok < 1 || pb.ld_tok > AIGV_MAX_KV_CAPACITY)
      return fail(c, AIGV_ERR_ARG, "%s: score attention tokens armed with ld_tok = %d, outside 1..%d, or without an output", op, pb.ld_tok, AIGV_MAX_KV_CAPACITY);
    for (int i = 0; i < a.n_rows; ++i) {
      const int keys = a.tab.r[i].off + (a.tab.r[i].row - a.tab.r[i].row0) + 1;
      if (keys > pb.ld_tok) return fail(c, AIGV_ERR_ARG, "%s: score attention tokens: ld_tok = %d is below the %d keys of probe row %d", op, pb.ld_tok, keys, i);
    }
  }
  *out = a;
  return 0;
}

int probe_layer(aigv_ctx* c, const ProbeArgs& plan, int li, bool cache, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const int D = c->head_dim, g = c->g, nkv = k.llm_kv_heads;
  ProbeArgs a = plan;
  if (cache) {
    const size_t kv_layer = (size_t)k.max_seqs * nkv * k.kv_capacity * D;
    a.k = c->kc + li * kv_layer; a.ldk = D; a.kv_head_stride = k.kv_capacity * D; a.kv_seq_stride = (size_t)nkv * k.kv_capacity * D;
    if (plan.val) { a.v = c->vc + li * kv_layer; a.ldv = D; }
  } else {
    a.k = c->l_qkv + (size_t)g * D; a.ldk = c->qkv_out; a.kv_head_stride = (g + 2) * D; a.kv_seq_stride = 0;
    if (plan.val) { a.v = c->l_qkv + (size_t)(g + 1) * D; a.ldv = c->qkv_out; }   // the V columns of the fused rows: at K + D within the kv head's group
  }
  a.out = plan.out + (size_t)li * k.llm_heads * plan.n_seg;
  if (plan.tok) a.tok = plan.tok + (size_t)li * k.llm_heads * plan.ld_tok;
  if (plan.val) a.val = plan.val + (size_t)li * k.llm_heads * (plan.n_seg + 1) * D;
  if (const char* m = aigv_probe_check(a, D, k.max_tokens, k.max_positions)) return fail(c, AIGV_ERR_ARG, "%s", m);
  HIPCHK(c, aigv_launch_attention_probe(a, D, s));
  return 0;
}

}  // namespace aigv

extern "C" {

static int arm(aigv_ctx* c, const char* op, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev, int ld_cached,
               int n_segments, float* out_dev, float* tok_out_dev, int ld_tok, float* val_out_dev = nullptr) {
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (!rows_host || !seg_new_dev || !out_dev) return fail(c, AIGV_ERR_ARG, "%s: null argument", op);
  if (ld_cached < 0) return fail(c, AIGV_ERR_ARG, "%s: ld_cached = %d must not be negative", op, ld_cached);
  // limits are refused by the PASS (with a message), as the rows are: the pass is what knows its row count.  Rows beyond the table's
  // capacity are not copied; the count alone makes the pass refuse.
  auto& pb = c->probe;
  pb.n_rows = n_rows; pb.n_seg = n_segments; pb.ld_cached = ld_cached;
  for (int i = 0; i < std::min(std::max(n_rows, 0), AIGV_MAX_PROBE_ROWS); ++i) pb.rows[i] = rows_host[i];
  pb.seg_new = seg_new_dev; pb.seg_cached = seg_cached_dev; pb.out = out_dev;
  pb.tok = tok_out_dev; pb.ld_tok = ld_tok;
  pb.val = val_out_dev;
  pb.armed = true;
  return 0;
}

int aigv_score_attention_arm(aigv_ctx* c, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev,
                             int ld_cached, int n_segments, float* out_dev) {
  return arm(c, "aigv_score_attention_arm", rows_host, n_rows, seg_new_dev, seg_cached_dev, ld_cached, n_segments, out_dev, nullptr, 0);
}

int aigv_score_attention_arm_tokens(aigv_ctx* c, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev,
                                    int ld_cached, int n_segments, float* out_dev, float* tok_out_dev, int ld_tok) {
  const char* op = "aigv_score_attention_arm_tokens";
  if (c && !tok_out_dev) return fail(c, AIGV_ERR_ARG, "%s: null tok_out_dev", op);
  if (c && ld_tok < 1) return fail(c, AIGV_ERR_ARG, "%s: ld_tok = %d must be positive", op, ld_tok);   // (too small for the rows, too large: the pass refuses)
  return arm(c, op, rows_host, n_rows, seg_new_dev, seg_cached_dev, ld_cached, n_segments, out_dev, tok_out_dev, ld_tok);
}

int aigv_score_attention_arm_values(aigv_ctx* c, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev,
                                    int ld_cached, int n_segments, float* out_dev, float* tok_out_dev, int ld_tok, float* val_out_dev) {
  const char* op = "aigv_score_attention_arm_values";
  if (c && !val_out_dev) return fail(c, AIGV_ERR_ARG, "%s: null val_out_dev", op);
  if (c && (tok_out_dev ? ld_tok < 1 : ld_tok != 0))   // the dense rows are optional here: both or neither
    return fail(c, AIGV_ERR_ARG, "%s: ld_tok = %d %s", op, ld_tok, tok_out_dev ? "must be positive" : "without tok_out_dev (pass NULL and 0)");
  return arm(c, op, rows_host, n_rows, seg_new_dev, seg_cached_dev, ld_cached, n_segments, out_dev, tok_out_dev, ld_tok, val_out_dev);
}

static int op_probe(const char* op, const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                    int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim, const void* cos,
                    const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new, const int32_t* seg_cached,
                    int ld_cached, int n_segments, float* out, float* tok_out, int ld_tok, void* stream, const void* v = nullptr, int ldv = 0,
                    float* val_out = nullptr) {
  if (!q || !k || !cu_host || !cos || !sin || !rows_host || !seg_new || !out) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (n_seq < 1 || n_seq > AIGV_SMALL_INTS / 2 - 1 || cu_host[0] != 0) return fail(nullptr, AIGV_ERR_ARG, "%s: needs 1 <= n_seq <= %d and cu[0] = 0", op, AIGV_SMALL_INTS / 2 - 1);
  for (int b = 0; b < n_seq; ++b)
    if (cu_host[b + 1] <= cu_host[b]) return fail(nullptr, AIGV_ERR_ARG, "%s: empty sequence %d", op, b);
  if (kv_seq_stride < 0 || ld_cached < 0 || max_pos < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: kv_seq_stride, ld_cached must not be negative, max_pos must be positive", op);
  if (kv_off_host && !kv_seq_stride) return fail(nullptr, AIGV_ERR_ARG, "%s: a key offset needs K in cache layout (kv_seq_stride)", op);
  if (n_heads < 1 || n_kv_heads < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: n_heads %d, n_kv_heads %d must be positive", op, n_heads, n_kv_heads);
  ProbeArgs a{};
  a.q = (const bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = ldk;
  a.n_heads = n_heads; a.n_kv_heads = n_kv_heads; a.q_group_stride = q_group_stride; a.kv_head_stride = kv_head_stride;
  a.kv_seq_stride = (size_t)kv_seq_stride;
  a.post_div = sqrtf((float)head_dim);
  a.rope_cos = (const bf16_t*)cos; a.rope_sin = (const bf16_t*)sin;
  a.seg_new = seg_new; a.seg_cached = seg_cached; a.ld_cached = ld_cached; a.n_seg = n_segments;
  a.out = out; a.out_row_stride = (size_t)n_heads * (n_segments > 0 ? n_segments : 0);
  a.tok = tok_out; a.ld_tok = ld_tok; a.tok_row_stride = (size_t)n_heads * (size_t)(ld_tok > 0 ? ld_tok : 0);
  a.v = (const bf16_t*)v; a.ldv = ldv; a.val = val_out; a.val_row_stride = (size_t)n_heads * (size_t)((n_segments > 0 ? n_segments : 0) + 1) * (size_t)(head_dim > 0 ? head_dim : 0);
  if (const char* m = fill_rows(a, rows_host, n_rows, cu_host, n_seq, kv_off_host)) return fail(nullptr, AIGV_ERR_ARG, "%s: %s", op, m);
  if (const char* m = aigv_probe_check(a, head_dim, cu_host[n_seq], max_pos)) return fail(nullptr, AIGV_ERR_ARG, "%s: %s", op, m);
  HIPCHK(nullptr, aigv_launch_attention_probe(a, head_dim, (hipStream_t)stream));
  return 0;
}

int aigv_op_attention_probe(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                            int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim, const void* cos,
                            const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new, const int32_t* seg_cached,
                            int ld_cached, int n_segments, float* out, void* stream) {
  return op_probe("aigv_op_attention_probe", q, ldq, k, ldk, cu_host, n_seq, n_heads, n_kv_heads, q_group_stride, kv_head_stride, kv_seq_stride, kv_off_host,
                  head_dim, cos, sin, max_pos, rows_host, n_rows, seg_new, seg_cached, ld_cached, n_segments, out, nullptr, 0, stream);
}

int aigv_op_attention_probe_tokens(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                                   int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim,
                                   const void* cos, const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new,
                                   const int32_t* seg_cached, int ld_cached, int n_segments, float* out, float* tok_out, int ld_tok, void* stream) {
  return op_probe("aigv_op_attention_probe_tokens", q, ldq, k, ldk, cu_host, n_seq, n_heads, n_kv_heads, q_group_stride, kv_head_stride, kv_seq_stride,
                  kv_off_host, head_dim, cos, sin, max_pos, rows_host, n_rows, seg_new, seg_cached, ld_cached, n_segments, out, tok_out, ld_tok, stream);
}

int aigv_op_attention_probe_values(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                                   int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim,
                                   const void* cos, const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new,
                                   const int32_t* seg_cached, int ld_cached, int n_segments, float* out, float* tok_out, int ld_tok, const void* v, int ldv,
                                   float* val_out, void* stream) {
  const char* op = "aigv_op_attention_probe_values";
  if (!v || !val_out) return fail(nullptr, AIGV_ERR_ARG, "%s: null %s", op, v ? "val_out" : "v");   // (this entry point IS the values form: neither half may be missing)
  return op_probe(op, q, ldq, k, ldk, cu_host, n_seq, n_heads, n_kv_heads, q_group_stride, kv_head_stride, kv_seq_stride, kv_off_host, head_dim, cos, sin,
                  max_pos, rows_host, n_rows, seg_new, seg_cached, ld_cached, n_segments, out, tok_out, ld_tok, stream, v, ldv, val_out);
}

}  // extern "C"
