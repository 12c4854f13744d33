// The score-row attention probe of the C ABI (include/aigv_amd.h): aigv_score_attention_arm / _arm_tokens / _arm_values, what an armed
// aigv_llm_prefill / aigv_llm_extend launches per layer (probe_plan / probe_layer, called from passes.hip) and the context-free
// aigv_op_attention_probe / _probe_tokens / _probe_values - and its all-rows sibling, the attention flow map: aigv_attention_map_arm, what an armed
// aigv_llm_prefill launches per layer (map_plan / map_layer) and the context-free aigv_op_attention_map.
// Host-side C++ only; the kernels are attnprobe.hip and attnmap.hip.
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

// ---- the attention flow map (attnmap.hip): every row of every head, per layer ---------------------------------------------------------
static const char* fill_cu(AttnMapArgs& a, const int32_t* cu, int B) {
  if (B < 1 || B > AIGV_MAP_MAX_SEQS) return "the number of sequences is outside 1..127";
  a.n_seq = B;
  for (int b = 0; b <= B; ++b) a.cu[b] = cu[b];
  return nullptr;
}

int map_plan(aigv_ctx* c, const int32_t* cu, int B, int keep_kv, AttnMapArgs* out) {
  const char* op = "aigv_llm_prefill";
  const aigv_config& k = c->cfg;
  const int D = c->head_dim, g = c->g;
  const auto& mp = c->amap;
  if (c->drop.armed) return fail(c, AIGV_ERR_ARG, "%s: a key-drop mask and the attention map are both armed: the map does not know the mask", op);
  if (keep_kv) return fail(c, AIGV_ERR_ARG, "%s: keep_kv with the attention map armed: the map has no cache form, and a pass that keeps its KV is followed by continuations it cannot cover", op);
  if (mp.n_seg < 1 || mp.n_seg > AIGV_MAX_ATTN_SEGMENTS) return fail(c, AIGV_ERR_ARG, "%s: attention map armed with %d segments, outside 1..%d", op, mp.n_seg, AIGV_MAX_ATTN_SEGMENTS);
  if (!mp.seg) return fail(c, AIGV_ERR_ARG, "%s: attention map armed without a segment table", op);
  if (!mp.seg_out && !mp.rows_out) return fail(c, AIGV_ERR_ARG, "%s: attention map armed without an output (seg_out and rows_out both NULL)", op);
  if (mp.lo < 0 || mp.lo > mp.hi || mp.hi > k.llm_layers) return fail(c, AIGV_ERR_ARG, "%s: attention map rows armed for layers [%d, %d), outside 0 <= lo <= hi <= %d", op, mp.lo, mp.hi, k.llm_layers);
  if (!mp.rows_out && mp.lo != mp.hi) return fail(c, AIGV_ERR_ARG, "%s: attention map armed with the layer window [%d, %d) and rows_out NULL", op, mp.lo, mp.hi);
  if (mp.seg_out && !mp.scratch && mp.hi - mp.lo < k.llm_layers) return fail(c, AIGV_ERR_ARG, "%s: attention map armed with seg_out and without the per-layer scratch the layers outside [%d, %d) need", op, mp.lo, mp.hi);
  AttnMapArgs a{};
  a.q = c->l_qkv; a.ldq = c->qkv_out;
  a.k = c->l_qkv + (size_t)g * D; a.ldk = c->qkv_out;
  a.n_heads = k.llm_heads; a.n_kv_heads = k.llm_kv_heads;
  a.q_group_stride = a.kv_head_stride = (g + 2) * D;
  a.post_div = sqrtf((float)D);
  a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
  a.seg = mp.seg; a.n_seg = mp.n_seg;
  a.rows = mp.scratch ? mp.scratch : mp.rows_out;   // (per layer: map_layer; here only so that the check sees an output)
  a.seg_out = mp.seg_out; a.seg_out_seq_stride = (size_t)k.llm_layers * k.llm_heads * mp.n_seg * mp.n_seg;
  if (const char* m = fill_cu(a, cu, B)) return fail(c, AIGV_ERR_ARG, "%s: attention map: %s", op, m);
  if (const char* m = aigv_attn_map_check(a, D, k.max_positions)) return fail(c, AIGV_ERR_ARG, "%s: %s", op, m);
  *out = a;
  return 0;
}

int map_layer(aigv_ctx* c, const AttnMapArgs& plan, int li, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const auto& mp = c->amap;
  const bool in_window = mp.rows_out && li >= mp.lo && li < mp.hi;
  if (!in_window && !mp.seg_out) return 0;   // nobody reads this layer's rows
  AttnMapArgs a = plan;
  const size_t layer_rows = (size_t)a.cu[a.n_seq] * k.llm_heads * a.n_seg;
  a.rows = in_window ? mp.rows_out + (size_t)(li - mp.lo) * layer_rows : mp.scratch;
  if (mp.seg_out) a.seg_out = mp.seg_out + (size_t)li * k.llm_heads * a.n_seg * a.n_seg;
  // (checked by map_plan: only the two output addresses differ from layer to layer, and its refusals leave neither null where it is used)
  HIPCHK(c, aigv_launch_attention_map(a, c->head_dim, s));
  return 0;
}

}  // namespace aigv

extern "C" {

int aigv_attention_map_arm(aigv_ctx* c, const int32_t* seg_dev, int n_segments, float* scratch_dev, float* seg_out_dev, float* rows_out_dev, int layer_lo,
                           int layer_hi) {
  const char* op = "aigv_attention_map_arm";
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (!seg_dev) return fail(c, AIGV_ERR_ARG, "%s: null segment table", op);
  if (!seg_out_dev && !rows_out_dev) return fail(c, AIGV_ERR_ARG, "%s: seg_out_dev and rows_out_dev are both null: nothing to report", op);
  // limits (segments, the window, the scratch a fold needs) are refused by the PASS, with a message: it is what knows its layers and rows
  auto& mp = c->amap;
  mp.seg = seg_dev; mp.n_seg = n_segments; mp.scratch = scratch_dev; mp.seg_out = seg_out_dev; mp.rows_out = rows_out_dev;
  mp.lo = layer_lo; mp.hi = layer_hi;
  mp.armed = true;
  return 0;
}

int aigv_op_attention_map(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads, int q_group_stride,
                          int kv_head_stride, int head_dim, const void* cos, const void* sin, int max_pos, const int32_t* seg, int n_segments, float* rows_out,
                          float* seg_out, void* stream) {
  const char* op = "aigv_op_attention_map";
  if (!q || !k || !cu_host || !cos || !sin || !seg || !rows_out) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (max_pos < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: max_pos must be positive", op);
  AttnMapArgs a{};
  a.q = (const bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = ldk;
  a.n_heads = n_heads; a.n_kv_heads = n_kv_heads; a.q_group_stride = q_group_stride; a.kv_head_stride = kv_head_stride;
  a.post_div = sqrtf((float)head_dim);
  a.rope_cos = (const bf16_t*)cos; a.rope_sin = (const bf16_t*)sin;
  a.seg = seg; a.n_seg = n_segments;
  a.rows = rows_out;
  a.seg_out = seg_out; a.seg_out_seq_stride = (size_t)(n_heads > 0 ? n_heads : 0) * (size_t)(n_segments > 0 ? n_segments : 0) * (size_t)(n_segments > 0 ? n_segments : 0);
  if (const char* m = fill_cu(a, cu_host, n_seq)) return fail(nullptr, AIGV_ERR_ARG, "%s: %s", op, m);
  if (const char* m = aigv_attn_map_check(a, head_dim, max_pos)) return fail(nullptr, AIGV_ERR_ARG, "%s: %s", op, m);
  HIPCHK(nullptr, aigv_launch_attention_map(a, head_dim, (hipStream_t)stream));
  return 0;
}

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
