// What the host sources of the C ABI (include/aigv_amd.h) share - context.hip (life cycle, weight store, errors), dispatch.hip (which GEMM kernel
// runs which rows), passes.hip (the scoring passes, the decode step), ops.hip (aigv_op_*), tune.hip (knob table, mode setters, profiler read-out):
// the context, error plumbing, device allocation, the profiling brackets, the knobs in force for a call, the dispatcher's interface.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/aigv_amd.h"
#include "kernels.h"

namespace aigv {

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

struct VitLayer {
  const bf16_t *ls1, *ls2, *qkv_w, *qkv_b, *qn, *kn, *proj_w, *proj_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b, *n1w, *n1b, *n2w, *n2b;
};
struct LlmLayer {
  const bf16_t *wqkv, *wo, *w13, *w2, *an, *fn;
};

struct LlmLayerFp8 {   // e4m3 copies of a decoder layer's weights, one fp32 scale per output channel (aigv_set_precision)
  uint8_t *wqkv = nullptr, *wo = nullptr, *w13 = nullptr, *w2 = nullptr;
  float *s_wqkv = nullptr, *s_wo = nullptr, *s_w13 = nullptr, *s_w2 = nullptr;
};

struct ProfRec {
  int cls;
  hipEvent_t a, b;
  double flops, bytes;
};

// Row plan of one pass (round 4): how the rows of the activation matrices divide into INDEPENDENT sequences (InternViT frames,
// InternLM2 clips) and, from that alone, which kernel form every row runs in - so that a row's bits never depend on its batch mates:
//   body: rows [0, 256 * floor(L / 256)) of every sequence -> full-K 256x256 kernel, whole tiles addressed through the half-tile table;
//   tail: the remaining < 256 rows of every sequence      -> one or two (ragged) half tiles; run with a split-K factor that is a
//                                                            function of the GEMM's (N, K) only (1 = inside the body's launch);
//   tiny: tails of <= TINY_TAIL rows (InternViT: 1025 = 4 * 256 + 1) -> the weight-streaming skinny kernel in its fixed 4-slice form.
struct RowPlan {
  struct Tiny { int row0, stride_rows, count; };   // rows row0 + i * stride_rows, i < count
  std::vector<Tiny> tiny;
  int rows = 0, body_halves = 0, tail_halves = 0, tail_rows = 0;
  int32_t* d_tab = nullptr;     // device: (base row, valid rows) per half, body halves first
  int cap_halves = 0;
};

}  // namespace aigv

struct aigv_ctx {
  aigv_config cfg{};
  int device = 0;
  std::string err;
  std::unordered_map<std::string, aigv::DevBuf> w;
  std::vector<void*> allocs;      // weight-side device memory: derived weights, e4m3 copies
  std::vector<void*> ws_allocs;   // capacity-sized workspaces (aigv_ctx_create / aigv_ctx_resize)
  bool ws_phase = false;          // dalloc books into ws_allocs while the workspaces are being allocated
  bool finalized = false;
  // derived sizes
  int np = 0, S = 0, Kp = 0, grid = 0, ntok = 0, proj_in = 0, qkv_out = 0, head_dim = 0, vit_head_dim = 0, g = 0;
  // derived weights
  std::vector<aigv::VitLayer> vit;
  std::vector<aigv::LlmLayer> llm;
  const bf16_t *patch_w = nullptr, *patch_b = nullptr, *pos = nullptr, *cls_pos = nullptr;
  const bf16_t *tok_emb = nullptr, *final_norm = nullptr, *lm_head = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
  const bf16_t *p_ln_w[2] = {nullptr, nullptr}, *p_ln_b[2] = {nullptr, nullptr}, *p_w1[2] = {nullptr, nullptr},
               *p_b1[2] = {nullptr, nullptr}, *p_w2[2] = {nullptr, nullptr}, *p_b2[2] = {nullptr, nullptr};  // 0 mlp1, 1 motion_mlp
  ScoreHeadArgs score{};
  // workspaces
  bf16_t *v_col = nullptr, *v_x = nullptr, *v_t = nullptr, *v_qkv = nullptr, *v_ao = nullptr, *v_h = nullptr;
  int32_t* v_cu = nullptr;
  bf16_t *p_t = nullptr, *p_mid = nullptr;
  bf16_t *l_h = nullptr, *l_t = nullptr, *l_qkv = nullptr, *l_ao = nullptr, *l_ffn = nullptr, *l_rows = nullptr;
  int32_t *l_pos = nullptr, *l_seq = nullptr, *l_cu = nullptr, *l_rowidx = nullptr, *l_rowidx2 = nullptr, *l_kvlen = nullptr;
  unsigned long long* l_packed = nullptr;
  int32_t* l_neg1 = nullptr;   // max_tokens x int32 -1: the "plain text token" slot map of aigv_llm_extend
  // fp8 mode of the InternLM2 prefill GEMMs (aigv_set_precision): weights quantised once, activations per row on the fly
  bool fp8_llm = false;
  bool llm_lin_dirty = false;  // an InternLM2 linear (wqkv / wo / w1 / w3 / w2) was (re)loaded since the e4m3 copies were made
  std::vector<aigv::LlmLayerFp8> llm8;
  uint8_t* q8 = nullptr;       // [max_tokens, max(H, I)] e4m3 activations of the GEMM about to run
  float* q8_scale = nullptr;   // [max_tokens]
  aigv::RowPlan rp_vit, rp_llm;           // row plans of the InternViT frames of the current chunk and of the current prefill's clips
  const aigv::RowPlan* cur_rp = nullptr;  // plan the InternLM2 layer helpers run under (null: batch-level dispatch, aigv_llm_extend)
  bool trim_last_layer = true;
  int attn_round_scores = AIGV_ATTENTION_NUMERICS_DEFAULT;   // prefill attention: 1 = the reference's bf16 rounding points of the score matrix, 0 = fp32 scores (default since round 5: profiles/r5_parity_stats.txt)
  // the experiment knobs of this context, by AIGV_TUNE_* (aigv_ctx_tune / aigv_set_gemm_mode): -1 = follow the process default (aigv_tune_*)
  int tune[AIGV_TUNE_COUNT];
  aigv_ctx() { std::fill(tune, tune + AIGV_TUNE_COUNT, -1); }
  size_t splitk_floats = 0;
  // fp32 slabs of the split-K row bands, owned by the context.  Two of them: aigv_vit_forward launches on `splitk_ws_vit`, every other entry
  // point on `splitk_ws` - so ONE visual front (InternViT on a stream of its own: InternVLChatModel.prefetch) may run beside ONE
  // projector / InternLM2 pass of the same context.  Within each half the rule stays: one launch stream at a time.
  float* splitk_ws = nullptr;
  float* splitk_ws_vit = nullptr;
  bool on_vit_front = false;   // host-side: set while aigv_vit_forward enqueues (SplitkVitScope)
  bf16_t* l_trim = nullptr;   // last-layer row trimming: compact [64, H] x 2 (attention out, normed) + [64, I], reused per 64 consumed rows
  bf16_t* l_trim_h = nullptr; // ... and the consumed rows' hidden states [max_out_rows + max_seqs + 64, H]
  bf16_t* l_score_ws = nullptr;
  bf16_t* l_lp = nullptr;     // aigv_out_row_logprob: lm-head logits of 64 consumed rows [64, lp_ldo], reused per 64 rows; aigv_decode_step_topk_logprob: the step's logits
  int lp_ldo = 0;
  bf16_t *kc = nullptr, *vc = nullptr;   // [layer][seq][kv head][cap][D]
  bf16_t *kc_alt = nullptr, *vc_alt = nullptr;   // second cache of the same size, made by the first aigv_kv_reorder (beam search gathers into it, then the two swap)
  int32_t* beam_ints = nullptr;                  // [2 * max_seqs]: parent slots | live lengths of a reorder
  // Key-drop mask of the KV cache, [max_seqs][kv_drop_ld = ceil(kv_capacity / 64)] words in AttnArgs::key_drop's layout by absolute position: allocated, freed
  // and resized with the caches.  Written by aigv_llm_prefill(keep_kv) under an armed mask, which sets kv_masked (an unmasked keep_kv prefill clears it);
  // read by aigv_llm_extend and the decode steps while kv_masked; aigv_kv_fork replicates its rows, aigv_kv_reorder gathers them into kv_drop_alt and swaps.
  uint64_t *kv_drop = nullptr, *kv_drop_alt = nullptr;
  int kv_drop_ld = 0;
  bool kv_masked = false;
  float* dec_ws = nullptr;
  float2* dec_lse = nullptr;  // aigv_decode_step_logprob: per-16-column log-sum-exp partials [min(max_seqs, 64)][ceil(vocab / 16)]
  bf16_t* dec_cand = nullptr; // aigv_decode_step_cand_logprob: bf16 logits of the candidate columns [min(max_seqs, 64)][AIGV_MAX_CANDIDATES]
  int32_t *dec_pos = nullptr, *dec_seq = nullptr, *dec_kvlen = nullptr, *dec_slot = nullptr;   // device-side decode state
  std::vector<int32_t> h_dec;
  std::vector<int32_t> h_pos, h_seq, h_rowidx, h_kvlen;
  int kv_seqs = 0;
  bool kv_valid = false;
  // score-row attention probe (aigv_score_attention_arm): armed for exactly the next aigv_llm_prefill / aigv_llm_extend
  struct {
    bool armed = false;
    int n_rows = 0, n_seg = 0, ld_cached = 0;
    int32_t rows[AIGV_MAX_PROBE_ROWS];
    const int32_t *seg_new = nullptr, *seg_cached = nullptr;
    float* out = nullptr;
    float* tok = nullptr;   // aigv_score_attention_arm_tokens: the dense rows [n_rows][layers][n_heads][ld_tok], else nullptr / 0
    int ld_tok = 0;
    float* val = nullptr;   // aigv_score_attention_arm_values: the value vectors [n_rows][layers][n_heads][n_seg + 1][D], else nullptr
  } probe;
  // attention flow map (aigv_attention_map_arm): armed for exactly the next aigv_llm_prefill, which launches the all-rows map kernel (attnmap.hip) after
  // llm_layer_qkv of every layer - into slice li - lo of rows_out for the layers of the window, else into scratch - and folds it into seg_out
  struct {
    bool armed = false;
    const int32_t* seg = nullptr;      // device [T]
    int n_seg = 0;
    float* scratch = nullptr;          // device, the caller's: [T][n_heads][n_seg], rewritten by every layer outside the window
    float* seg_out = nullptr;          // device, the caller's: [n_clips][layers][n_heads][n_seg][n_seg], or nullptr
    float* rows_out = nullptr;         // device, the caller's: [hi - lo][T][n_heads][n_seg], or nullptr
    int lo = 0, hi = 0;
  } amap;
  // InternViT attention map (aigv_vit_attention_arm): armed for exactly the next aigv_vit_forward, which launches the map kernels (vitmap.hip) between the
  // QK-norm and the flash attention of every layer lo <= li < hi - into out[absolute frame][li - lo] - and nothing for a layer outside the window
  struct {
    bool armed = false;
    float* out = nullptr;              // device, the caller's: [n_frames][hi - lo][S][S], per_head: [n_frames][hi - lo][vit_heads][S][S]
    int lo = 0, hi = 0, per_head = 0;
  } vmap;
  // InternViT patch mask (aigv_vit_key_drop_arm): armed for exactly the next aigv_vit_forward, whose flash attention of every layer lo <= li < hi runs
  // the non-causal key-drop form under the words of its chunk's frames, words + f0 * ld; the other layers run the unmasked kernel
  struct {
    bool armed = false;
    const uint64_t* words = nullptr;   // device, the caller's: [n_frames][ld] words, AttnArgs::key_drop's layout (key 0 = cls, key 1 + grid * y + x = patch (y, x))
    int ld = 0;
    int lo = 0, hi = 0;
  } vdrop;
  float2* v_mapstats = nullptr;        // [vit_chunk][vit_heads][S] (m, total) of the map's rows: owned by the context, nothing is allocated in the pass
  // key-drop mask (aigv_key_drop_arm / _ex): armed for exactly the next aigv_llm_prefill, which applies it in the attention of the layers
  // [layer_begin, layer_end) - every layer for aigv_key_drop_arm - to the query rows `rows` selects (null: every row); keep_kv, which takes
  // neither qualifier: and keeps it with the cache, kv_drop above
  struct {
    bool armed = false;
    const uint64_t* words = nullptr;   // device: [n_clips][ld] words, AttnArgs::key_drop's layout
    const uint64_t* rows = nullptr;    // device: [n_clips][ld] words, AttnArgs::drop_rows' layout, or null
    int ld = 0;
    int layer_begin = 0, layer_end = 0;
  } drop;
  // depth lens (aigv_depth_lens_arm): armed for exactly the next aigv_llm_prefill, which copies the rows `rows` = [score rows | token rows] of the
  // residual stream after the embedding and after every layer into the caller's buffers (raw, and under the final norm) and runs the score head on
  // the score rows of every depth
  struct {
    bool armed = false;
    int n_score = 0, n_token = 0;
    int32_t rows[2 * AIGV_MAX_LENS_ROWS];
    bf16_t *hidden = nullptr, *normed = nullptr;   // device, the caller's: [llm_layers + 1][n_score + n_token][H]
    float* score = nullptr;                        // device, the caller's: [llm_layers + 1][n_score]
  } lens;
  int32_t* l_lensidx = nullptr;   // device [4 * AIGV_MAX_LENS_ROWS]: the armed pass's lens rows | their places among the consumed rows (row trimming)
  // The row options of a scoring pass: each armed for exactly the next aigv_llm_prefill.  What the eight share: rows - packed row numbers, copied on arming,
  // checked by the pass (inside [0, T), strictly ascending); all_rows (a scale only): every row the pass runs; the layer window lo <= li < hi; buf - device,
  // the caller's: [rows.size()][hi - lo][row width], slice li - lo belonging to layer li
  struct RowOpt {
    bool armed = false, all_rows = false;
    int lo = 0, hi = 0;
    std::vector<int32_t> rows;
    bf16_t* buf = nullptr;
  };
  // activation patching (aigv_stream_capture_arm / aigv_stream_patch_arm), rows of width H.  At the top of layer li the patch writes its slice over the rows
  // of the residual stream, then the capture copies its rows of the stream - as the layer consumes it - into its own
  RowOpt stream_patch, stream_cap;
  int32_t* l_streamidx = nullptr;   // device [2 * max_tokens]: the armed pass's patch rows | its capture rows
  // head knock-out / head patching (aigv_head_scale_arm / aigv_head_patch_arm / aigv_head_capture_arm), rows of width n_heads * D.  Between the attention of
  // layer li and its wo, on l_ao: first the scale (table row li, every head whose factor is not exactly 1), then the patch (the heads of bits[li - lo]), then
  // the capture (every head) - so a capture returns what wo consumes
  struct HeadRows : RowOpt {
    std::vector<uint64_t> bits;   // the patch: one mask per layer of the window (no list on arming: every head)
    std::vector<float> scale;     // the scale: [llm_layers][llm_heads]
  } head_scale, head_patch, head_cap;
  int32_t* l_headidx = nullptr;   // device [3 * max_tokens]: the armed pass's head-scale rows | head-patch rows | head-capture rows
  // MLP neuron knock-out / neuron patching (aigv_neuron_scale_arm / aigv_neuron_patch_arm / aigv_neuron_capture_arm), rows of width I or cols.size().  Between
  // the SwiGLU GEMM of layer li and its w2, on the row w2 consumes (l_ffn [T, I]; the streamed rows of the row-trimmed last layer: t_ffn): first the scale,
  // then the patch, then the capture - so a capture returns what w2 consumes.  cols empty and dense true: every neuron; else the sparse column list (capture,
  // patch: one list for the window; scale: (layer, column, factor) triples sorted by layer, sel_begin[l] .. sel_begin[l + 1] those of layer l)
  struct NeuronRows : RowOpt {
    bool dense = true;
    std::vector<int32_t> cols;
    std::vector<float> layer_scale;   // the scale, dense form: [llm_layers] (empty: none)
    std::vector<float> factors;       // the scale, sparse form: one per entry of cols
    std::vector<int32_t> sel_begin;   // the scale, sparse form: [llm_layers + 1]
  } neuron_scale, neuron_patch, neuron_cap;
  // ... and the eight in the order a layer applies them, with the words the passes' messages are built from: family, option, the arming entry point, and what
  // the last layer of a pass without output rows does not run for that family (the stream: nothing to skip).  DESIGN.md "Adding a pass option"
  struct RowOptEntry { RowOpt* opt; const char *family, *what, *arm, *skipped; };
  const RowOptEntry row_opts[8] = {
      {&stream_patch, "stream", "patch", "aigv_stream_patch_arm", nullptr},
      {&stream_cap, "stream", "capture", "aigv_stream_capture_arm", nullptr},
      {&head_scale, "head", "scale", "aigv_head_scale_arm", "attention"},
      {&head_patch, "head", "patch", "aigv_head_patch_arm", "attention"},
      {&head_cap, "head", "capture", "aigv_head_capture_arm", "attention"},
      {&neuron_scale, "neuron", "scale", "aigv_neuron_scale_arm", "MLP"},
      {&neuron_patch, "neuron", "patch", "aigv_neuron_patch_arm", "MLP"},
      {&neuron_cap, "neuron", "capture", "aigv_neuron_capture_arm", "MLP"}};
  // device: per option (scale | patch | capture) 3 * max_tokens ints - its packed rows | the activation rows of its last-layer launches | their side rows
  int32_t* l_neuronidx = nullptr;
  int32_t* l_neuroncol = nullptr;   // device [3 * AIGV_MAX_NEURON_SEL]: the scale's columns | the patch's | the capture's
  float* l_neuronfac = nullptr;     // device [AIGV_MAX_NEURON_SEL]: the scale's factors
  // profiling
  bool prof = false;
  int gemm_cls = AIGV_PROF_GEMM;   // class the GEMM launches are booked under: AIGV_PROF_GEMM_VIT inside aigv_vit_forward / aigv_project
  std::vector<aigv::ProfRec> recs;
  std::vector<hipEvent_t> ev_pool;
};

namespace aigv {

// records the message for aigv_last_error (of `c`, and of the calling thread) and returns `code`  (context.hip)
int fail(aigv_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, call)                                                                              \
  do {                                                                                               \
    hipError_t e_ = (call);                                                                          \
    if (e_ != hipSuccess) return fail(c, AIGV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define TRY(x)            \
  do {                    \
    int r_ = (x);         \
    if (r_ != 0) return r_; \
  } while (0)

template <typename T>
int dalloc(aigv_ctx* c, T** out, size_t count) {
  void* p = nullptr;
  const size_t bytes = (count ? count : 1) * sizeof(T);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return fail(c, AIGV_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  e = hipMemset(p, 0, bytes);
  if (e != hipSuccess) return fail(c, AIGV_ERR_HIP, "hipMemset failed: %s", hipGetErrorString(e));
  (c->ws_phase ? c->ws_allocs : c->allocs).push_back(p);
  *out = (T*)p;
  return 0;
}

// ---- profiling brackets --------------------------------------------------------------------------------
inline hipEvent_t get_event(aigv_ctx* c) {
  if (!c->ev_pool.empty()) {
    hipEvent_t e = c->ev_pool.back();
    c->ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
struct ProfScope {
  aigv_ctx* c;
  hipStream_t s;
  ProfRec r{};
  bool on;
  ProfScope(aigv_ctx* c_, int cls, double flops, double bytes, hipStream_t s_) : c(c_), s(s_), on(c_ && c_->prof) {
    if (!on) return;
    r.cls = cls; r.flops = flops; r.bytes = bytes;
    r.a = get_event(c); r.b = get_event(c);
    if (!r.a || !r.b) { on = false; return; }
    hipEventRecord(r.a, s);
  }
  ~ProfScope() {
    if (!on) return;
    hipEventRecord(r.b, s);
    c->recs.push_back(r);
  }
};

struct RowPlanScope {   // the InternLM2 layer helpers run under `rp` inside the scope
  aigv_ctx* c;
  RowPlanScope(aigv_ctx* c_, const RowPlan* rp) : c(c_) { c->cur_rp = rp; }
  ~RowPlanScope() { c->cur_rp = nullptr; }
};

struct SplitkVitScope {   // split-K launches inside the scope use the InternViT half of the context's scratch
  aigv_ctx* c;
  explicit SplitkVitScope(aigv_ctx* c_) : c(c_) { c->on_vit_front = true; }
  ~SplitkVitScope() { c->on_vit_front = false; }
};

struct GemmClassScope {   // GEMM launches inside the scope are booked under `cls` (per-class roofline entries of bench.py)
  aigv_ctx* c;
  int keep;
  GemmClassScope(aigv_ctx* c_, int cls) : c(c_), keep(c_->gemm_cls) { c->gemm_cls = cls; }
  ~GemmClassScope() { c->gemm_cls = keep; }
};

// ---- experiment knobs ------------------------------------------------------------------------------------------------------------
// The kernel files hold no mutable state: every launch carries its selectors (GemmArgs::order_sel / variant_sel, AttnArgs::waves), filled
// in from the context's own setting (aigv_ctx_tune / aigv_set_gemm_mode) or, where the context leaves a knob at -1 and for the
// context-free aigv_op_* entry points, from the process defaults (aigv_tune_*: tests and A/B scripts).  One value per AIGV_TUNE_* knob;
// defaults, value ranges and setters: the table in tune.hip.
struct Tune {
  int v[AIGV_TUNE_COUNT];
  constexpr int operator[](int knob) const { return v[knob]; }
};
extern Tune g_tune;   // the process defaults (tune.hip)
// one knob in force for a call: the context's own setting, else the process default
inline int tune_knob(const aigv_ctx* c, int knob) { return (c && c->tune[knob] >= 0) ? c->tune[knob] : g_tune.v[knob]; }
inline int resolved_gemm_mode(const aigv_ctx* c) { return tune_knob(c, AIGV_TUNE_GEMM_MODE); }
// ... and all of them
inline Tune tune_of(const aigv_ctx* c) {
  Tune t;
  for (int k = 0; k < AIGV_TUNE_COUNT; ++k) t.v[k] = tune_knob(c, k);
  return t;
}

// ---- the GEMM dispatcher (dispatch.hip) ------------------------------------------------------------------------------------------
GemmArgs gemm_args(const bf16_t* A, int lda, const bf16_t* W, int ldw, bf16_t* C, int ldc, int M, int N, int K);
// cu[0..n_seq]: row offsets of the sequences inside the activation matrices -> the plan and its device table (written on `s`)
int build_row_plan(aigv_ctx* c, RowPlan& rp, const int32_t* cu, int n_seq, hipStream_t s);
int launch_one(aigv_ctx* c, const GemmArgs& a, int epi, bool use256, hipStream_t s);    // one launch of the 256x256 / the 128x128 kernel
int run_gemm(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s);                   // batch-level cost model
int run_gemm_rows(aigv_ctx* c, const GemmArgs& a, int epi, const RowPlan& rp, hipStream_t s);   // rows follow the row plan
int run_gemm_full(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s);              // every row in full K on one tile kernel
int run_llm_gemm(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s);               // InternLM2 linears: the pass's row plan, else run_gemm
int run_gemm_fp8(aigv_ctx* c, const bf16_t* A, int lda, int K, const uint8_t* W8, const float* w_scale, bf16_t* C, int ldc, int T, int N,
                 int epi, const bf16_t* resid, int ldr, hipStream_t s);
const char* skinny_check(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, const bf16_t* resid, int ldr,
                         const bf16_t* out, int ldo, int epi);   // nullptr if run_skinny takes the layout
int run_skinny(aigv_ctx* c, const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, const bf16_t* bias,
               const bf16_t* resid, int ldr, bf16_t* out, int ldo, int epi, hipStream_t s, int p = 1);
constexpr size_t SPLITK_MAX_FLOATS = (size_t)64 << 20;   // 256 MB of fp32 split-K slabs: the planner never asks for more
int splitk_scratch(aigv_ctx* c, size_t need_floats, float** out);

// ---- the score-row attention probe of an armed pass (probe.hip) --------------------------------------------------------------------
// DisarmScope: the pass that finds the context armed - with the probe, a key-drop mask, the depth lens or any row option (aigv_ctx::row_opts; DESIGN.md "Adding
// a pass option") - disarms it on every way out.  probe_plan: the probe's arguments for this pass (rows validated against cu; off_host: keys cached in front of
// every sequence, or null), built ONCE per pass; probe_layer: the launch of layer li.
struct DisarmScope {
  aigv_ctx* c;
  explicit DisarmScope(aigv_ctx* c_) : c(c_) {}
  ~DisarmScope() {
    c->probe.armed = c->drop.armed = c->lens.armed = c->amap.armed = false;
    for (const aigv_ctx::RowOptEntry& e : c->row_opts) e.opt->armed = false;
  }
};
int probe_plan(aigv_ctx* c, const char* op, const int32_t* cu, int B, const int32_t* off_host, ProbeArgs* out);
int probe_layer(aigv_ctx* c, const ProbeArgs& plan, int li, bool cache, hipStream_t s);
// the attention flow map of an armed prefill (probe.hip): map_plan refuses what the pass cannot carry, checks every index (aigv_attn_map_check) and builds the arguments ONCE per pass, in front of
// its first launch; map_layer: the launch of layer li (nothing where the layer lies outside the window and no fold is asked for)
int map_plan(aigv_ctx* c, const int32_t* cu, int B, int keep_kv, AttnMapArgs* out);
int map_layer(aigv_ctx* c, const AttnMapArgs& plan, int li, hipStream_t s);
// the row list of a stream capture / patch against a pass of T packed rows and L layers (passes.hip; aigv_op_stream_rows shares it): every row inside
// [0, T), strictly ascending - so a patch's rows are unique - and the window 0 <= lo <= hi <= L
int stream_rows_check(aigv_ctx* c, const char* op, const int32_t* rows, int n, int T, int lo, int hi, int L);
extern double g_rate256;   // the cost model's throughput of the 256 kernel relative to the 128 kernel (aigv_tune_gemm overrides it)

}  // namespace aigv
