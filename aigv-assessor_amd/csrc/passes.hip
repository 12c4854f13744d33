// The passes of the C ABI (include/aigv_amd.h) over the gfx950 kernels: InternViT, the projectors, InternLM2 prefill / extend with the
// score and lm heads, the KV-cache operations and the decode step.  Host-side C++ only; every device op is one of the hand-written
// kernels, every GEMM goes through the dispatcher (dispatch.hip).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "ctx.h"

using namespace aigv;

// The row list of a stream capture / patch against the pass that runs it (ctx.h); `op`: what the message starts with.
namespace aigv {
int stream_rows_check(aigv_ctx* c, const char* op, const int32_t* rows, int n, int T, int lo, int hi, int L) {
  if (lo < 0 || lo > hi || hi > L) return fail(c, AIGV_ERR_ARG, "%s: depths [%d, %d) outside 0 <= lo <= hi <= %d", op, lo, hi, L);
  for (int i = 0; i < n; ++i) {
    if (rows[i] < 0 || rows[i] >= T) return fail(c, AIGV_ERR_ARG, "%s: row %d (packed row %d) outside [0, %d), the rows the pass runs", op, i, rows[i], T);
    if (i > 0 && rows[i] <= rows[i - 1])
      return fail(c, AIGV_ERR_ARG, "%s: rows %d and %d (packed rows %d, %d) are not strictly ascending", op, i - 1, i, rows[i - 1], rows[i]);
  }
  return 0;
}
}  // namespace aigv

extern "C" {

// ---- InternViT ---------------------------------------------------------------------------------------------
static int vit_norm(aigv_ctx* c, const bf16_t* x, const bf16_t* w, const bf16_t* b, bf16_t* y, int rows, hipStream_t s) {
  const aigv_config& k = c->cfg;
  if (k.vit_norm_rms) HIPCHK(c, aigv_launch_rmsnorm(x, k.vit_hidden, w, y, k.vit_hidden, rows, k.vit_hidden, k.vit_eps, nullptr, s));
  else HIPCHK(c, aigv_launch_layernorm(x, k.vit_hidden, w, b, y, k.vit_hidden, rows, k.vit_hidden, k.vit_eps, s));
  return 0;
}

// The InternViT attention map of an armed pass (aigv_vit_attention_arm; vitmap.hip): the arguments of layer li's launch for the chunk of F frames that
// starts at frame f0.  Only the frame count and the output address differ from launch to launch.
static VitMapArgs vit_map_args(const aigv_ctx* c, int f0, int F, int li) {
  const aigv_config& k = c->cfg;
  const auto& vm = c->vmap;
  VitMapArgs a{};
  a.q = c->v_qkv; a.k = c->v_qkv + k.vit_hidden; a.ldq = a.ldk = 3 * k.vit_hidden;
  a.n_seq = F; a.S = c->S; a.n_heads = k.vit_heads;
  a.post_div = sqrtf((float)c->vit_head_dim);
  a.per_head = vm.per_head;
  const size_t map_floats = (size_t)(vm.per_head ? k.vit_heads : 1) * c->S * c->S;
  a.out_frame_stride = (size_t)(vm.hi - vm.lo) * map_floats;
  a.out = vm.out + (size_t)f0 * a.out_frame_stride + (size_t)(li - vm.lo) * map_floats;
  a.stats = c->v_mapstats;
  return a;
}

struct VitDisarmScope {   // the aigv_vit_forward that finds the context armed disarms it on every way out
  aigv_ctx* c;
  explicit VitDisarmScope(aigv_ctx* c_) : c(c_) {}
  ~VitDisarmScope() { c->vmap.armed = false; c->vdrop.armed = false; }
};

int aigv_vit_forward(aigv_ctx* c, const void* frames, int n_frames, void* out_tokens, void* stream) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: null argument");
  VitDisarmScope disarm(c);
  if (!frames || !out_tokens) return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: null argument");
  if (!c->finalized) return fail(c, AIGV_ERR_STATE, "aigv_vit_forward: call aigv_finalize_weights first");
  const aigv_config& k = c->cfg;
  if (n_frames <= 0 || n_frames > k.max_frames) return fail(c, AIGV_ERR_ARG, "n_frames %d outside 1..%d", n_frames, k.max_frames);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  GemmClassScope gcls(c, AIGV_PROF_GEMM_VIT);
  SplitkVitScope svs(c);
  const int Hv = k.vit_hidden, Iv = k.vit_inter;
  int n_layers = k.vit_layers;
  if (k.select_layer != -1) n_layers = k.select_layer < 0 ? k.vit_layers + 1 + k.select_layer : k.select_layer;
  if (n_layers < 0 || n_layers > k.vit_layers) return fail(c, AIGV_ERR_ARG, "select_layer %d out of range", k.select_layer);
  const bool mapped = c->vmap.armed;
  if (mapped) {   // refused before anything is launched: the window against the layers THIS pass runs (select_layer's count), every index of the launches
    const auto& vm = c->vmap;
    if (vm.lo < 0 || vm.lo >= vm.hi || vm.hi > n_layers)
      return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: attention map armed for layers [%d, %d), outside 0 <= lo < hi <= %d, the layers the pass runs", vm.lo, vm.hi, n_layers);
    if (!c->v_mapstats) return fail(c, AIGV_ERR_STATE, "aigv_vit_forward: attention map armed on a context without its stats scratch");
    if (const char* m = aigv_vit_map_check(vit_map_args(c, 0, std::min(k.vit_chunk, n_frames), vm.lo), c->vit_head_dim)) return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: %s", m);
  }
  const bool masked = c->vdrop.armed;
  if (masked) {   // refused before anything is launched, like the map's window
    const auto& vd = c->vdrop;
    if (mapped) return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: armed with both the attention map and a patch mask: the map kernel does not know the mask");
    if (vd.lo < 0 || vd.lo >= vd.hi || vd.hi > n_layers)
      return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: patch mask armed for layers [%d, %d), outside 0 <= lo < hi <= %d, the layers the pass runs", vd.lo, vd.hi, n_layers);
    if (vd.ld < (c->S + 63) / 64) return fail(c, AIGV_ERR_ARG, "aigv_vit_forward: patch mask with %d words per frame, below ceil(%d / 64)", vd.ld, c->S);
  }
  const size_t frame_elems = (size_t)k.num_channels * k.image_size * k.image_size;
  for (int f0 = 0; f0 < n_frames; f0 += k.vit_chunk) {
    const int F = std::min(k.vit_chunk, n_frames - f0);
    const int rows = F * c->S;
    const bf16_t* fr = (const bf16_t*)frames + (size_t)f0 * frame_elems;
    {   // every frame is a sequence of S rows; the table is written by every pass (build_row_plan)
      std::vector<int32_t> cu(F + 1);
      for (int i = 0; i <= F; ++i) cu[i] = i * c->S;
      TRY(build_row_plan(c, c->rp_vit, cu.data(), F, s));
    }
    const RowPlan& rp = c->rp_vit;
    // patch embed: im2col + GEMM with the bias / position / row-remap epilogue (modeling_intern_vit.py:95-107)
    HIPCHK(c, aigv_launch_im2col(fr, F, k.num_channels, k.image_size, k.patch_size, c->Kp, c->v_col, s));
    HIPCHK(c, aigv_launch_cls_rows(c->cls_pos, c->v_x, F, c->S, Hv, s));
    {
      GemmArgs a = gemm_args(c->v_col, c->Kp, c->patch_w, c->Kp, c->v_x, Hv, F * c->np, Hv, c->Kp);
      a.bias = c->patch_b; a.pos = c->pos; a.np = c->np;
      // (every row in full K on ONE tile kernel chosen by the shape of a frame: batch-invariant)
      TRY(launch_one(c, a, EPI_PATCH, Hv % 256 == 0 && resolved_gemm_mode(c) != 1, s));
    }
    for (int li = 0; li < n_layers; ++li) {
      const VitLayer& L = c->vit[li];
      TRY(vit_norm(c, c->v_x, L.n1w, L.n1b, c->v_t, rows, s));
      {
        GemmArgs a = gemm_args(c->v_t, Hv, L.qkv_w, Hv, c->v_qkv, 3 * Hv, rows, 3 * Hv, Hv);
        a.bias = L.qkv_b;
        TRY(run_gemm_rows(c, a, EPI_STORE, rp, s));
      }
      if (k.vit_qk_norm) {  // full-width RMSNorm of q and k, in place (modeling_intern_vit.py:148-151)
        HIPCHK(c, aigv_launch_rmsnorm(c->v_qkv, 3 * Hv, L.qn, c->v_qkv, 3 * Hv, rows, Hv, k.vit_eps, nullptr, s));
        HIPCHK(c, aigv_launch_rmsnorm(c->v_qkv + Hv, 3 * Hv, L.kn, c->v_qkv + Hv, 3 * Hv, rows, Hv, k.vit_eps, nullptr, s));
      }
      if (mapped && li >= c->vmap.lo && li < c->vmap.hi) HIPCHK(c, aigv_launch_vit_map(vit_map_args(c, f0, F, li), c->vit_head_dim, s));   // (reads q and k; writes the caller's buffer and v_mapstats alone)
      {
        AttnArgs a{};
        a.q = c->v_qkv; a.k = c->v_qkv + Hv; a.v = c->v_qkv + 2 * Hv;
        a.ldq = a.ldk = a.ldv = 3 * Hv;
        a.o = c->v_ao; a.ldo = Hv;
        a.cu = c->v_cu; a.n_seq = F; a.max_len = c->S;
        a.n_heads = a.n_kv_heads = k.vit_heads;
        a.q_group_stride = a.kv_head_stride = c->vit_head_dim;
        a.causal = 0; a.post_div = 1.0f; a.q_prescale = 1.0f / sqrtf((float)c->vit_head_dim);
        a.round_scores = c->attn_round_scores; a.waves = tune_knob(c, AIGV_TUNE_ATTN_WAVES); a.lead_key = tune_knob(c, AIGV_TUNE_ATTN_LEAD_KEY);
        a.uniform_len = 1;
        const bool drop = masked && li >= c->vdrop.lo && li < c->vdrop.hi;
        if (drop) { a.key_drop = c->vdrop.words + (size_t)f0 * c->vdrop.ld; a.ld_drop = c->vdrop.ld; }   // (the chunk's own frames)
        if (const char* m = aigv_attn_check(a, c->vit_head_dim, drop)) return fail(c, AIGV_ERR_ARG, "%s", m);
        ProfScope ps(c, AIGV_PROF_ATTN_VIT, 4.0 * F * (double)c->S * c->S * Hv, 2.0 * 4 * rows * (double)Hv, s);
        HIPCHK(c, aigv_launch_attention(a, c->vit_head_dim, s));
      }
      {
        GemmArgs a = gemm_args(c->v_ao, Hv, L.proj_w, Hv, c->v_x, Hv, rows, Hv, Hv);
        a.bias = L.proj_b; a.ls = L.ls1; a.resid = c->v_x; a.ldr = Hv;
        TRY(run_gemm_rows(c, a, EPI_LS_RESID, rp, s));
      }
      TRY(vit_norm(c, c->v_x, L.n2w, L.n2b, c->v_t, rows, s));
      {
        GemmArgs a = gemm_args(c->v_t, Hv, L.fc1_w, Hv, c->v_h, Iv, rows, Iv, Hv);
        a.bias = L.fc1_b;
        TRY(run_gemm_rows(c, a, EPI_GELU, rp, s));
      }
      {
        GemmArgs a = gemm_args(c->v_h, Iv, L.fc2_w, Iv, c->v_x, Hv, rows, Hv, Iv);
        a.bias = L.fc2_b; a.ls = L.ls2; a.resid = c->v_x; a.ldr = Hv;
        TRY(run_gemm_rows(c, a, EPI_LS_RESID, rp, s));
      }
    }
    HIPCHK(c, aigv_launch_pixel_shuffle(c->v_x, c->grid, Hv, (bf16_t*)out_tokens + (size_t)f0 * c->ntok * c->proj_in, F, s));
  }
  return 0;
}

int aigv_vit_attention_arm(aigv_ctx* c, float* out_dev, int layer_lo, int layer_hi, int per_head) {
  const char* op = "aigv_vit_attention_arm";
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (!out_dev) return fail(c, AIGV_ERR_ARG, "%s: null out_dev", op);
  if ((uintptr_t)out_dev & 3) return fail(c, AIGV_ERR_ARG, "%s: out_dev must be 4-byte aligned", op);
  // the window is refused by the PASS, with a message: it is what knows how many layers it runs (select_layer)
  auto& vm = c->vmap;
  vm.out = out_dev; vm.lo = layer_lo; vm.hi = layer_hi; vm.per_head = per_head ? 1 : 0;
  vm.armed = true;
  return 0;
}

int aigv_vit_key_drop_arm(aigv_ctx* c, const uint64_t* words_dev, int ld_words, int layer_lo, int layer_hi) {
  const char* op = "aigv_vit_key_drop_arm";
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (!words_dev) return fail(c, AIGV_ERR_ARG, "%s: null words_dev", op);
  if ((uintptr_t)words_dev & 7) return fail(c, AIGV_ERR_ARG, "%s: words_dev must be 8-byte aligned", op);
  if (ld_words < (c->S + 63) / 64) return fail(c, AIGV_ERR_ARG, "%s: ld_words = %d is below ceil(%d / 64) words per frame", op, ld_words, c->S);
  // the window is refused by the PASS, with a message: it is what knows how many layers it runs (select_layer)
  auto& vd = c->vdrop;
  vd.words = words_dev; vd.ld = ld_words; vd.lo = layer_lo; vd.hi = layer_hi;
  vd.armed = true;
  return 0;
}

int aigv_project(aigv_ctx* c, const void* tokens, int rows, void* out, void* stream) {
  if (!c || !tokens || !out) return fail(c, AIGV_ERR_ARG, "aigv_project: null argument");
  if (!c->finalized) return fail(c, AIGV_ERR_STATE, "aigv_project: call aigv_finalize_weights first");
  if (rows <= 0) return fail(c, AIGV_ERR_ARG, "aigv_project: rows must be positive");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden, Pin = c->proj_in;
  GemmClassScope gcls(c, AIGV_PROF_GEMM_VIT);
  const int chunk = k.vit_chunk * c->ntok;
  for (int r0 = 0; r0 < rows; r0 += chunk) {
    const int R = std::min(chunk, rows - r0);
    const bf16_t* x = (const bf16_t*)tokens + (size_t)r0 * Pin;
    HIPCHK(c, aigv_launch_layernorm(x, Pin, c->p_ln_w[0], c->p_ln_b[0], c->p_t, Pin, R, Pin, 1e-5f, s));
    {
      GemmArgs a = gemm_args(c->p_t, Pin, c->p_w1[0], Pin, c->p_mid, H, R, H, Pin);
      a.bias = c->p_b1[0];
      TRY(run_gemm_full(c, a, EPI_GELU, s));
    }
    {
      GemmArgs a = gemm_args(c->p_mid, H, c->p_w2[0], H, (bf16_t*)out + (size_t)r0 * H, H, R, H, H);
      a.bias = c->p_b2[0];
      TRY(run_gemm_full(c, a, EPI_STORE, s));
    }
  }
  return 0;
}

int aigv_motion_project(aigv_ctx* c, const void* motion_feature, int n_clips, void* out, void* stream) {
  if (!c || !motion_feature || !out) return fail(c, AIGV_ERR_ARG, "aigv_motion_project: null argument");
  if (!c->finalized) return fail(c, AIGV_ERR_STATE, "aigv_motion_project: call aigv_finalize_weights first");
  if (n_clips <= 0 || n_clips > c->cfg.max_seqs) return fail(c, AIGV_ERR_ARG, "n_clips %d outside 1..%d", n_clips, c->cfg.max_seqs);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden, Md = k.motion_dim;
  // scratch: p_t (>= ntok*proj_in elements) holds the normalised feature, p_mid the hidden layer
  if ((size_t)n_clips * Md > (size_t)k.vit_chunk * c->ntok * c->proj_in || n_clips > k.vit_chunk * c->ntok)
    return fail(c, AIGV_ERR_STATE, "motion batch does not fit the projector workspace");
  HIPCHK(c, aigv_launch_layernorm((const bf16_t*)motion_feature, Md, c->p_ln_w[1], c->p_ln_b[1], c->p_t, Md, n_clips, Md, 1e-5f, s));
  for (int r0 = 0; r0 < n_clips; r0 += 64) {
    const int R = std::min(64, n_clips - r0);
    TRY(run_skinny(c, c->p_t + (size_t)r0 * Md, Md, R, c->p_w1[1], Md, H, Md, c->p_b1[1], nullptr, 0,
                   c->p_mid + (size_t)r0 * H, H, SK_GELU, s, 0));
    TRY(run_skinny(c, c->p_mid + (size_t)r0 * H, H, R, c->p_w2[1], H, H, H, c->p_b2[1], nullptr, 0,
                   (bf16_t*)out + (size_t)r0 * H, H, SK_STORE, s, 0));
  }
  return 0;
}

// ---- InternLM2 -----------------------------------------------------------------------------------------------
// rows whose final hidden state is consumed: [score rows (one per clip) | logit rows], validated and uploaded to l_rowidx
static int upload_out_rows(aigv_ctx* c, const int32_t* score_rows, bool with_score, int B, const int32_t* logit_rows, int R,
                           int total_rows, hipStream_t s) {
  const aigv_config& k = c->cfg;
  if (R > k.max_out_rows) return fail(c, AIGV_ERR_ARG, "%d logit rows exceed max_out_rows %d", R, k.max_out_rows);
  c->h_rowidx.clear();
  for (int i = 0; i < (with_score ? B : 0); ++i) c->h_rowidx.push_back(score_rows[i]);
  for (int i = 0; i < R; ++i) c->h_rowidx.push_back(logit_rows[i]);
  for (int v : c->h_rowidx)
    if (v < 0 || v >= total_rows) return fail(c, AIGV_ERR_ARG, "output row index %d outside 0..%d", v, total_rows - 1);
  if (!c->h_rowidx.empty()) HIPCHK(c, aigv_launch_write_ints(c->h_rowidx.data(), (int)c->h_rowidx.size(), c->l_rowidx, s));
  return 0;
}

// final RMSNorm + heads on the consumed rows.  compact: `hidden` already holds exactly those rows, in l_rowidx order.
static int final_rows(aigv_ctx* c, float* score, int B, int R, int64_t* argmax, const bf16_t* hidden, bool compact, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden;
  const int nS = score ? B : 0;
  const int n = nS + R;
  if (n == 0) return 0;
  // final RMSNorm only on the rows that are consumed (modeling_internlm2.py:984)
  HIPCHK(c, aigv_launch_rmsnorm(hidden, H, c->final_norm, c->l_rows, H, n, H, k.rms_eps, compact ? nullptr : c->l_rowidx, s));
  for (int b0 = 0; b0 < nS; b0 += 64) {
    // NB: the reference's NaN guard looks at the whole batch slice; batches above 64 clips are guarded per 64
    ScoreHeadArgs a = c->score;
    a.x = c->l_rows + (size_t)b0 * H; a.ldx = H; a.B = std::min(64, nS - b0); a.score = score + b0;
    HIPCHK(c, aigv_launch_score_head(a, c->l_score_ws, s));
  }
  for (int r0 = 0; r0 < R; r0 += 64) {
    const int rr = std::min(64, R - r0);
    ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * rr * (double)k.vocab * H, 2.0 * (double)k.vocab * H, s);
    HIPCHK(c, aigv_launch_lm_head_argmax(c->l_rows + (size_t)(nS + r0) * H, rr, H, c->lm_head, k.vocab, c->l_packed,
                                         argmax + r0, nullptr, s));
  }
  return 0;
}

// ---- the two halves of an InternLM2 decoder layer around its attention, shared by aigv_llm_prefill and aigv_llm_extend (rows of
// c->l_h, T of them).  fp8 mode: every linear of the layer in e4m3 except the post-attention half of the LAST layer (wo, w1|w3, w2
// there act on the few consumed rows - weight streaming, nothing for fp8 MFMA to gain - and stay bf16 with or without row trimming).
// attention_norm -> wqkv -> RoPE on K in place (one of g + 2 slots per group; the query heads are rotated by the attention kernel as
// it loads them)
static int llm_layer_qkv(aigv_ctx* c, int li, int T, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const LlmLayer& L = c->llm[li];
  const int H = k.llm_hidden, D = c->head_dim, g = c->g, nkv = k.llm_kv_heads;
  if (c->fp8_llm) {
    HIPCHK(c, aigv_launch_rmsnorm_quant_fp8(c->l_h, H, L.an, c->q8, H, c->q8_scale, T, H, k.rms_eps, s));
    TRY(run_gemm_fp8(c, nullptr, H, H, c->llm8[li].wqkv, c->llm8[li].s_wqkv, c->l_qkv, c->qkv_out, T, c->qkv_out, EPI_STORE, nullptr, 0, s));
  } else {
    HIPCHK(c, aigv_launch_rmsnorm(c->l_h, H, L.an, c->l_t, H, T, H, k.rms_eps, nullptr, s));
    TRY(run_llm_gemm(c, gemm_args(c->l_t, H, L.wqkv, H, c->l_qkv, c->qkv_out, T, c->qkv_out, H), EPI_STORE, s));
  }
  HIPCHK(c, aigv_launch_rope(c->l_qkv, c->qkv_out, c->l_pos, c->rope_cos, c->rope_sin, T, 1, g + 2, nkv, D, s, g));
  return 0;
}

// MLP neuron knock-out / neuron patching: what an armed pass launches between a SwiGLU GEMM and its w2.  Built once per pass (neuron_plan); the row
// tables live in l_neuronidx, per option o (0 scale, 1 patch, 2 capture) at o * 3 * max_tokens: its packed rows | the activation rows of its last-layer
// launches | their side rows.  The last-layer lists hold, in launch order, the entries of the streamed chunks (activation row: the position inside the
// 64-row chunk of t_ffn) and then, for a mixed batch, those of every other selected row (activation row: the packed row of l_ffn).
struct NeuronPlan {
  bool split_last = false;            // the last layer finishes (some) rows on the weight-streaming path: its launches take the last-layer lists
  struct Last { std::vector<int32_t> act, side; std::vector<int> chunk_begin; int rest_begin = 0; } last[3];
};
enum { NEURON_AT_ROWS = -1, NEURON_AT_REST = -2 };   // where a hook acts: every row of l_ffn | l_ffn without the streamed rows | (>= 0) streamed chunk number

// the launches of layer li on `act` [.., I]: scale, then patch, then capture; n_all: the rows `act` holds (what a scale of every row covers)
static int neuron_hook(aigv_ctx* c, const NeuronPlan& P, int li, bf16_t* act, int where, int n_all, hipStream_t s) {
  const int I = c->cfg.llm_inter;
  const size_t mt = (size_t)c->cfg.max_tokens;
  const bool last = P.split_last && li == c->cfg.llm_layers - 1;
  const aigv_ctx::NeuronRows* opt[3] = {&c->neuron_scale, &c->neuron_patch, &c->neuron_cap};
  for (int o = 0; o < 3; ++o) {
    const aigv_ctx::NeuronRows& r = *opt[o];
    if (!r.armed || li < r.lo || li >= r.hi) continue;
    const int32_t* base = c->l_neuronidx + (size_t)o * 3 * mt;
    const int32_t *idx = nullptr, *sidx = nullptr;
    int n = n_all;
    if (!r.all_rows) {
      if (!last) { idx = base; n = (int)r.rows.size(); }
      else {
        const NeuronPlan::Last& q = P.last[o];
        const int b = where == NEURON_AT_REST ? q.rest_begin : q.chunk_begin[where];
        const int e = where == NEURON_AT_REST ? (int)q.act.size() : q.chunk_begin[where + 1];
        idx = base + mt + b; sidx = base + 2 * mt + b; n = e - b;
      }
    }
    if (o == 0) {
      if (!r.layer_scale.empty())
        HIPCHK(c, aigv_launch_neuron_rows(act, I, idx, nullptr, n, nullptr, 1, 0, I, nullptr, 0, NEURON_SCALE, nullptr, r.layer_scale[li], s));
      const int b = r.sel_begin.empty() ? 0 : r.sel_begin[li], e = r.sel_begin.empty() ? 0 : r.sel_begin[li + 1];
      if (e > b) HIPCHK(c, aigv_launch_neuron_rows(act, I, idx, nullptr, n, nullptr, 1, 0, I, c->l_neuroncol + b, e - b, NEURON_SCALE, c->l_neuronfac + b, 1.0f, s));
    } else {
      const int32_t* cols = r.dense ? nullptr : c->l_neuroncol + (size_t)o * AIGV_MAX_NEURON_SEL;
      if (r.dense || !r.cols.empty())
        HIPCHK(c, aigv_launch_neuron_rows(act, I, idx, sidx, n, r.buf, r.hi - r.lo, li - r.lo, I, cols, (int)r.cols.size(), o == 1 ? NEURON_PATCH : NEURON_CAPTURE, nullptr, 1.0f, s));
    }
  }
  return 0;
}

// The tables of the armed neuron options go up on this stream, and the plan of their last-layer launches is built.  In the last layer of a trimmed or mixed
// batch the value captured, patched or scaled for a row is the input of the w2 launch whose output the pass keeps for it: the streamed rows' (small_rows, 64 at
// a time) is t_ffn - the packed row translated to (chunk, position), the side row passed beside it; trim: no other row's MLP runs; mixed: every other row's is l_ffn
static int neuron_plan(aigv_ctx* c, const std::vector<int32_t>& small_rows, bool trim, bool mixed, hipStream_t s, NeuronPlan* plan) {
  const aigv_config& k = c->cfg;
  const aigv_ctx::NeuronRows* opt[3] = {&c->neuron_scale, &c->neuron_patch, &c->neuron_cap};
  plan->split_last = trim || mixed;
  const int last = k.llm_layers - 1, n_fin = (int)small_rows.size();
  for (int o = 0; o < 3; ++o) {
    const aigv_ctx::NeuronRows& r = *opt[o];
    if (!r.armed) continue;
    int32_t* base = c->l_neuronidx + (size_t)o * 3 * k.max_tokens;
    if (!r.all_rows) HIPCHK(c, aigv_launch_write_ints(r.rows.data(), (int)r.rows.size(), base, s));
    if (!r.cols.empty()) HIPCHK(c, aigv_launch_write_ints(r.cols.data(), (int)r.cols.size(), c->l_neuroncol + (size_t)o * AIGV_MAX_NEURON_SEL, s));
    if (!r.factors.empty()) HIPCHK(c, aigv_launch_write_ints((const int32_t*)r.factors.data(), (int)r.factors.size(), (int32_t*)c->l_neuronfac, s));
    if (!plan->split_last || r.all_rows || last < r.lo || last >= r.hi) continue;
    NeuronPlan::Last& q = plan->last[o];
    std::vector<char> streamed(r.rows.size(), 0);
    for (int r0 = 0; r0 < n_fin; r0 += 64) {
      q.chunk_begin.push_back((int)q.act.size());
      for (int p = r0; p < std::min(n_fin, r0 + 64); ++p) {
        const auto it = std::lower_bound(r.rows.begin(), r.rows.end(), small_rows[p]);
        if (it == r.rows.end() || *it != small_rows[p]) continue;
        q.act.push_back(p - r0); q.side.push_back((int32_t)(it - r.rows.begin()));
        streamed[it - r.rows.begin()] = 1;
      }
    }
    q.chunk_begin.push_back((int)q.act.size());
    q.rest_begin = (int)q.act.size();
    if (mixed)
      for (size_t i = 0; i < r.rows.size(); ++i) if (!streamed[i]) { q.act.push_back(r.rows[i]); q.side.push_back((int32_t)i); }
    if ((int)q.act.size() > k.max_tokens) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: the neuron options' last-layer row list (%d entries) exceeds max_tokens = %d", (int)q.act.size(), k.max_tokens);
    if (!q.act.empty()) {
      HIPCHK(c, aigv_launch_write_ints(q.act.data(), (int)q.act.size(), base + k.max_tokens, s));
      HIPCHK(c, aigv_launch_write_ints(q.side.data(), (int)q.side.size(), base + 2 * (size_t)k.max_tokens, s));
    }
  }
  return 0;
}

// activation patching: the stream layer li consumes - first the patch's rows written over it, then the capture's rows read from it (so a capture armed beside
// a patch sees the patched rows); one launch each.  Row tables: l_streamidx, the patch's | the capture's
static int stream_hook(aigv_ctx* c, int li, hipStream_t s) {
  const int H = c->cfg.llm_hidden;
  const aigv_ctx::RowOpt* opt[2] = {&c->stream_patch, &c->stream_cap};
  for (int o = 0; o < 2; ++o) {
    const aigv_ctx::RowOpt& r = *opt[o];
    if (r.armed && li >= r.lo && li < r.hi)
      HIPCHK(c, aigv_launch_stream_rows(c->l_h, H, c->l_streamidx + (size_t)o * c->cfg.max_tokens, (int)r.rows.size(), r.buf, r.hi - r.lo, li - r.lo, H, o == 0, s));
  }
  return 0;
}

// head knock-out / head patching: l_ao [T, n_heads * D] as wo of layer li consumes it - scale, then patch, then capture; at most one launch each (a table row
// of ones: none).  Row tables: l_headidx, the scale's | the patch's | the capture's
static int head_hook(aigv_ctx* c, int li, int T, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden, D = c->head_dim;
  const size_t mt = (size_t)k.max_tokens;
  const aigv_ctx::HeadRows &hs = c->head_scale, &hp = c->head_patch, &hc = c->head_cap;
  if (hs.armed)
    HIPCHK(c, aigv_launch_head_rows(c->l_ao, H, hs.all_rows ? nullptr : c->l_headidx, hs.all_rows ? T : (int)hs.rows.size(), nullptr, 1, 0, k.llm_heads, D, HEAD_SCALE,
                                    ~(uint64_t)0, hs.scale.data() + (size_t)li * k.llm_heads, s));
  if (hp.armed && li >= hp.lo && li < hp.hi)
    HIPCHK(c, aigv_launch_head_rows(c->l_ao, H, c->l_headidx + mt, (int)hp.rows.size(), hp.buf, hp.hi - hp.lo, li - hp.lo, k.llm_heads, D, HEAD_PATCH,
                                    hp.bits[li - hp.lo], nullptr, s));
  if (hc.armed && li >= hc.lo && li < hc.hi)
    HIPCHK(c, aigv_launch_head_rows(c->l_ao, H, c->l_headidx + 2 * mt, (int)hc.rows.size(), hc.buf, hc.hi - hc.lo, li - hc.lo, k.llm_heads, D, HEAD_CAPTURE,
                                    ~(uint64_t)0, nullptr, s));
  return 0;
}

// h += wo(attention output);  h += w2(silu(w1 n) * w3 n), n = ffn_norm(h); np (an armed pass): its neuron launches between the SwiGLU GEMM and w2
static int llm_layer_post(aigv_ctx* c, int li, int T, hipStream_t s, const NeuronPlan* np = nullptr, int where = NEURON_AT_ROWS) {
  const aigv_config& k = c->cfg;
  const LlmLayer& L = c->llm[li];
  const int H = k.llm_hidden, I = k.llm_inter;
  if (c->fp8_llm && li != k.llm_layers - 1) {
    const LlmLayerFp8& Q = c->llm8[li];
    TRY(run_gemm_fp8(c, c->l_ao, H, H, Q.wo, Q.s_wo, c->l_h, H, T, H, EPI_RESID, c->l_h, H, s));
    HIPCHK(c, aigv_launch_rmsnorm_quant_fp8(c->l_h, H, L.fn, c->q8, H, c->q8_scale, T, H, k.rms_eps, s));
    TRY(run_gemm_fp8(c, nullptr, H, H, Q.w13, Q.s_w13, c->l_ffn, I, T, 2 * I, EPI_SWIGLU, nullptr, 0, s));
    if (np) TRY(neuron_hook(c, *np, li, c->l_ffn, where, T, s));   // (l_ffn is bf16 here too: run_gemm_fp8 quantises it afterwards)
    TRY(run_gemm_fp8(c, c->l_ffn, I, I, Q.w2, Q.s_w2, c->l_h, H, T, H, EPI_RESID, c->l_h, H, s));
    return 0;
  }
  {
    GemmArgs a = gemm_args(c->l_ao, H, L.wo, H, c->l_h, H, T, H, H);
    a.resid = c->l_h; a.ldr = H;
    TRY(run_llm_gemm(c, a, EPI_RESID, s));
  }
  HIPCHK(c, aigv_launch_rmsnorm(c->l_h, H, L.fn, c->l_t, H, T, H, k.rms_eps, nullptr, s));
  TRY(run_llm_gemm(c, gemm_args(c->l_t, H, L.w13, H, c->l_ffn, I, T, 2 * I, H), EPI_SWIGLU, s));
  if (np) TRY(neuron_hook(c, *np, li, c->l_ffn, where, T, s));
  GemmArgs a = gemm_args(c->l_ffn, I, L.w2, I, c->l_h, H, T, H, I);
  a.resid = c->l_h; a.ldr = H;
  TRY(run_llm_gemm(c, a, EPI_RESID, s));
  return 0;
}

// The decode state of the N kept sequences, from their lengths h_kvlen: position of the next token | sequence | visible KV length | slot (-1:
// a text token), uploaded once and advanced on the device (aigv_launch_advance)
static int upload_decode_state(aigv_ctx* c, int N, hipStream_t s) {
  c->h_dec.resize((size_t)4 * N);
  for (int i = 0; i < N; ++i) {
    const int len = c->h_kvlen[i];
    c->h_dec[i] = len; c->h_dec[N + i] = i; c->h_dec[2 * N + i] = len + 1; c->h_dec[3 * N + i] = -1;
  }
  HIPCHK(c, aigv_launch_write_ints(c->h_dec.data(), N, c->dec_pos, s));
  HIPCHK(c, aigv_launch_write_ints(c->h_dec.data() + N, N, c->dec_seq, s));
  HIPCHK(c, aigv_launch_write_ints(c->h_dec.data() + 2 * N, N, c->dec_kvlen, s));
  HIPCHK(c, aigv_launch_write_ints(c->h_dec.data() + 3 * N, N, c->dec_slot, s));
  c->kv_seqs = N;
  return 0;
}

// The AttnArgs that aigv_llm_prefill and aigv_llm_extend share: causal GQA attention of the rows of l_qkv, the query heads rotated as they
// are loaded.  The caller adds where K / V live (k, v, ldk, ldv, kv_head_stride; the cache: kv_seq_stride, kv_off), max_len and q_tail.
static AttnArgs llm_attn_args(const aigv_ctx* c, int B) {
  const aigv_config& k = c->cfg;
  const int D = c->head_dim;
  AttnArgs a{};
  a.q = c->l_qkv; a.ldq = c->qkv_out;
  a.o = c->l_ao; a.ldo = k.llm_hidden;
  a.cu = c->l_cu; a.n_seq = B;
  a.n_heads = k.llm_heads; a.n_kv_heads = k.llm_kv_heads;
  a.q_group_stride = (c->g + 2) * D;
  a.causal = 1; a.post_div = sqrtf((float)D); a.q_prescale = 1.0f;
  a.round_scores = c->attn_round_scores; a.waves = tune_knob(c, AIGV_TUNE_ATTN_WAVES);
  a.rope_pos = c->l_pos; a.rope_cos = c->rope_cos; a.rope_sin = c->rope_sin;
  a.rope_pos_is_row = 1;   // l_pos[t] = t - cu[seq] (+ the cached length): aigv_launch_seqpos
  return a;
}

// the first armed row option of a family ("stream", "head", "neuron") in the order a layer applies them: the one a refusal names; null: none is armed
static const aigv_ctx::RowOptEntry* first_armed(const aigv_ctx* c, const char* family) {
  for (const aigv_ctx::RowOptEntry& e : c->row_opts)
    if (e.opt->armed && !strcmp(e.family, family)) return &e;
  return nullptr;
}

// does the armed option act in layer `last`?  A scale: a factor there that is not exactly 1; a patch, a capture: the window
static bool acts_in_layer(const aigv_ctx* c, const aigv_ctx::RowOpt* r, int last) {
  if (r == &c->head_scale) {
    const float* f = c->head_scale.scale.data() + (size_t)last * c->cfg.llm_heads;
    return std::any_of(f, f + c->cfg.llm_heads, [](float x) { return x != 1.0f; });
  }
  if (r == &c->neuron_scale) {
    const aigv_ctx::NeuronRows& ns = c->neuron_scale;
    return (!ns.layer_scale.empty() && ns.layer_scale[last] != 1.0f) || (!ns.sel_begin.empty() && ns.sel_begin[last + 1] > ns.sel_begin[last]);
  }
  return r->lo <= last && last < r->hi;
}

// What aigv_llm_prefill is armed with, against the pass: T packed rows, nS score rows and R logit rows.  The row options family by family - a pass that keeps
// its KV cache takes none (they are the scoring pass's: the paths that continue from a cache do not carry them); the row lists and windows against T and the L
// layers; a pass without output rows breaks out in front of its last attention, so it takes no head or neuron option that acts in layer L - 1.  Then the depth
// lens: every lens row must be a consumed row [score rows | logit rows] - the last layer finishes only those; lens_at: its place among them
static int pass_options_check(aigv_ctx* c, int T, int keep_kv, const int32_t* score_rows, int nS, const int32_t* logit_rows, int R, int32_t* lens_at) {
  const aigv_config& k = c->cfg;
  const int last = k.llm_layers - 1;
  const bool cut = nS + R == 0 && c->trim_last_layer;   // the pass breaks out in front of its last attention
  for (const char* family : {"stream", "head", "neuron"}) {
    const aigv_ctx::RowOptEntry* first = first_armed(c, family);
    if (!first) continue;
    if (keep_kv) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: keep_kv while a %s %s is armed (%s): only a pass without a KV cache takes one", family, first->what, first->arm);
    if (!strcmp(family, "head") && (k.llm_heads > AIGV_MAX_HEAD_BITS || (c->head_dim != 64 && c->head_dim != 128)))
      return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: a head %s is armed (%s) on a model of %d heads x %d: at most %d heads of 64 or 128", first->what, first->arm, k.llm_heads, c->head_dim, AIGV_MAX_HEAD_BITS);
    bool reaches = false;
    for (const aigv_ctx::RowOptEntry& e : c->row_opts) {
      const aigv_ctx::RowOpt& r = *e.opt;
      if (!r.armed || strcmp(e.family, family)) continue;
      char label[96];
      snprintf(label, sizeof label, "aigv_llm_prefill: the %s %s (%s)", e.family, e.what, e.arm);
      if (!r.all_rows) TRY(stream_rows_check(c, label, r.rows.data(), (int)r.rows.size(), T, r.lo, r.hi, k.llm_layers));
      reaches |= cut && e.skipped && acts_in_layer(c, &r, last);
    }
    if (reaches)
      return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: a %s option reaches layer %d and the pass has no output rows (n_out == 0): the last layer's %s does not run", family, last, first->skipped);
  }
  if (!c->lens.armed) return 0;
  if (nS + R == 0) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: the depth lens is armed and the pass has no output rows (n_out == 0): nothing finishes the last layer");
  if (c->lens.n_score > 0 && nS == 0) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: the depth lens is armed with %d score rows and the pass has score == NULL (no score head runs)", c->lens.n_score);
  for (int i = 0; i < c->lens.n_score + c->lens.n_token; ++i) {
    int at = -1;
    for (int j = 0; j < nS && at < 0; ++j) if (score_rows[j] == c->lens.rows[i]) at = j;
    for (int j = 0; j < R && at < 0; ++j) if (logit_rows[j] == c->lens.rows[i]) at = nS + j;
    if (at < 0) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: depth-lens row %d (packed row %d) is not among the pass's consumed rows (its score rows and logit rows): the last layer finishes only those", i, c->lens.rows[i]);
    lens_at[i] = at;
  }
  return 0;
}

int aigv_llm_prefill(aigv_ctx* c, const int64_t* ids, const int32_t* slot, const int32_t* cu, int B, const void* vis,
                     int n_vis, const void* motion, const int32_t* score_rows, float* score, const int32_t* logit_rows,
                     int R, int64_t* argmax, int keep_kv, void* stream) {
  if (!c || !ids || !slot || !cu) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: null argument");
  // What the pass finds the context armed with stays in the records until the scope below ends, which disarms all of it on every way out.  probe
  // (aigv_score_attention_arm): this pass carries the probe; drop (aigv_key_drop_arm / _ex): the attention of the armed layers runs under the mask; lens
  // (aigv_depth_lens_arm): the lens rows are tapped after the embedding and after every layer; the row options (aigv_ctx::row_opts): stream rows overwritten /
  // copied out in front of the armed layers, l_ao between the attention and wo, the row w2 consumes
  DisarmScope disarm(c);
  if (!c->finalized) return fail(c, AIGV_ERR_STATE, "aigv_llm_prefill: call aigv_finalize_weights first");
  if (c->drop.armed && c->probe.armed) return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: a key-drop mask and the score-attention probe are both armed: the probe does not know the mask");
  const aigv_config& k = c->cfg;
  if (c->drop.armed && (c->drop.layer_begin < 0 || c->drop.layer_begin > c->drop.layer_end || c->drop.layer_end > k.llm_layers))
    return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: key-drop mask armed for layers [%d, %d), outside 0 <= begin <= end <= %d", c->drop.layer_begin, c->drop.layer_end, k.llm_layers);
  if (c->drop.armed && keep_kv && (c->drop.rows || c->drop.layer_begin != 0 || c->drop.layer_end != k.llm_layers))
    return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: keep_kv under a key-drop mask with row words or a partial layer window (aigv_key_drop_arm_ex): the mask kept "
                                 "beside the KV cache has neither");
  if (B <= 0 || B > k.max_seqs) return fail(c, AIGV_ERR_ARG, "n_clips %d outside 1..%d", B, k.max_seqs);
  if (cu[0] != 0) return fail(c, AIGV_ERR_ARG, "cu_seqlens[0] must be 0");
  int max_len = 0;
  for (int b = 0; b < B; ++b) {
    const int len = cu[b + 1] - cu[b];
    if (len <= 0) return fail(c, AIGV_ERR_ARG, "clip %d has an empty token sequence", b);
    if (len > k.max_positions) return fail(c, AIGV_ERR_ARG, "clip %d: %d tokens exceed the RoPE table (%d)", b, len, k.max_positions);
    max_len = std::max(max_len, len);
  }
  const int T = cu[B];
  if (T > k.max_tokens) return fail(c, AIGV_ERR_ARG, "%d packed tokens exceed max_tokens %d", T, k.max_tokens);
  if ((score && !score_rows) || (R > 0 && (!logit_rows || !argmax))) return fail(c, AIGV_ERR_ARG, "output rows/buffers inconsistent");
  if (n_vis < 0 || (n_vis > 0 && !vis)) return fail(c, AIGV_ERR_ARG, "visual tokens missing");
  if (keep_kv && (k.kv_capacity <= 0 || max_len >= k.kv_capacity))
    return fail(c, AIGV_ERR_STATE, "keep_kv needs kv_capacity > longest prompt (%d vs %d)", k.kv_capacity, max_len);
  if (c->drop.armed && (!c->drop.words || c->drop.ld < (max_len + 63) / 64))
    return fail(c, AIGV_ERR_ARG, "aigv_llm_prefill: key-drop mask armed with %d words per clip, the longest clip (%d tokens) needs %d", c->drop.ld, max_len,
                (max_len + 63) / 64);
  const int n_lens = c->lens.armed ? c->lens.n_score + c->lens.n_token : 0;
  int32_t lens_at[2 * AIGV_MAX_LENS_ROWS];   // the lens rows' places among the consumed rows
  TRY(pass_options_check(c, T, keep_kv, score_rows, score ? B : 0, logit_rows, R, lens_at));
  AttnMapArgs amap{};
  if (c->amap.armed) TRY(map_plan(c, cu, B, keep_kv, &amap));   // (refusals: in front of the pass's first launch)
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const int H = k.llm_hidden, I = k.llm_inter, D = c->head_dim, g = c->g, nkv = k.llm_kv_heads;

  if (B + 1 > AIGV_SMALL_INTS / 2) return fail(c, AIGV_ERR_ARG, "at most %d clips per prefill call", AIGV_SMALL_INTS / 2 - 1);
  // positions / sequence ids / cu_seqlens are produced on the device from cu passed as a kernel argument
  HIPCHK(c, aigv_launch_seqpos(cu, B, c->l_pos, c->l_seq, c->l_cu, T, s));
  // every clip is a sequence: the kernel form of a row follows from its place in its own clip (struct RowPlan)
  TRY(build_row_plan(c, c->rp_llm, cu, B, s));
  RowPlanScope rps(c, &c->rp_llm);   // (fp8 mode: its bf16 GEMMs - the post-attention half of the last layer - follow the per-clip plan too)

  HIPCHK(c, aigv_launch_embed(ids, slot, c->tok_emb, (const bf16_t*)vis, (const bf16_t*)motion, n_vis, c->l_h, T, H, s));
  TRY(upload_out_rows(c, score_rows, score != nullptr, B, logit_rows, R, T, s));
  // depth d of the lens: rows idx[0 .. n_lens) of src -> slice d of the caller's two buffers, one launch
  const int32_t* lens_idx = c->l_lensidx;
  auto lens_tap = [&](int depth, const bf16_t* src, const int32_t* idx) -> int {
    const size_t off = (size_t)depth * n_lens * H;
    HIPCHK(c, aigv_launch_lens_tap(src, H, idx, n_lens, c->final_norm, c->lens.hidden + off, c->lens.normed + off, H, k.rms_eps, s));
    return 0;
  };
  // the row tables of the armed stream and head options go up on this stream, a max_tokens slot each in the order a layer applies them (the neuron options': neuron_plan)
  const aigv_ctx::RowOpt *st[2] = {&c->stream_patch, &c->stream_cap}, *hd[3] = {&c->head_scale, &c->head_patch, &c->head_cap};
  for (int o = 0; o < 2; ++o)
    if (st[o]->armed) HIPCHK(c, aigv_launch_write_ints(st[o]->rows.data(), (int)st[o]->rows.size(), c->l_streamidx + (size_t)o * k.max_tokens, s));
  for (int o = 0; o < 3; ++o)
    if (hd[o]->armed && !hd[o]->all_rows) HIPCHK(c, aigv_launch_write_ints(hd[o]->rows.data(), (int)hd[o]->rows.size(), c->l_headidx + (size_t)o * k.max_tokens, s));
  if (c->lens.armed) {
    HIPCHK(c, aigv_launch_write_ints(c->lens.rows, n_lens, c->l_lensidx, s));
    HIPCHK(c, aigv_launch_write_ints(lens_at, n_lens, c->l_lensidx + 2 * AIGV_MAX_LENS_ROWS, s));
  }
  // Row trimming: after the last layer's attention every row is independent, and only the consumed rows (one score row per
  // clip + the answer rows) are read afterwards (stage2_eval.py:940-941; modeling_internvl_chat.py:469-481).  When they are
  // few, the last layer finishes just those rows: attention for the query blocks that contain them, then wo / MLP on a
  // compact copy through the weight-streaming skinny kernel.  K/V of the last layer still cover every row (keep_kv).
  const int n_out = (int)c->h_rowidx.size();
  int q_tail = 0;   // the farthest a consumed row lies from the end of its clip
  // The rule is PER CLIP, so that a clip's consumed rows take the same kernels whatever its batch mates are: the consumed rows of a clip
  // with at most TRIM_ROWS of them finish on the weight-streaming kernel (its fixed form), those of a clip with more on the tile kernels
  // with all the other rows.  All clips small (the eval scripts' case): `trim` - the last layer runs for the consumed rows only.  Mixed
  // batch: the last layer runs for every row AND the small clips' consumed rows are finished on the streaming path and put back in place.
  constexpr int TRIM_ROWS = 16;
  std::vector<int32_t> small_rows;
  {
    std::vector<int> per_clip(B, 0), clip_of(c->h_rowidx.size());
    for (size_t i = 0; i < c->h_rowidx.size(); ++i) {
      int b = 0;
      while (cu[b + 1] <= c->h_rowidx[i]) ++b;
      clip_of[i] = b;
      ++per_clip[b];
      q_tail = std::max(q_tail, cu[b + 1] - c->h_rowidx[i]);
    }
    for (size_t i = 0; i < c->h_rowidx.size(); ++i)
      if (per_clip[clip_of[i]] <= TRIM_ROWS) small_rows.push_back(c->h_rowidx[i]);
  }
  const bool trim_ok = c->trim_last_layer && n_out > 0 && H % 128 == 0 && I % 128 == 0;
  const bool trim = trim_ok && (int)small_rows.size() == n_out;
  const bool mixed = trim_ok && !trim && !small_rows.empty();
  if (mixed) HIPCHK(c, aigv_launch_write_ints(small_rows.data(), (int)small_rows.size(), c->l_rowidx2, s));
  NeuronPlan nplan;
  const NeuronPlan* np = first_armed(c, "neuron") ? &nplan : nullptr;
  if (np) TRY(neuron_plan(c, small_rows, trim, mixed, s, &nplan));
  ProbeArgs probe{};
  if (c->probe.armed) TRY(probe_plan(c, "aigv_llm_prefill", cu, B, nullptr, &probe));
  double attn_flops = 0;
  for (int b = 0; b < B; ++b) { const double L = cu[b + 1] - cu[b]; attn_flops += 4.0 * (L * (L + 1) / 2) * D * k.llm_heads; }
  const size_t kv_layer = (size_t)k.max_seqs * nkv * k.kv_capacity * D;
  for (int li = 0; li < k.llm_layers; ++li) {
    const LlmLayer& L = c->llm[li];
    TRY(stream_hook(c, li, s));
    if (c->lens.armed) TRY(lens_tap(li, c->l_h, lens_idx));   // depth li < L: the stream this layer consumes, behind a patch of this depth
    TRY(llm_layer_qkv(c, li, T, s));
    if (keep_kv)
      HIPCHK(c, aigv_launch_kv_store(c->l_qkv, c->qkv_out, c->l_seq, c->l_pos, c->kc + li * kv_layer, c->vc + li * kv_layer, T,
                                     nkv, g, D, k.kv_capacity, s));
    if (c->probe.armed) TRY(probe_layer(c, probe, li, false, s));   // Q and rotated K of this pass's rows, straight from l_qkv (every layer: it does not read l_ao)
    if (c->amap.armed) TRY(map_layer(c, amap, li, s));              // every row of every head, from the same columns (the row-trimmed last layer included: Q and K exist for all T rows)
    // a pass that only fills the cache (no output rows) needs nothing of the last layer beyond its K/V
    if (n_out == 0 && c->trim_last_layer && li == k.llm_layers - 1) break;
    {
      AttnArgs a = llm_attn_args(c, B);   // K / V: this pass's rows of l_qkv
      a.k = c->l_qkv + (size_t)g * D; a.v = c->l_qkv + (size_t)(g + 1) * D;
      a.ldk = a.ldv = c->qkv_out; a.kv_head_stride = (g + 2) * D;
      a.max_len = max_len;
      const bool last_trim = trim && li == k.llm_layers - 1;
      // (a head capture of the last layer reads rows the trimmed launch would skip: that one launch covers every row - in the causal kernel q_tail
      // only skips blocks and waves, so the consumed rows keep their bits)
      const aigv_ctx::HeadRows& hc = c->head_cap;
      a.q_tail = last_trim && !(hc.armed && li >= hc.lo && li < hc.hi && !hc.rows.empty()) ? q_tail : 0;
      // the armed layers, the row-trimmed last one included; the others run the unmasked launch they always ran
      if (c->drop.armed && li >= c->drop.layer_begin && li < c->drop.layer_end) { a.key_drop = c->drop.words; a.ld_drop = c->drop.ld; a.drop_rows = c->drop.rows; }
      if (const char* m = aigv_attn_check(a, D)) return fail(c, AIGV_ERR_ARG, "%s", m);
      ProfScope ps(c, AIGV_PROF_ATTN_LLM, last_trim ? 0.0 : attn_flops, 2.0 * T * ((double)c->qkv_out + H), s);
      HIPCHK(c, aigv_launch_attention(a, D, s));
    }
    TRY(head_hook(c, li, T, s));
    if ((trim || mixed) && li == k.llm_layers - 1) {
      // 64 rows at a time through the weight-streaming kernel in its fixed 4-slice form (p = 0: the same bits whatever the row count);
      // the finished rows collect in l_trim_h, in l_rowidx (mixed: l_rowidx2) order
      const int32_t* idx = trim ? c->l_rowidx : c->l_rowidx2;
      const int n_fin = trim ? n_out : (int)small_rows.size();
      bf16_t *t_ao = c->l_trim, *t_n = t_ao + (size_t)64 * H, *t_ffn = t_n + (size_t)64 * H, *t_h = c->l_trim_h;
      for (int r0 = 0; r0 < n_fin; r0 += 64) {
        const int nr = std::min(64, n_fin - r0);
        bf16_t* h = t_h + (size_t)r0 * H;
        HIPCHK(c, aigv_launch_gather_rows(c->l_ao, H, idx + r0, nr, t_ao, H, s));
        HIPCHK(c, aigv_launch_gather_rows(c->l_h, H, idx + r0, nr, h, H, s));
        TRY(run_skinny(c, t_ao, H, nr, L.wo, H, H, H, nullptr, h, H, h, H, SK_RESID, s, 0));
        HIPCHK(c, aigv_launch_rmsnorm(h, H, L.fn, t_n, H, nr, H, k.rms_eps, nullptr, s));
        TRY(run_skinny(c, t_n, H, nr, L.w13, H, 2 * I, H, nullptr, nullptr, 0, t_ffn, I, SK_SWIGLU, s, 0));
        if (np) TRY(neuron_hook(c, *np, li, t_ffn, r0 / 64, nr, s));
        TRY(run_skinny(c, t_ffn, I, nr, L.w2, I, H, I, nullptr, h, H, h, H, SK_RESID, s, 0));
      }
      if (trim) {
        if (c->lens.armed) TRY(lens_tap(k.llm_layers, t_h, lens_idx + 2 * AIGV_MAX_LENS_ROWS));          // depth L: the finished rows, in l_rowidx order
        TRY(final_rows(c, score, B, R, argmax, t_h, true, s));
        break;
      }
      TRY(llm_layer_post(c, li, T, s, np, NEURON_AT_REST));                                      // every row on the tile kernels ...
      HIPCHK(c, aigv_launch_scatter_rows(t_h, c->l_rowidx2, n_fin, c->l_h, H, H, s));            // ... the small clips' consumed rows put back
      if (c->lens.armed) TRY(lens_tap(k.llm_layers, c->l_h, lens_idx));
      break;
    }
    TRY(llm_layer_post(c, li, T, s, np));
    if (c->lens.armed && li == k.llm_layers - 1) TRY(lens_tap(k.llm_layers, c->l_h, lens_idx));   // depth L of a pass whose last layer ran for every row
  }
  if (!trim) TRY(final_rows(c, score, B, R, argmax, c->l_h, false, s));
  if (c->lens.armed && c->lens.n_score > 0) {
    // the score head on the score rows of every depth: each depth a batch slice with a NaN guard of its own, as many depths per call as the
    // head's workspace (64 rows) holds
    const int nS = c->lens.n_score, per = std::max(1, 64 / nS);
    for (int d0 = 0; d0 <= k.llm_layers; d0 += per) {
      ScoreHeadArgs a = c->score;
      a.x = c->lens.normed + (size_t)d0 * n_lens * H; a.ldx = H; a.B = nS; a.score = c->lens.score + (size_t)d0 * nS;
      HIPCHK(c, aigv_launch_score_head_groups(a, std::min(per, k.llm_layers + 1 - d0), (size_t)n_lens * H, c->l_score_ws, s));
    }
  }
  if (keep_kv) {
    c->h_kvlen.resize(B);
    for (int b = 0; b < B; ++b) c->h_kvlen[b] = cu[b + 1] - cu[b];
    TRY(upload_decode_state(c, B, s));
    // a masked pass keeps its mask with the cache: every clip's words cut to its length, zero from there to the row's end (on the pass's stream, into
    // the context's own buffer: nothing is allocated, the pass still captures); aigv_llm_extend and the decode steps then run under it
    if (c->drop.armed) HIPCHK(c, aigv_launch_kv_drop_rows(c->drop.words, c->drop.ld, nullptr, c->l_cu, 1, c->kv_drop, c->kv_drop_ld, B, s));
    c->kv_masked = c->drop.armed;
    c->kv_valid = true;
  } else {
    c->kv_valid = false;
    c->kv_masked = false;
  }
  return 0;
}

// Arms the next aigv_llm_prefill with a key-drop mask (include/aigv_amd.h): the words are read when that pass runs (keep_kv: and copied into the cache's mask).
static int key_drop_arm(const char* op, aigv_ctx* c, const uint64_t* words_dev, const uint64_t* row_words_dev, int ld_words, int layer_begin, int layer_end) {
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (!words_dev || ((uintptr_t)words_dev & 7)) return fail(c, AIGV_ERR_ARG, "%s: words_dev is null or not 8-byte aligned", op);
  if ((uintptr_t)row_words_dev & 7) return fail(c, AIGV_ERR_ARG, "%s: row_words_dev is not 8-byte aligned", op);
  if (ld_words < 1) return fail(c, AIGV_ERR_ARG, "%s: ld_words = %d must be positive", op, ld_words);
  if (layer_begin < 0 || layer_begin > layer_end || layer_end > c->cfg.llm_layers)
    return fail(c, AIGV_ERR_ARG, "%s: layers [%d, %d) outside 0 <= begin <= end <= %d", op, layer_begin, layer_end, c->cfg.llm_layers);
  c->drop.words = words_dev; c->drop.rows = row_words_dev; c->drop.ld = ld_words;
  c->drop.layer_begin = layer_begin; c->drop.layer_end = layer_end;
  c->drop.armed = true;
  return 0;
}

int aigv_key_drop_arm(aigv_ctx* c, const uint64_t* words_dev, int ld_words) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_key_drop_arm: null context");
  return key_drop_arm("aigv_key_drop_arm", c, words_dev, nullptr, ld_words, 0, c->cfg.llm_layers);
}

// ... for the query rows row_words_dev selects (null: every row) in the layers [layer_begin, layer_end) only (include/aigv_amd.h)
int aigv_key_drop_arm_ex(aigv_ctx* c, const uint64_t* words_dev, const uint64_t* row_words_dev, int ld_words, int layer_begin, int layer_end) {
  return key_drop_arm("aigv_key_drop_arm_ex", c, words_dev, row_words_dev, ld_words, layer_begin, layer_end);
}

// Arms the next aigv_llm_prefill with the depth lens (include/aigv_amd.h): the row lists are copied here, the buffers are written when that pass runs.
int aigv_depth_lens_arm(aigv_ctx* c, const int32_t* score_rows_host, int n_score, const int32_t* token_rows_host, int n_token, void* hidden_out_bf16,
                        void* normed_out_bf16, float* score_out) {
  const char* op = "aigv_depth_lens_arm";
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (n_score < 0 || n_score > AIGV_MAX_LENS_ROWS || n_token < 0 || n_token > AIGV_MAX_LENS_ROWS)
    return fail(c, AIGV_ERR_ARG, "%s: %d score rows and %d token rows: each list holds 0..%d rows", op, n_score, n_token, AIGV_MAX_LENS_ROWS);
  if (n_score + n_token == 0) return fail(c, AIGV_ERR_ARG, "%s: no row to read (n_score = n_token = 0)", op);
  if ((n_score > 0 && !score_rows_host) || (n_token > 0 && !token_rows_host)) return fail(c, AIGV_ERR_ARG, "%s: null row list", op);
  if (!hidden_out_bf16 || ((uintptr_t)hidden_out_bf16 & 15)) return fail(c, AIGV_ERR_ARG, "%s: hidden_out_bf16 is null or not 16-byte aligned", op);
  if (!normed_out_bf16 || ((uintptr_t)normed_out_bf16 & 15)) return fail(c, AIGV_ERR_ARG, "%s: normed_out_bf16 is null or not 16-byte aligned", op);
  if (n_score > 0 && (!score_out || ((uintptr_t)score_out & 3))) return fail(c, AIGV_ERR_ARG, "%s: score_out is null or not 4-byte aligned", op);
  for (int i = 0; i < n_score; ++i) c->lens.rows[i] = score_rows_host[i];
  for (int i = 0; i < n_token; ++i) c->lens.rows[n_score + i] = token_rows_host[i];
  c->lens.n_score = n_score; c->lens.n_token = n_token;
  c->lens.hidden = (bf16_t*)hidden_out_bf16; c->lens.normed = (bf16_t*)normed_out_bf16; c->lens.score = score_out;
  c->lens.armed = true;
  return 0;
}

// Arm the next aigv_llm_prefill with a row option (include/aigv_amd.h; aigv_ctx::row_opts): what the arming entry points share.  The row numbers are copied
// here and checked, with the window, when that pass runs; the device buffer is the caller's.  rows_optional (a scale): no row list means every row;
// need_buf: the option moves data through `buf`; family_check (null: none), handed cols_host and m: the family's own checks, run where they have always run -
// behind the row list's, in front of the buffer's
typedef int (*FamilyCheck)(const char* op, aigv_ctx* c, const int32_t* cols_host, int m);
static int rows_arm(const char* op, aigv_ctx* c, aigv_ctx::RowOpt* st, const int32_t* rows_host, int n, int lo, int hi, void* buf_bf16_dev, bool rows_optional, bool need_buf,
                    FamilyCheck family_check = nullptr, const int32_t* cols_host = nullptr, int m = 0) {
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (n < 0 || n > c->cfg.max_tokens) return fail(c, AIGV_ERR_ARG, "%s: %d rows outside 0..max_tokens = %d", op, n, c->cfg.max_tokens);
  if (n > 0 && !rows_host && !rows_optional) return fail(c, AIGV_ERR_ARG, "%s: null row list", op);
  if (family_check) TRY(family_check(op, c, cols_host, m));
  if (need_buf && n > 0 && hi > lo && (!buf_bf16_dev || ((uintptr_t)buf_bf16_dev & 15))) return fail(c, AIGV_ERR_ARG, "%s: the device buffer is null or not 16-byte aligned", op);
  st->all_rows = rows_optional && !rows_host;
  if (rows_host) st->rows.assign(rows_host, rows_host + n); else st->rows.clear();
  st->lo = lo; st->hi = hi;
  st->buf = (bf16_t*)buf_bf16_dev;
  st->armed = true;
  return 0;
}

// ---- residual-stream rows
int aigv_stream_capture_arm(aigv_ctx* c, const int32_t* rows_host, int n, int lo, int hi, void* out_bf16_dev) {
  return rows_arm("aigv_stream_capture_arm", c, c ? &c->stream_cap : nullptr, rows_host, n, lo, hi, out_bf16_dev, false, true);
}

int aigv_stream_patch_arm(aigv_ctx* c, const int32_t* rows_host, int n, int lo, int hi, const void* values_bf16_dev) {
  return rows_arm("aigv_stream_patch_arm", c, c ? &c->stream_patch : nullptr, rows_host, n, lo, hi, const_cast<void*>(values_bf16_dev), false, true);
}

// ---- per-head attention outputs: the host arrays are copied here
static int head_count_check(const char* op, aigv_ctx* c, const int32_t*, int) {
  if (c->cfg.llm_heads > AIGV_MAX_HEAD_BITS) return fail(c, AIGV_ERR_ARG, "%s: the model has %d query heads: a head mask holds at most %d", op, c->cfg.llm_heads, AIGV_MAX_HEAD_BITS);
  return 0;
}

int aigv_head_capture_arm(aigv_ctx* c, const int32_t* rows_host, int n, int lo, int hi, void* out_bf16_dev) {
  return rows_arm("aigv_head_capture_arm", c, c ? &c->head_cap : nullptr, rows_host, n, lo, hi, out_bf16_dev, false, true, head_count_check);
}

int aigv_head_patch_arm(aigv_ctx* c, const int32_t* rows_host, int n, int lo, int hi, const uint64_t* head_bits_host, const void* values_bf16_dev) {
  TRY(rows_arm("aigv_head_patch_arm", c, c ? &c->head_patch : nullptr, rows_host, n, lo, hi, const_cast<void*>(values_bf16_dev), false, true, head_count_check));
  const int w = hi > lo ? hi - lo : 0;
  if (head_bits_host) c->head_patch.bits.assign(head_bits_host, head_bits_host + w); else c->head_patch.bits.assign(w, ~(uint64_t)0);
  return 0;
}

int aigv_head_scale_arm(aigv_ctx* c, const int32_t* rows_host, int n, const float* scale_host) {
  const char* op = "aigv_head_scale_arm";
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  if (!scale_host) return fail(c, AIGV_ERR_ARG, "%s: null scale table", op);
  const size_t cells = (size_t)c->cfg.llm_layers * c->cfg.llm_heads;
  for (size_t i = 0; i < cells; ++i)
    if (scale_host[i] != scale_host[i])
      return fail(c, AIGV_ERR_ARG, "%s: scale[%d][%d] is NaN", op, (int)(i / c->cfg.llm_heads), (int)(i % c->cfg.llm_heads));
  TRY(rows_arm(op, c, &c->head_scale, rows_host, rows_host ? n : 0, 0, c->cfg.llm_layers, nullptr, true, false, head_count_check));
  c->head_scale.scale.assign(scale_host, scale_host + cells);
  return 0;
}

// ---- MLP neurons: the host arrays are copied here.  The family's checks: the model's I, then the column list (null: every neuron)
static int neuron_cols_check(const char* op, aigv_ctx* c, const int32_t* cols, int m) {
  const int I = c->cfg.llm_inter;
  if (I % 8) return fail(c, AIGV_ERR_ARG, "%s: the model's intermediate size %d is no multiple of 8", op, I);
  if (!cols) return 0;
  if (m < 0 || m > AIGV_MAX_NEURON_SEL) return fail(c, AIGV_ERR_ARG, "%s: %d columns outside 0..%d", op, m, AIGV_MAX_NEURON_SEL);
  for (int j = 0; j < m; ++j) {
    if (cols[j] < 0 || cols[j] >= I) return fail(c, AIGV_ERR_ARG, "%s: column %d (entry %d) outside 0..%d", op, cols[j], j, I - 1);
    if (j && cols[j] <= cols[j - 1]) return fail(c, AIGV_ERR_ARG, "%s: columns not strictly ascending at entry %d (%d after %d)", op, j, cols[j], cols[j - 1]);
  }
  return 0;
}

// a capture / a patch of the columns cols_host (null: every neuron); an empty list moves nothing and needs no buffer
static int neuron_window_arm(const char* op, aigv_ctx* c, aigv_ctx::NeuronRows* st, const int32_t* rows_host, int n, int lo, int hi, const int32_t* cols_host, int m, void* buf_bf16_dev) {
  TRY(rows_arm(op, c, st, rows_host, n, lo, hi, buf_bf16_dev, false, !cols_host || m > 0, neuron_cols_check, cols_host, m));
  st->dense = !cols_host;
  if (cols_host) st->cols.assign(cols_host, cols_host + m); else st->cols.clear();
  return 0;
}

int aigv_neuron_capture_arm(aigv_ctx* c, const int32_t* rows_host, int n, int lo, int hi, const int32_t* cols_host, int m, void* out_bf16_dev) {
  return neuron_window_arm("aigv_neuron_capture_arm", c, c ? &c->neuron_cap : nullptr, rows_host, n, lo, hi, cols_host, m, out_bf16_dev);
}

int aigv_neuron_patch_arm(aigv_ctx* c, const int32_t* rows_host, int n, int lo, int hi, const int32_t* cols_host, int m, const void* values_bf16_dev) {
  return neuron_window_arm("aigv_neuron_patch_arm", c, c ? &c->neuron_patch : nullptr, rows_host, n, lo, hi, cols_host, m, const_cast<void*>(values_bf16_dev));
}

int aigv_neuron_scale_arm(aigv_ctx* c, const int32_t* rows_host, int n, const float* layer_scale_host, const int32_t* sel_layers_host, const int32_t* sel_cols_host,
                          const float* sel_factors_host, int m) {
  const char* op = "aigv_neuron_scale_arm";
  if (!c) return fail(c, AIGV_ERR_ARG, "%s: null context", op);
  const int L = c->cfg.llm_layers, I = c->cfg.llm_inter;
  if (rows_host && (n < 0 || n > c->cfg.max_tokens)) return fail(c, AIGV_ERR_ARG, "%s: %d rows outside 0..max_tokens = %d", op, n, c->cfg.max_tokens);
  if (I % 8) return fail(c, AIGV_ERR_ARG, "%s: the model's intermediate size %d is no multiple of 8", op, I);
  if (m < 0 || m > AIGV_MAX_NEURON_SEL) return fail(c, AIGV_ERR_ARG, "%s: %d selected neurons outside 0..%d", op, m, AIGV_MAX_NEURON_SEL);
  if (m > 0 && (!sel_layers_host || !sel_cols_host || !sel_factors_host)) return fail(c, AIGV_ERR_ARG, "%s: null selection list", op);
  if (!layer_scale_host && m == 0 && !sel_layers_host) return fail(c, AIGV_ERR_ARG, "%s: neither a per-layer table nor a selection", op);
  if (layer_scale_host)
    for (int l = 0; l < L; ++l) if (layer_scale_host[l] != layer_scale_host[l]) return fail(c, AIGV_ERR_ARG, "%s: layer_scale[%d] is NaN", op, l);
  std::vector<int32_t> begin(L + 1, 0);
  for (int j = 0; j < m; ++j) {
    const int l = sel_layers_host[j], col = sel_cols_host[j];
    if (l < 0 || l >= L) return fail(c, AIGV_ERR_ARG, "%s: layer %d (entry %d) outside 0..%d", op, l, j, L - 1);
    if (col < 0 || col >= I) return fail(c, AIGV_ERR_ARG, "%s: column %d (entry %d) outside 0..%d", op, col, j, I - 1);
    if (j && (l < sel_layers_host[j - 1] || (l == sel_layers_host[j - 1] && col <= sel_cols_host[j - 1])))
      return fail(c, AIGV_ERR_ARG, "%s: the selection is not strictly ascending in (layer, column) at entry %d", op, j);
    if (sel_factors_host[j] != sel_factors_host[j]) return fail(c, AIGV_ERR_ARG, "%s: factor %d is NaN", op, j);
    ++begin[l + 1];
  }
  for (int l = 0; l < L; ++l) begin[l + 1] += begin[l];
  // (its checks done, the shared helper has nothing left to refuse: it fills the base record)
  TRY(rows_arm(op, c, &c->neuron_scale, rows_host, rows_host ? n : 0, 0, L, nullptr, true, false));
  aigv_ctx::NeuronRows& st = c->neuron_scale;
  if (layer_scale_host) st.layer_scale.assign(layer_scale_host, layer_scale_host + L); else st.layer_scale.clear();
  st.dense = m == 0;
  if (m > 0) { st.cols.assign(sel_cols_host, sel_cols_host + m); st.factors.assign(sel_factors_host, sel_factors_host + m); st.sel_begin = begin; }
  else { st.cols.clear(); st.factors.clear(); st.sel_begin.clear(); }
  return 0;
}

// Continue the sequences kept by aigv_llm_prefill(keep_kv = 1) with new TEXT tokens: causal attention of the new rows over the
// cached keys plus themselves.  commit = 0 leaves the cache lengths where they were, so several continuations of ONE prefix
// (the four quality-perspective questions behind the same video tokens) can be scored one after the other.
int aigv_llm_extend(aigv_ctx* c, const int64_t* ids, const int32_t* cu, int B, const int32_t* score_rows, float* score,
                    const int32_t* logit_rows, int R, int64_t* argmax, int commit, void* stream) {
  if (!c || !ids || !cu) return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: null argument");
  DisarmScope disarm(c);   // (what the context is armed with stays in the records until the scope ends)
  for (const char* family : {"neuron", "head", "stream"})
    if (const aigv_ctx::RowOptEntry* e = first_armed(c, family))
      return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: a %s %s is armed (%s): the continuation pass takes none, only aigv_llm_prefill does", family, e->what, e->arm);
  if (c->lens.armed) return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: the depth lens is armed (aigv_depth_lens_arm): the continuation pass takes no lens, only aigv_llm_prefill does");
  if (c->amap.armed) return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: the attention map is armed (aigv_attention_map_arm): the continuation pass takes no map (it has no cache form), only aigv_llm_prefill does");
  if (c->drop.armed) return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: a key-drop mask is armed (aigv_key_drop_arm): the continuation pass takes no mask, only aigv_llm_prefill does");
  if (!c->kv_valid) return fail(c, AIGV_ERR_STATE, "aigv_llm_extend: no KV state (run aigv_llm_prefill with keep_kv)");
  if (c->probe.armed && c->kv_masked) return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: the score-attention probe is armed and the KV cache carries a key-drop mask: the probe does not know the mask");
  const aigv_config& k = c->cfg;
  if (B != c->kv_seqs) return fail(c, AIGV_ERR_ARG, "aigv_llm_extend: %d sequences, the cache holds %d", B, c->kv_seqs);
  if (B + 1 > AIGV_SMALL_INTS / 2) return fail(c, AIGV_ERR_ARG, "at most %d clips per call", AIGV_SMALL_INTS / 2 - 1);
  if (cu[0] != 0) return fail(c, AIGV_ERR_ARG, "cu_seqlens[0] must be 0");
  int max_new = 0, max_cached = 0;
  for (int b = 0; b < B; ++b) {
    const int n = cu[b + 1] - cu[b];
    max_cached = std::max(max_cached, (int)c->h_kvlen[b]);
    if (n <= 0) return fail(c, AIGV_ERR_ARG, "clip %d: no new tokens", b);
    if (c->h_kvlen[b] + n > k.kv_capacity || c->h_kvlen[b] + n > k.max_positions)
      return fail(c, AIGV_ERR_STATE, "clip %d: KV cache / RoPE table exhausted (%d cached + %d new, capacity %d)", b, c->h_kvlen[b], n, k.kv_capacity);
    max_new = std::max(max_new, n);
  }
  const int T = cu[B];
  if (T > k.max_tokens) return fail(c, AIGV_ERR_ARG, "%d new tokens exceed max_tokens %d", T, k.max_tokens);
  if ((score && !score_rows) || (R > 0 && (!logit_rows || !argmax))) return fail(c, AIGV_ERR_ARG, "output rows/buffers inconsistent");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const int H = k.llm_hidden, D = c->head_dim, g = c->g, nkv = k.llm_kv_heads;
  // positions continue after the cached tokens; the cached lengths are the per-sequence key offsets of the attention
  HIPCHK(c, aigv_launch_seqpos(cu, B, c->l_pos, c->l_seq, c->l_cu, T, s, c->h_kvlen.data()));
  HIPCHK(c, aigv_launch_write_ints(c->h_kvlen.data(), B, c->l_kvlen, s));
  HIPCHK(c, aigv_launch_embed(ids, c->l_neg1, c->tok_emb, nullptr, nullptr, 0, c->l_h, T, H, s));
  TRY(upload_out_rows(c, score_rows, score != nullptr, B, logit_rows, R, T, s));
  ProbeArgs probe{};
  if (c->probe.armed) TRY(probe_plan(c, "aigv_llm_extend", cu, B, c->h_kvlen.data(), &probe));
  double attn_flops = 0;
  for (int b = 0; b < B; ++b) { const double n = cu[b + 1] - cu[b]; attn_flops += 4.0 * n * (c->h_kvlen[b] + (n + 1) / 2) * D * k.llm_heads; }
  const size_t kv_layer = (size_t)k.max_seqs * nkv * k.kv_capacity * D;
  for (int li = 0; li < k.llm_layers; ++li) {
    // (fp8 mode: the linears aigv_llm_prefill runs in e4m3 run in e4m3 here too, so a continuation scores like the same tokens inside
    // one prefill of that mode)
    TRY(llm_layer_qkv(c, li, T, s));
    HIPCHK(c, aigv_launch_kv_store(c->l_qkv, c->qkv_out, c->l_seq, c->l_pos, c->kc + li * kv_layer, c->vc + li * kv_layer, T, nkv, g, D,
                                   k.kv_capacity, s));
    if (c->probe.armed) TRY(probe_layer(c, probe, li, true, s));   // K from the cache: the cached keys and, behind them, the rows just appended
    {
      AttnArgs a = llm_attn_args(c, B);   // K / V: the cache, the new rows behind each sequence's cached keys
      a.k = c->kc + li * kv_layer; a.v = c->vc + li * kv_layer;
      a.ldk = a.ldv = D; a.kv_head_stride = k.kv_capacity * D; a.kv_seq_stride = (size_t)nkv * k.kv_capacity * D;
      a.kv_off = c->l_kvlen;
      a.max_len = max_new;
      // a masked cache: the key-drop form under the cache's mask (by absolute position; the new rows' bits are clear, so they see each other and not
      // what was hidden in front of them); kv_len_offset states the largest cached length for the check, the kernel reads kv_off
      if (c->kv_masked) { a.key_drop = c->kv_drop; a.ld_drop = c->kv_drop_ld; a.kv_len_offset = max_cached; }
      if (const char* m = aigv_attn_check(a, D)) return fail(c, AIGV_ERR_ARG, "%s", m);
      ProfScope ps(c, AIGV_PROF_ATTN_LLM, attn_flops, 2.0 * T * ((double)c->qkv_out + H), s);
      HIPCHK(c, aigv_launch_attention(a, D, s));
    }
    TRY(llm_layer_post(c, li, T, s));
  }
  TRY(final_rows(c, score, B, R, argmax, c->l_h, false, s));
  if (commit) {
    for (int b = 0; b < B; ++b) {
      const int len = c->h_kvlen[b] + (cu[b + 1] - cu[b]);
      c->h_kvlen[b] = len;
      c->h_dec[b] = len; c->h_dec[2 * B + b] = len + 1;
    }
    HIPCHK(c, aigv_launch_write_ints(c->h_dec.data(), B, c->dec_pos, s));
    HIPCHK(c, aigv_launch_write_ints(c->h_dec.data() + 2 * B, B, c->dec_kvlen, s));
  }
  return 0;
}

// Replicate the kept sequences: slots [0, B) -> [B, 2B), ... so that `copies` different continuations of every sequence can
// be extended in ONE pass (the decoder weights are then streamed once for all of them).
int aigv_kv_fork(aigv_ctx* c, int copies, void* stream) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_kv_fork: null context");
  if (!c->kv_valid) return fail(c, AIGV_ERR_STATE, "aigv_kv_fork: no KV state (run aigv_llm_prefill with keep_kv)");
  const aigv_config& k = c->cfg;
  const int B = c->kv_seqs;
  if (copies < 1 || (long)B * copies > k.max_seqs) return fail(c, AIGV_ERR_ARG, "aigv_kv_fork: %d x %d sequences exceed max_seqs %d", B, copies, k.max_seqs);
  if (copies == 1) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  const size_t slot = (size_t)k.llm_kv_heads * k.kv_capacity * c->head_dim;      // elements per sequence and layer
  const size_t kv_layer = (size_t)k.max_seqs * slot;
  for (int li = 0; li < k.llm_layers; ++li)
    for (int cpy = 1; cpy < copies; ++cpy) {
      HIPCHK(c, hipMemcpyAsync(c->kc + li * kv_layer + (size_t)cpy * B * slot, c->kc + li * kv_layer, (size_t)B * slot * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
      HIPCHK(c, hipMemcpyAsync(c->vc + li * kv_layer + (size_t)cpy * B * slot, c->vc + li * kv_layer, (size_t)B * slot * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
    }
  if (c->kv_masked)   // the mask rows go with their slots
    for (int cpy = 1; cpy < copies; ++cpy)
      HIPCHK(c, hipMemcpyAsync(c->kv_drop + (size_t)cpy * B * c->kv_drop_ld, c->kv_drop, (size_t)B * c->kv_drop_ld * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  const int N = B * copies;
  c->h_kvlen.resize(N);
  for (int i = B; i < N; ++i) c->h_kvlen[i] = c->h_kvlen[i % B];
  return upload_decode_state(c, N, s);
}

// Beam search over the kept sequences: sequence i continues from what sequence parent[i] has cached (its first len[i] positions); the
// device-side positions of aigv_decode_step are untouched (all beams of a search have one length).  A gather into a second cache that
// is allocated on first use (workspace: freed and re-made by aigv_ctx_resize), after which the two caches swap.
int aigv_kv_reorder(aigv_ctx* c, const int32_t* parent, const int32_t* len, int n, void* stream) {
  if (!c || !parent || !len) return fail(c, AIGV_ERR_ARG, "aigv_kv_reorder: null argument");
  if (!c->kv_valid) return fail(c, AIGV_ERR_STATE, "aigv_kv_reorder: no KV state (run aigv_llm_prefill with keep_kv)");
  const aigv_config& k = c->cfg;
  if (n != c->kv_seqs) return fail(c, AIGV_ERR_ARG, "aigv_kv_reorder: %d sequences, the cache holds %d", n, c->kv_seqs);
  int max_len = 0;
  for (int i = 0; i < n; ++i) {
    if (parent[i] < 0 || parent[i] >= n) return fail(c, AIGV_ERR_ARG, "aigv_kv_reorder: parent[%d] = %d outside 0..%d", i, parent[i], n - 1);
    if (len[i] <= 0 || len[i] > k.kv_capacity) return fail(c, AIGV_ERR_ARG, "aigv_kv_reorder: len[%d] = %d outside 1..%d", i, len[i], k.kv_capacity);
    max_len = std::max(max_len, len[i]);
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  if (!c->kc_alt || !c->vc_alt || !c->beam_ints) {
    // The second cache is made on first use.  No memset: the gather below writes every position a later step reads, and a
    // blocking null-stream memset would not be ordered against a gather on a non-blocking stream `s`.  All three or none: a partial
    // failure frees what it got, so the next call starts over instead of finding one pointer set.
    const size_t per = (size_t)k.llm_layers * k.max_seqs * k.llm_kv_heads * k.kv_capacity * c->head_dim;
    void *a = nullptr, *b = nullptr, *i = nullptr;
    const hipError_t e1 = hipMalloc(&a, per * sizeof(bf16_t));
    const hipError_t e2 = e1 == hipSuccess ? hipMalloc(&b, per * sizeof(bf16_t)) : e1;
    const hipError_t e3 = e2 == hipSuccess ? hipMalloc(&i, (size_t)2 * k.max_seqs * sizeof(int32_t)) : e2;
    if (e3 != hipSuccess) {
      if (a) hipFree(a);
      if (b) hipFree(b);
      if (i) hipFree(i);
      c->kc_alt = c->vc_alt = nullptr; c->beam_ints = nullptr;
      return fail(c, AIGV_ERR_ALLOC, "aigv_kv_reorder: second KV cache (2 x %zu bytes): %s", per * sizeof(bf16_t), hipGetErrorString(e3));
    }
    c->kc_alt = (bf16_t*)a; c->vc_alt = (bf16_t*)b; c->beam_ints = (int32_t*)i;
    c->ws_allocs.push_back(a); c->ws_allocs.push_back(b); c->ws_allocs.push_back(i);
  }
  HIPCHK(c, aigv_launch_write_ints(parent, n, c->beam_ints, s));
  HIPCHK(c, aigv_launch_write_ints(len, n, c->beam_ints + k.max_seqs, s));
  const size_t kv_layer = (size_t)k.max_seqs * k.llm_kv_heads * k.kv_capacity * c->head_dim;
  hipError_t e = aigv_launch_kv_reorder(c->kc, c->vc, c->kc_alt, c->vc_alt, c->beam_ints, c->beam_ints + k.max_seqs, n, k.llm_layers, k.llm_kv_heads,
                                        k.kv_capacity, c->head_dim, kv_layer, max_len, s);
  if (e != hipSuccess) return fail(c, AIGV_ERR_HIP, "aigv_kv_reorder (n=%d): %s", n, hipGetErrorString(e));
  std::swap(c->kc, c->kc_alt);
  std::swap(c->vc, c->vc_alt);
  if (c->kv_masked) {   // the mask rows are gathered by parent like the slots (cut to len: what a beam appends is visible), then the two buffers swap
    HIPCHK(c, aigv_launch_kv_drop_rows(c->kv_drop, c->kv_drop_ld, c->beam_ints, c->beam_ints + k.max_seqs, 0, c->kv_drop_alt, c->kv_drop_ld, n, s));
    std::swap(c->kv_drop, c->kv_drop_alt);
  }
  return 0;
}

// Which form (P = 1, 2, 4: 16, 8, 4 rows of W per workgroup and slab) each decode GEMV runs in.  A GEMV's rate depends on how
// evenly its workgroups fill the 256 CUs and on how many there are (scripts/gemv_balance_probe.py; in-box sweep of the 8B decode
// step, profiles/r2_decode_forms.txt: wqkv 1 -> 4: -0.16 ms/token, w1|w3 1 -> 2: -0.16, 1 -> 4: -0.24, w2 1 -> 2: -0.08, 1 -> 4: -0.04,
// wo: no change): the finest form the batch allows whose K sub-range per wave still fills one 8-deep load group; long-K GEMVs
// (w2) stop at 8 rows.
static int pick_form(int max_p, int K) {
  int best = 1;
  for (int p = 2; p <= max_p; p *= 2) {
    if (K % (128 * p) || K / (4 * p) < 256 || (K > 8192 && p > 2)) break;
    best = p;
  }
  return best;
}

static void decode_forms(aigv_ctx* c, int B, int* pq, int* po, int* p13, int* p2) {
  const aigv_config& k = c->cfg;
  const int max_p = B <= 4 ? 4 : B <= 8 ? 2 : 1;
  if (resolved_gemm_mode(c) == 1) {   // batch-invariant bits: ONE form whatever the batch (p = 1 here; run_skinny then pins the K split too)
    *pq = *po = *p13 = *p2 = 1;
    return;
  }
  *pq = *po = *p13 = pick_form(max_p, k.llm_hidden);
  *p2 = pick_form(max_p, k.llm_inter);
  // AIGV_TUNE_SKINNY_P (experiments): one value for all four, or - value = 1000 + a packed "wqkv, wo, w1|w3, w2" word with 3 bits each
  // (1 / 2 / 4) - one per GEMV (scripts/decode_bench.py; the sweep of profiles/r2_decode_forms.txt)
  if (const int sp = tune_knob(c, AIGV_TUNE_SKINNY_P)) {
    if (sp < 1000) *pq = *po = *p13 = *p2 = std::min(sp, max_p);
    else {
      int* out[4] = {pq, po, p13, p2};
      for (int i = 0; i < 4; ++i) {
        const int v = ((sp - 1000) >> (3 * i)) & 7;
        if ((v == 1 || v == 2 || v == 4) && v <= max_p) *out[i] = v;
      }
    }
  }
}

// decode attention of layer `li`: the new token of every sequence over its cached keys
static int decode_attention(aigv_ctx* c, int li, int B, int max_vis, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden, D = c->head_dim, g = c->g, nkv = k.llm_kv_heads;
  const size_t kv_layer = (size_t)k.max_seqs * nkv * k.kv_capacity * D;
  HIPCHK(c, aigv_launch_attention_decode(c->l_qkv, c->qkv_out, (g + 2) * D, c->kc + li * kv_layer, c->vc + li * kv_layer,
                                         c->dec_kvlen, k.kv_capacity, c->l_ao, H, B, nkv, g, D, sqrtf((float)D), max_vis,
                                         c->dec_ws, s, c->kv_masked ? c->kv_drop : nullptr, c->kv_drop_ld));   // a masked cache: the key-drop form (the appended keys' bits are clear)
  return 0;
}

// the bf16 tail of a decode layer, from the bf16 weights: h += wo(attention output);  h += w2(silu(w1 n) * w3 n), n = ffn_norm(h) - applied
// by the w1|w3 GEMV itself when `fused`.  po / p13 / p2: the GEMVs' forms (decode_forms).
static int decode_tail_bf16(aigv_ctx* c, const LlmLayer& L, int B, bool fused, int po, int p13, int p2, hipStream_t s) {
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden, I = k.llm_inter;
  TRY(run_skinny(c, c->l_ao, H, B, L.wo, H, H, H, nullptr, c->l_h, H, c->l_h, H, SK_RESID, s, po));
  if (fused) {
    ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * B * 2.0 * I * H, 2.0 * 2.0 * I * H, s);
    HIPCHK(c, aigv_launch_skinny_swiglu_normed(c->l_h, H, B, L.w13, H, 2 * I, H, c->l_ffn, I, L.fn, k.rms_eps, s, p13));
  } else {
    HIPCHK(c, aigv_launch_rmsnorm(c->l_h, H, L.fn, c->l_t, H, B, H, k.rms_eps, nullptr, s));
    TRY(run_skinny(c, c->l_t, H, B, L.w13, H, 2 * I, H, nullptr, nullptr, 0, c->l_ffn, I, SK_SWIGLU, s, p13));
  }
  TRY(run_skinny(c, c->l_ffn, I, B, L.w2, I, H, I, nullptr, c->l_h, H, c->l_h, H, SK_RESID, s, p2));
  return 0;
}

// aigv_decode_step / aigv_decode_step_logprob (logprob != nullptr: the lm-head runs its argmax + log-sum-exp form) /
// aigv_decode_step_cand_logprob (cand_lp != nullptr, C >= 1: the same form, with the candidates' GEMV in front of its finisher) /
// aigv_decode_step_topk_logprob (topk >= 1: the lm-head keeps its bf16 logits in c->l_lp - no scoring pass is in flight on a context that
// decodes - and the finisher selects from them; candidates stay optional)
static int decode_step(aigv_ctx* c, const int64_t* ids, int64_t* next, float* logprob, void* stream, const int64_t* cand = nullptr, int C = 0,
                       float* cand_lp = nullptr, int topk = 0, int64_t* top_ids = nullptr, float* top_lp = nullptr) {
  const char* op = topk ? "aigv_decode_step_topk_logprob" : cand_lp ? "aigv_decode_step_cand_logprob" : logprob ? "aigv_decode_step_logprob" : "aigv_decode_step";
  if (!c || !ids || !next) return fail(c, AIGV_ERR_ARG, "%s: null argument", op);
  if (!c->kv_valid) return fail(c, AIGV_ERR_STATE, "%s: no KV state (run aigv_llm_prefill with keep_kv)", op);
  const aigv_config& k = c->cfg;
  const int B = c->kv_seqs, H = k.llm_hidden, I = k.llm_inter, D = c->head_dim, g = c->g, nkv = k.llm_kv_heads;
  if (B > 64) return fail(c, AIGV_ERR_ARG, "decode supports at most 64 clips per step");
  for (int b = 0; b < B; ++b)
    if (c->h_kvlen[b] + 1 > k.kv_capacity || c->h_kvlen[b] + 1 > k.max_positions)
      return fail(c, AIGV_ERR_STATE, "clip %d: KV cache / RoPE table exhausted at %d tokens", b, c->h_kvlen[b]);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  // positions of the new tokens (= current lengths) and the visible KV lengths live on the device (dec_pos, dec_kvlen)
  // and are advanced by a one-block kernel at the end of the step: no host copies or syncs inside a decode step
  int max_vis = 0;
  for (int b = 0; b < B; ++b) max_vis = std::max(max_vis, c->h_kvlen[b] + 1);
  HIPCHK(c, aigv_launch_embed(ids, c->dec_slot, c->tok_emb, nullptr, nullptr, 0, c->l_h, B, H, s));
  const size_t kv_layer = (size_t)k.max_seqs * nkv * k.kv_capacity * D;
  // Up to 4 sequences: attention_norm / ffn_norm are applied by the GEMV that consumes them (NormArgs in head.hip; same bits), 6
  // launches per layer instead of 8.  AIGV_TUNE_DECODE_FUSED = 0 keeps the separate norm kernels (A/B).
  const Tune tn_ = tune_of(c);
  const bool fused = tn_[AIGV_TUNE_DECODE_FUSED] != 0 && B <= 4 && aigv_skinny_norm_fusable(H);
  // sub-slab forms of the four GEMVs (skinny_kernel's P; head.hip): chosen so that the workgroups come to a whole number per CU.
  // AIGV_TUNE_SKINNY_P / aigv_tune_skinny force one value everywhere it is legal (or one per GEMV: decode_forms).
  int pq, po, p13, p2;
  decode_forms(c, B, &pq, &po, &p13, &p2);
  // fp8 mode: the linears the prefill runs in e4m3 stream their e4m3 copies here too (head8.hip: half the bytes per token; the
  // x rows are normalised and quantised by the GEMV itself) - up to 4 sequences and for the widths the kernel is built for; larger
  // batches decode from the bf16 weights.  AIGV_TUNE_DECODE_FP8 = 0 keeps the bf16 GEMVs (A/B); AIGV_TUNE_SKINNY_P8 = one form for all four.
  const bool f8 = tn_[AIGV_TUNE_DECODE_FP8] != 0 && c->fp8_llm && B <= 4 && aigv_skinny_fp8_supported(H, true) && aigv_skinny_fp8_supported(I, false) && D == 128;
  int q8[4] = {4, 2, 4, 2};
  {
    if (const int v = tn_[AIGV_TUNE_SKINNY_P8])
      for (int i = 0; i < 4; ++i) q8[i] = v;
    if (I / (4 * q8[3]) < 256 || I % (512 * q8[3])) q8[3] = 1;
  }
  for (int li = 0; li < k.llm_layers; ++li) {
    const LlmLayer& L = c->llm[li];
    if (f8) {
      const LlmLayerFp8& Q = c->llm8[li];
      const bool post8 = li != k.llm_layers - 1;   // the post-attention half of the last layer stays bf16, as in the prefill
      const AigvRopeKv rk{c->dec_pos, c->dec_seq, c->rope_cos, c->rope_sin, c->kc + li * kv_layer, c->vc + li * kv_layer, g, nkv, k.kv_capacity};
      {
        ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * B * (double)c->qkv_out * H, (double)c->qkv_out * H, s);
        HIPCHK(c, aigv_launch_skinny_fp8(c->l_h, H, B, Q.wqkv, H, Q.s_wqkv, c->qkv_out, H, nullptr, 0, c->l_qkv, c->qkv_out, SK_ROPE_KV, &rk, L.an, k.rms_eps, q8[0], s));
      }
      TRY(decode_attention(c, li, B, max_vis, s));
      if (post8) {
        ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * B * ((double)H * H + 3.0 * H * I), (double)H * H + 3.0 * H * I, s);
        HIPCHK(c, aigv_launch_skinny_fp8(c->l_ao, H, B, Q.wo, H, Q.s_wo, H, H, c->l_h, H, c->l_h, H, SK_RESID, nullptr, nullptr, 0.f, q8[1], s));
        HIPCHK(c, aigv_launch_skinny_fp8(c->l_h, H, B, Q.w13, H, Q.s_w13, 2 * I, H, nullptr, 0, c->l_ffn, I, SK_SWIGLU, nullptr, L.fn, k.rms_eps, q8[2], s));
        HIPCHK(c, aigv_launch_skinny_fp8(c->l_ffn, I, B, Q.w2, I, Q.s_w2, H, I, c->l_h, H, c->l_h, H, SK_RESID, nullptr, nullptr, 0.f, q8[3], s));
      } else {
        TRY(decode_tail_bf16(c, L, B, fused, po, p13, p2, s));
      }
      continue;
    }
    if (!fused) HIPCHK(c, aigv_launch_rmsnorm(c->l_h, H, L.an, c->l_t, H, B, H, k.rms_eps, nullptr, s));
    {   // wqkv with RoPE + KV-cache append in its epilogue: one launch instead of GEMV + rope / store
      ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * B * (double)c->qkv_out * H, 2.0 * (double)c->qkv_out * H, s);
      HIPCHK(c, aigv_launch_skinny_rope_kv(fused ? c->l_h : c->l_t, H, B, L.wqkv, H, c->qkv_out, H, c->l_qkv, c->qkv_out, c->dec_pos, c->dec_seq, c->rope_cos,
                                           c->rope_sin, c->kc + li * kv_layer, c->vc + li * kv_layer, g, nkv, k.kv_capacity, D, s,
                                           fused ? L.an : nullptr, k.rms_eps, pq));
    }
    TRY(decode_attention(c, li, B, max_vis, s));
    TRY(decode_tail_bf16(c, L, B, fused, po, p13, p2, s));
  }
  HIPCHK(c, aigv_launch_rmsnorm(c->l_h, H, c->final_norm, c->l_rows, H, B, H, k.rms_eps, nullptr, s));
  if (logprob) HIPCHK(c, aigv_launch_lm_head_argmax_logprob(c->l_rows, B, H, c->lm_head, k.vocab, c->l_packed, c->dec_lse, next, nullptr, logprob, s, cand, C,
                                                            c->dec_cand, cand_lp, topk, c->l_lp, c->lp_ldo, top_ids, top_lp));
  else HIPCHK(c, aigv_launch_lm_head_argmax(c->l_rows, B, H, c->lm_head, k.vocab, c->l_packed, next, nullptr, s));
  HIPCHK(c, aigv_launch_advance(c->dec_pos, c->dec_kvlen, B, s));
  for (int b = 0; b < B; ++b) c->h_kvlen[b] += 1;
  return 0;
}

int aigv_decode_step(aigv_ctx* c, const int64_t* ids, int64_t* next, void* stream) { return decode_step(c, ids, next, nullptr, stream); }

int aigv_decode_step_logprob(aigv_ctx* c, const int64_t* ids, int64_t* next, float* logprob, void* stream) {
  if (!logprob) return fail(c, AIGV_ERR_ARG, "aigv_decode_step_logprob: null argument");
  return decode_step(c, ids, next, logprob, stream);
}

int aigv_decode_step_cand_logprob(aigv_ctx* c, const int64_t* ids, int64_t* next, float* logprob, const int64_t* cand_ids, int C, float* cand_logprob,
                                  void* stream) {
  const char* op = "aigv_decode_step_cand_logprob";
  if (C < 1 || C > AIGV_MAX_CANDIDATES) return fail(c, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d", op, C, AIGV_MAX_CANDIDATES);
  if (!logprob || !cand_ids || !cand_logprob) return fail(c, AIGV_ERR_ARG, "%s: null argument", op);
  return decode_step(c, ids, next, logprob, stream, cand_ids, C, cand_logprob);
}

int aigv_decode_step_topk_logprob(aigv_ctx* c, const int64_t* ids, int64_t* next, float* logprob, int k, int64_t* top_ids, float* top_logprob,
                                  const int64_t* cand_ids, int C, float* cand_logprob, void* stream) {
  const char* op = "aigv_decode_step_topk_logprob";
  if (k < 1 || k > AIGV_MAX_TOPK || (c && k > c->cfg.vocab)) return fail(c, AIGV_ERR_ARG, "%s: k = %d outside 1..min(%d, vocab)", op, k, AIGV_MAX_TOPK);
  if (cand_ids ? (C < 1 || C > AIGV_MAX_CANDIDATES) : C != 0) return fail(c, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d (0 without cand_ids)", op, C, AIGV_MAX_CANDIDATES);
  if (!logprob || !top_ids || !top_logprob || (cand_ids && !cand_logprob)) return fail(c, AIGV_ERR_ARG, "%s: null argument", op);
  return decode_step(c, ids, next, logprob, stream, cand_ids, C, cand_ids ? cand_logprob : nullptr, k, top_ids, top_logprob);
}

// What every aigv_out_row_* entry point checks before it touches the device - the handle and the caller's pointers (args_ok), finalized
// weights, the row window inside the consumed-row buffer - and the device selection.
static int out_rows_begin(aigv_ctx* c, const char* op, bool args_ok, int first_row, int n_rows) {
  if (!c || !args_ok) return fail(c, AIGV_ERR_ARG, "%s: null argument", op);
  if (!c->finalized) return fail(c, AIGV_ERR_STATE, "%s: call aigv_finalize_weights first", op);
  const int cap = c->cfg.max_out_rows + c->cfg.max_seqs + 64;
  if (first_row < 0 || n_rows <= 0 || first_row + n_rows > cap) return fail(c, AIGV_ERR_ARG, "%s: rows %d..%d outside 0..%d", op, first_row, first_row + n_rows - 1, cap - 1);
  HIPCHK(c, hipSetDevice(c->device));
  return 0;
}

int aigv_out_row_logits(aigv_ctx* c, int first_row, int n_rows, void* logits_bf16, int ldo, void* stream) {
  TRY(out_rows_begin(c, "aigv_out_row_logits", logits_bf16, first_row, n_rows));
  const aigv_config& k = c->cfg;
  hipStream_t s = (hipStream_t)stream;
  for (int r0 = 0; r0 < n_rows; r0 += 64) {
    const int rr = std::min(64, n_rows - r0);
    ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * rr * (double)k.vocab * k.llm_hidden, 2.0 * (double)k.vocab * k.llm_hidden, s);
    hipError_t e = aigv_launch_lm_head_logits(c->l_rows + (size_t)(first_row + r0) * k.llm_hidden, rr, k.llm_hidden, c->lm_head, k.vocab,
                                              (bf16_t*)logits_bf16 + (size_t)r0 * ldo, ldo, s);
    if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "lm-head logits (rows=%d ldo=%d): %s", rr, ldo, hipGetErrorString(e));
  }
  return 0;
}

// The loop of aigv_out_row_logprob (label_out: labels, one per row), aigv_out_row_cand_logprob (cand_out: C candidates for every row),
// aigv_out_row_topk_logprob (top_out: the k largest logits of every row, their ids into top_ids) and aigv_depth_lens_token_readout (top-1
// and candidates from one fill): n_rows normed rows at `rows` (leading dimension ld) in chunks of 64, the lm-head logits of a chunk into
// c->l_lp in the 4-slice form of every row count (a row's logits do not depend on its chunk), then the row kernels of logprob.hip read them.
static int row_logprobs(aigv_ctx* c, const bf16_t* rows, int ld, int n_rows, const int64_t* labels, float* label_out, const int64_t* cand, int C,
                        float* cand_out, int k_top, int64_t* top_ids, float* top_out, hipStream_t s) {
  const aigv_config& k = c->cfg;
  for (int r0 = 0; r0 < n_rows; r0 += 64) {
    const int rr = std::min(64, n_rows - r0);
    {
      ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * rr * (double)k.vocab * k.llm_hidden, 2.0 * (double)k.vocab * k.llm_hidden, s);
      hipError_t e = aigv_launch_lm_head_logits(rows + (size_t)r0 * ld, rr, k.llm_hidden, c->lm_head, k.vocab, c->l_lp, c->lp_ldo, s, /*one_form=*/true, ld);
      if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "lm-head logits (rows=%d ldo=%d): %s", rr, c->lp_ldo, hipGetErrorString(e));
    }
    if (top_out) {
      const hipError_t e = aigv_launch_topk_logprob(c->l_lp, rr, k.vocab, c->lp_ldo, k_top, top_ids + (size_t)r0 * k_top, top_out + (size_t)r0 * k_top, s);
      if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "top-k log-probabilities (rows=%d, k=%d): %s", rr, k_top, hipGetErrorString(e));
    }
    if (label_out) {
      const hipError_t e = aigv_launch_label_logprob(c->l_lp, rr, k.vocab, c->lp_ldo, labels + r0, label_out + r0, s);
      if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "label log-probabilities (rows=%d): %s", rr, hipGetErrorString(e));
    }
    if (cand_out) {
      const hipError_t e = aigv_launch_cand_logprob(c->l_lp, rr, k.vocab, c->lp_ldo, cand, C, cand_out + (size_t)r0 * C, s);
      if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "candidate log-probabilities (rows=%d, C=%d): %s", rr, C, hipGetErrorString(e));
    }
  }
  return 0;
}

int aigv_out_row_logprob(aigv_ctx* c, int first_row, int n_rows, const int64_t* labels, float* logprob, void* stream) {
  TRY(out_rows_begin(c, "aigv_out_row_logprob", labels && logprob, first_row, n_rows));
  return row_logprobs(c, c->l_rows + (size_t)first_row * c->cfg.llm_hidden, c->cfg.llm_hidden, n_rows, labels, logprob, nullptr, 0, nullptr, 0, nullptr, nullptr, (hipStream_t)stream);
}

int aigv_out_row_cand_logprob(aigv_ctx* c, int first_row, int n_rows, const int64_t* cand_ids, int C, float* cand_logprob, void* stream) {
  const char* op = "aigv_out_row_cand_logprob";
  if (C < 1 || C > AIGV_MAX_CANDIDATES) return fail(c, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d", op, C, AIGV_MAX_CANDIDATES);
  TRY(out_rows_begin(c, op, cand_ids && cand_logprob, first_row, n_rows));
  return row_logprobs(c, c->l_rows + (size_t)first_row * c->cfg.llm_hidden, c->cfg.llm_hidden, n_rows, nullptr, nullptr, cand_ids, C, cand_logprob, 0, nullptr, nullptr, (hipStream_t)stream);
}

int aigv_out_row_topk_logprob(aigv_ctx* c, int first_row, int n_rows, int k, int64_t* top_ids, float* top_logprob, void* stream) {
  const char* op = "aigv_out_row_topk_logprob";
  if (k < 1 || k > AIGV_MAX_TOPK || (c && k > c->cfg.vocab)) return fail(c, AIGV_ERR_ARG, "%s: k = %d outside 1..min(%d, vocab)", op, k, AIGV_MAX_TOPK);
  TRY(out_rows_begin(c, op, top_ids && top_logprob, first_row, n_rows));
  return row_logprobs(c, c->l_rows + (size_t)first_row * c->cfg.llm_hidden, c->cfg.llm_hidden, n_rows, nullptr, nullptr, nullptr, 0, nullptr, k, top_ids, top_logprob, (hipStream_t)stream);
}

// the depth lens' lm-head read-out (include/aigv_amd.h): the caller's normed rows instead of the consumed-row buffer, top-1 and candidates from one fill
int aigv_depth_lens_token_readout(aigv_ctx* c, const void* normed_rows_dev, int ld, int n_rows, const int64_t* cand_ids, int C, int64_t* top_id,
                                  float* top_logprob, float* cand_logprob, void* stream) {
  const char* op = "aigv_depth_lens_token_readout";
  if (!c || !normed_rows_dev || !top_id || !top_logprob) return fail(c, AIGV_ERR_ARG, "%s: null argument", op);
  if (!c->finalized) return fail(c, AIGV_ERR_STATE, "%s: call aigv_finalize_weights first", op);
  if (n_rows < 1) return fail(c, AIGV_ERR_ARG, "%s: n_rows = %d must be positive", op, n_rows);
  if (ld < c->cfg.llm_hidden || ld % 8 || ((uintptr_t)normed_rows_dev & 15))
    return fail(c, AIGV_ERR_ARG, "%s: the rows must be 16-byte aligned with a leading dimension (%d) that is a multiple of 8 and >= %d", op, ld, c->cfg.llm_hidden);
  if (cand_ids || cand_logprob || C) {
    if (C < 1 || C > AIGV_MAX_CANDIDATES) return fail(c, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d", op, C, AIGV_MAX_CANDIDATES);
    if (!cand_ids || !cand_logprob) return fail(c, AIGV_ERR_ARG, "%s: null argument (cand_ids and cand_logprob go together)", op);
  }
  HIPCHK(c, hipSetDevice(c->device));
  return row_logprobs(c, (const bf16_t*)normed_rows_dev, ld, n_rows, nullptr, nullptr, cand_ids, C, cand_logprob, 1, top_id, top_logprob, (hipStream_t)stream);
}

int aigv_out_row_hidden(aigv_ctx* c, int first_row, int n_rows, void* hidden_bf16, int ldo, void* stream) {
  TRY(out_rows_begin(c, "aigv_out_row_hidden", hidden_bf16, first_row, n_rows));
  const aigv_config& k = c->cfg;
  if (ldo < k.llm_hidden) return fail(c, AIGV_ERR_ARG, "aigv_out_row_hidden: ldo %d < %d", ldo, k.llm_hidden);
  HIPCHK(c, hipMemcpy2DAsync(hidden_bf16, (size_t)ldo * sizeof(bf16_t), c->l_rows + (size_t)first_row * k.llm_hidden, (size_t)k.llm_hidden * sizeof(bf16_t),
                             (size_t)k.llm_hidden * sizeof(bf16_t), n_rows, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int aigv_decode_eos(aigv_ctx* c, int64_t* tokens, int32_t* state, const int64_t* eos_ids, int n_eos, int64_t pad_id, void* stream) {
  if (!c || !tokens || !state) return fail(c, AIGV_ERR_ARG, "aigv_decode_eos: null argument");
  if (!c->kv_valid) return fail(c, AIGV_ERR_STATE, "aigv_decode_eos: no KV state (run aigv_llm_prefill with keep_kv)");
  if (n_eos < 0 || n_eos > 8 || (n_eos > 0 && !eos_ids)) return fail(c, AIGV_ERR_ARG, "aigv_decode_eos: 0..8 end-of-sequence ids");
  if (c->kv_seqs > 64) return fail(c, AIGV_ERR_ARG, "aigv_decode_eos: at most 64 sequences");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, aigv_launch_decode_eos(tokens, state, c->kv_seqs, eos_ids, n_eos, pad_id, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
