// Life cycle of a context of the C ABI (include/aigv_amd.h): creation, the capacity-sized workspaces, the weight store and the fp8 copies
// of the InternLM2 linears; the error text behind aigv_last_error.  Host-side C++ only.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "ctx.h"

using namespace aigv;

static thread_local std::string g_err;

int aigv::fail(aigv_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  g_err = buf;
  return code;
}

static_assert(AIGV_MAX_KV_CAPACITY == AIGV_DECODE_MAX_CHUNKS * AIGV_DECODE_KEYS_PER_CHUNK, "the header's bound is the decode merge pass's");

// The KV capacity every kernel of the context can serve: the decode attention's merge pass bounds it (kernels.h); the others
// address the caches in 64-bit offsets.
static const char* kv_capacity_check(int kv_capacity) {
  if (kv_capacity < 0 || kv_capacity > AIGV_MAX_KV_CAPACITY)
    return kv_capacity < 0 ? "kv_capacity must not be negative"
                           : "kv_capacity above AIGV_MAX_KV_CAPACITY (262144 tokens per clip: the decode attention's merge pass holds its chunk statistics in LDS)";
  return nullptr;
}

static inline uint16_t f32_to_bf16_host(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float bf16_to_f32_host(uint16_t v) {
  uint32_t u = (uint32_t)v << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

static int roundup(int x, int m) { return (x + m - 1) / m * m; }

static void drop_alloc(aigv_ctx* c, void* p) {   // frees one weight-side allocation (dalloc outside the workspace phase)
  if (!p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) c->allocs.erase(it);
  hipFree(p);
}

static int need(aigv_ctx* c, const std::string& name, size_t elems, const bf16_t** out) {
  auto it = c->w.find(name);
  if (it == c->w.end()) return fail(c, AIGV_ERR_STATE, "weight '%s' was never loaded", name.c_str());
  if (it->second.bytes != elems * 2)
    return fail(c, AIGV_ERR_STATE, "weight '%s' has %zu elements, expected %zu", name.c_str(), it->second.bytes / 2, elems);
  *out = (const bf16_t*)it->second.p;
  return 0;
}

void aigv_set_error(const char* msg) { g_err = msg ? msg : ""; }

// ==========================================================================================================
extern "C" {

int aigv_abi_version(void) { return AIGV_ABI_VERSION; }
int aigv_sizeof_config(void) { return (int)sizeof(aigv_config); }

const char* aigv_last_error(const aigv_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

void aigv_clear_hip_error(void) { (void)hipGetLastError(); }

// Everything whose size depends on the capacities of aigv_config (frames, tokens, sequences, output rows, KV): activations, index
// arrays, split-K scratch, KV caches.  Booked in ws_allocs so that aigv_ctx_resize can replace them without touching the weights.
static int alloc_workspaces(aigv_ctx* c) {
  const aigv_config& k = c->cfg;
  hipError_t e = hipSuccess;
  int rc = 0;
  c->ws_phase = true;
  c->kc = c->vc = nullptr;   // (no KV capacity: no caches)
  c->kc_alt = c->vc_alt = nullptr; c->beam_ints = nullptr;
  c->kv_drop = c->kv_drop_alt = nullptr; c->kv_drop_ld = 0; c->kv_masked = false;
  c->dec_ws = nullptr; c->dec_pos = c->dec_seq = c->dec_kvlen = c->dec_slot = nullptr;
  const size_t vr = (size_t)k.vit_chunk * c->S;
  const size_t pr = (size_t)k.vit_chunk * c->ntok;
  const size_t T = (size_t)k.max_tokens;
  do {
    if ((rc = dalloc(c, &c->v_col, (size_t)k.vit_chunk * c->np * c->Kp))) break;
    if ((rc = dalloc(c, &c->v_x, vr * k.vit_hidden))) break;
    if ((rc = dalloc(c, &c->v_t, vr * k.vit_hidden))) break;
    if ((rc = dalloc(c, &c->v_qkv, vr * 3 * k.vit_hidden))) break;
    if ((rc = dalloc(c, &c->v_ao, vr * k.vit_hidden))) break;
    if ((rc = dalloc(c, &c->v_h, vr * k.vit_inter))) break;
    if ((rc = dalloc(c, &c->v_cu, (size_t)k.vit_chunk + 1))) break;
    if ((rc = dalloc(c, &c->v_mapstats, (size_t)k.vit_chunk * k.vit_heads * c->S))) break;   // (here, never inside a pass: aigv_vit_attention_arm)
    if ((rc = dalloc(c, &c->p_t, pr * c->proj_in))) break;
    if ((rc = dalloc(c, &c->p_mid, pr * k.llm_hidden))) break;
    if ((rc = dalloc(c, &c->l_h, T * k.llm_hidden))) break;
    if ((rc = dalloc(c, &c->l_t, T * k.llm_hidden))) break;
    if ((rc = dalloc(c, &c->l_qkv, T * c->qkv_out))) break;
    if ((rc = dalloc(c, &c->l_ao, T * k.llm_hidden))) break;
    if ((rc = dalloc(c, &c->l_ffn, T * k.llm_inter))) break;
    if ((rc = dalloc(c, &c->l_rows, (size_t)(k.max_out_rows + k.max_seqs + 64) * k.llm_hidden))) break;
    if ((rc = dalloc(c, &c->l_pos, T))) break;
    if ((rc = dalloc(c, &c->l_seq, T))) break;
    if ((rc = dalloc(c, &c->l_cu, (size_t)k.max_seqs + 1))) break;
    if ((rc = dalloc(c, &c->l_rowidx, (size_t)k.max_out_rows + k.max_seqs + 64))) break;
    if ((rc = dalloc(c, &c->l_rowidx2, (size_t)k.max_out_rows + k.max_seqs + 64))) break;
    if ((rc = dalloc(c, &c->l_kvlen, (size_t)k.max_seqs))) break;
    if ((rc = dalloc(c, &c->l_packed, (size_t)64))) break;
    if ((rc = dalloc(c, &c->l_trim, (size_t)64 * (2 * k.llm_hidden + k.llm_inter)))) break;
    if ((rc = dalloc(c, &c->l_trim_h, (size_t)(k.max_out_rows + k.max_seqs + 64) * k.llm_hidden))) break;
    if ((rc = dalloc(c, &c->l_neg1, (size_t)k.max_tokens))) break;
    if ((rc = dalloc(c, &c->l_lensidx, (size_t)4 * AIGV_MAX_LENS_ROWS))) break;   // (here, never inside a pass: the armed pass may be captured)
    if ((rc = dalloc(c, &c->l_streamidx, (size_t)2 * k.max_tokens))) break;      // (likewise: the row numbers of a stream patch | of a stream capture)
    if ((rc = dalloc(c, &c->l_headidx, (size_t)3 * k.max_tokens))) break;        // (likewise: those of a head scale | of a head patch | of a head capture)
    if ((rc = dalloc(c, &c->l_neuronidx, (size_t)9 * k.max_tokens))) break;      // (likewise: per neuron option its rows | its last-layer activation rows | their side rows)
    if ((rc = dalloc(c, &c->l_neuroncol, (size_t)3 * AIGV_MAX_NEURON_SEL))) break;   // (likewise: the column lists of a neuron scale | patch | capture)
    if ((rc = dalloc(c, &c->l_neuronfac, (size_t)AIGV_MAX_NEURON_SEL))) break;       // (likewise: the factors of a sparse neuron scale)
    c->rp_vit = RowPlan(); c->rp_llm = RowPlan(); c->cur_rp = nullptr;
    c->rp_vit.cap_halves = (int)(vr / 128) + 2 * k.vit_chunk + 2;
    c->rp_llm.cap_halves = (int)(T / 128) + 2 * k.max_seqs + 2;
    if ((rc = dalloc(c, &c->rp_vit.d_tab, (size_t)2 * c->rp_vit.cap_halves))) break;
    if ((rc = dalloc(c, &c->rp_llm.d_tab, (size_t)2 * c->rp_llm.cap_halves))) break;
    {   // split-K slabs: the planner's cap, or less when no GEMM of this context can reach it (8 slices x most rows x widest N)
      const size_t widest = (size_t)std::max(std::max(std::max(2 * k.llm_inter, c->qkv_out), std::max(k.vit_inter, 3 * k.vit_hidden)), k.llm_hidden);
      const size_t rows = std::max((size_t)k.max_tokens, (size_t)k.vit_chunk * c->S);
      c->splitk_floats = std::min(SPLITK_MAX_FLOATS, (size_t)8 * rows * widest);
      void* p = nullptr;
      if (hipMalloc(&p, c->splitk_floats * sizeof(float)) != hipSuccess) { rc = fail(c, AIGV_ERR_ALLOC, "hipMalloc(split-K scratch) failed"); break; }
      c->ws_allocs.push_back(p);
      c->splitk_ws = (float*)p;
      // the InternViT half (same size: `rows` / `widest` above cover its GEMMs)
      if (hipMalloc(&p, c->splitk_floats * sizeof(float)) != hipSuccess) { rc = fail(c, AIGV_ERR_ALLOC, "hipMalloc(split-K scratch, InternViT) failed"); break; }
      c->ws_allocs.push_back(p);
      c->splitk_ws_vit = (float*)p;
    }
    if (hipMemset(c->l_neg1, 0xFF, (size_t)k.max_tokens * sizeof(int32_t)) != hipSuccess) { rc = fail(c, AIGV_ERR_HIP, "hipMemset failed"); break; }
    {
      int maxd = k.llm_hidden;
      for (int i = 0; i < k.n_score_layers; ++i) maxd = std::max(maxd, (int)k.score_dims[i]);
      if ((rc = dalloc(c, &c->l_score_ws, (size_t)3 * 64 * maxd))) break;
    }
    c->lp_ldo = (k.vocab + 3) / 4 * 4;   // allocated here, never inside a pass: the logprob pass may be captured into a graph
    if ((rc = dalloc(c, &c->l_lp, (size_t)64 * c->lp_ldo))) break;
    // allocated here for the same reason (a decode step may be captured); a resize re-runs this function
    if ((rc = dalloc(c, &c->dec_lse, (size_t)std::min(k.max_seqs, 64) * aigv_lm_head_lse_slots(k.vocab)))) break;
    if ((rc = dalloc(c, &c->dec_cand, aigv_cand_logit_elems(std::min(k.max_seqs, 64))))) break;
    if (k.kv_capacity > 0) {
      const size_t per = (size_t)k.llm_layers * k.max_seqs * k.llm_kv_heads * k.kv_capacity * c->head_dim;
      if ((rc = dalloc(c, &c->kc, per))) break;
      if ((rc = dalloc(c, &c->vc, per))) break;
      c->kv_drop_ld = (k.kv_capacity + 63) / 64;   // the caches' key-drop mask and the buffer aigv_kv_reorder gathers it into (a few KB: never made inside a pass)
      if ((rc = dalloc(c, &c->kv_drop, (size_t)k.max_seqs * c->kv_drop_ld))) break;
      if ((rc = dalloc(c, &c->kv_drop_alt, (size_t)k.max_seqs * c->kv_drop_ld))) break;
      if ((rc = dalloc(c, &c->dec_ws, aigv_attention_decode_ws_floats(k.max_seqs, k.llm_kv_heads, c->g, k.kv_capacity)))) break;
      if ((rc = dalloc(c, &c->dec_pos, (size_t)k.max_seqs))) break;
      if ((rc = dalloc(c, &c->dec_seq, (size_t)k.max_seqs))) break;
      if ((rc = dalloc(c, &c->dec_kvlen, (size_t)k.max_seqs))) break;
      if ((rc = dalloc(c, &c->dec_slot, (size_t)k.max_seqs))) break;
    }
    std::vector<int32_t> cu(k.vit_chunk + 1);
    for (int i = 0; i <= k.vit_chunk; ++i) cu[i] = i * c->S;
    e = hipMemcpy(c->v_cu, cu.data(), cu.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = fail(c, AIGV_ERR_HIP, "hipMemcpy: %s", hipGetErrorString(e));
  } while (0);
  c->ws_phase = false;
  return rc;
}

int aigv_ctx_create(int device, const aigv_config* cfg, aigv_ctx** out) {
  if (!cfg || !out) return fail(nullptr, AIGV_ERR_ARG, "aigv_ctx_create: null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, AIGV_ERR_HIP, "aigv_ctx_create: no HIP device is visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, AIGV_ERR_ARG, "aigv_ctx_create: device %d out of range (%d visible)", device, ndev);
  const aigv_config& k = *cfg;
  // ---- shape constraints of the kernels ----
  if (k.vit_hidden <= 0 || k.vit_heads <= 0 || k.vit_hidden % k.vit_heads) return fail(nullptr, AIGV_ERR_ARG, "bad ViT head split");
  if (k.vit_hidden / k.vit_heads != 64 && k.vit_hidden / k.vit_heads != 128)
    return fail(nullptr, AIGV_ERR_ARG, "ViT head_dim %d not supported (64 or 128)", k.vit_hidden / k.vit_heads);
  if (k.llm_hidden <= 0 || k.llm_heads <= 0 || k.llm_hidden % k.llm_heads || k.llm_hidden / k.llm_heads != 128)
    return fail(nullptr, AIGV_ERR_ARG, "LLM head_dim must be 128");
  if (k.llm_kv_heads <= 0 || k.llm_heads % k.llm_kv_heads) return fail(nullptr, AIGV_ERR_ARG, "bad GQA split");
  if (k.llm_heads / k.llm_kv_heads > 8)   // the decode attention is instantiated for 1..8 query heads per KV head (InternLM2-8B: 4, -20B: 6): say so here, not at the first decode step
    return fail(nullptr, AIGV_ERR_ARG, "GQA groups of more than 8 query heads per KV head are not supported (%d / %d)", k.llm_heads, k.llm_kv_heads);
  if (k.vit_hidden % 128 || k.vit_inter % 128 || k.llm_hidden % 128 || k.llm_inter % 128)
    return fail(nullptr, AIGV_ERR_ARG, "hidden/intermediate sizes must be multiples of 128");
  if (k.image_size % k.patch_size || k.shuffle != 2 || ((k.image_size / k.patch_size) % 2))
    return fail(nullptr, AIGV_ERR_ARG, "image/patch/shuffle combination not supported");
  if (k.motion_dim % 128) return fail(nullptr, AIGV_ERR_ARG, "motion_dim must be a multiple of 128");
  if (k.n_score_layers < 1 || k.n_score_layers > 8) return fail(nullptr, AIGV_ERR_ARG, "n_score_layers out of range");
  if (k.max_frames <= 0 || k.vit_chunk <= 0 || k.max_tokens <= 0 || k.max_seqs <= 0 || k.max_out_rows <= 0)
    return fail(nullptr, AIGV_ERR_ARG, "capacities must be positive");
  if (const char* m = kv_capacity_check(k.kv_capacity)) return fail(nullptr, AIGV_ERR_ARG, "%s", m);

  aigv_ctx* c = new (std::nothrow) aigv_ctx();
  if (!c) return fail(nullptr, AIGV_ERR_ALLOC, "out of host memory");
  c->cfg = k;
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) { delete c; return fail(nullptr, AIGV_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e)); }
  c->grid = k.image_size / k.patch_size;
  c->np = c->grid * c->grid;
  c->S = c->np + 1;
  c->Kp = roundup(k.num_channels * k.patch_size * k.patch_size, 64);
  c->ntok = c->np / (k.shuffle * k.shuffle);
  c->proj_in = k.vit_hidden * k.shuffle * k.shuffle;
  c->head_dim = k.llm_hidden / k.llm_heads;
  c->vit_head_dim = k.vit_hidden / k.vit_heads;
  c->g = k.llm_heads / k.llm_kv_heads;
  c->qkv_out = (k.llm_heads + 2 * k.llm_kv_heads) * c->head_dim;

  int rc = alloc_workspaces(c);
  if (rc) {
    g_err = c->err;
    aigv_ctx_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void aigv_ctx_destroy(aigv_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  for (void* p : c->allocs) hipFree(p);
  for (void* p : c->ws_allocs) hipFree(p);
  for (auto& kv : c->w) hipFree(kv.second.p);
  for (auto& r : c->recs) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
  for (auto e : c->ev_pool) hipEventDestroy(e);
  delete c;
}

int aigv_ctx_resize(aigv_ctx* c, const aigv_config* cfg) {
  if (!c || !cfg) return fail(c, AIGV_ERR_ARG, "aigv_ctx_resize: null argument");
  aigv_config a = c->cfg, b = *cfg;   // the model must be the same: compare with the capacity fields levelled
  a.max_frames = b.max_frames; a.vit_chunk = b.vit_chunk; a.max_tokens = b.max_tokens; a.max_seqs = b.max_seqs; a.max_out_rows = b.max_out_rows;
  a.kv_capacity = b.kv_capacity; a.max_positions = b.max_positions;
  if (memcmp(&a, &b, sizeof(aigv_config)) != 0) return fail(c, AIGV_ERR_ARG, "aigv_ctx_resize: only the capacities may change (create a new context for another model)");
  if (b.max_frames <= 0 || b.vit_chunk <= 0 || b.max_tokens <= 0 || b.max_seqs <= 0 || b.max_out_rows <= 0)
    return fail(c, AIGV_ERR_ARG, "capacities must be positive");
  if (const char* m = kv_capacity_check(b.kv_capacity)) return fail(c, AIGV_ERR_ARG, "%s", m);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  for (void* p : c->ws_allocs) hipFree(p);
  c->ws_allocs.clear();
  const bool had_q8 = c->q8 != nullptr;
  if (had_q8) {   // the e4m3 activation rows are sized by max_tokens too (they live on the weight side: aigv_set_precision made them)
    drop_alloc(c, c->q8); drop_alloc(c, c->q8_scale);
    c->q8 = nullptr; c->q8_scale = nullptr;
  }
  const int old_pos = c->cfg.max_positions;
  c->cfg = b;
  c->kv_valid = false;   // (alloc_workspaces clears kv_masked with the mask buffers it re-makes)
  int rc = alloc_workspaces(c);
  if (!rc && had_q8) {
    rc = dalloc(c, &c->q8, (size_t)b.max_tokens * (size_t)std::max(b.llm_hidden, b.llm_inter));
    if (!rc) rc = dalloc(c, &c->q8_scale, (size_t)b.max_tokens);
  }
  if (rc) return rc;   // the context is unusable after a failed resize: destroy it
  if (b.max_positions != old_pos) c->finalized = false;   // the rotary tables must be loaded again at the new length, then aigv_finalize_weights
  return 0;
}

int aigv_load_weight(aigv_ctx* c, const char* name, const void* data, const int64_t* shape, int ndim, int dtype,
                     int on_device) {
  if (!c || !name || !data || !shape || ndim <= 0) return fail(c, AIGV_ERR_ARG, "aigv_load_weight: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] <= 0) return fail(c, AIGV_ERR_ARG, "aigv_load_weight(%s): bad shape", name);
    n *= (size_t)shape[i];
  }
  const std::string key(name);
  const aigv_config& k = c->cfg;
  const bool is_patch = key == "vision_model.embeddings.patch_embedding.weight";
  const bool is_w1 = key.find("feed_forward.w1.weight") != std::string::npos;
  const bool is_w3 = key.find("feed_forward.w3.weight") != std::string::npos;
  std::vector<uint16_t> host;
  const void* src = data;           // bf16 source (host or device)
  bool src_dev = on_device != 0;
  if (dtype == AIGV_F32 || is_patch) {
    // stage through the host: convert and/or repack
    std::vector<uint8_t> raw;
    const void* hsrc = data;
    const size_t esz = dtype == AIGV_F32 ? 4 : 2;
    if (on_device) {
      raw.resize(n * esz);
      HIPCHK(c, hipMemcpy(raw.data(), data, n * esz, hipMemcpyDeviceToHost));
      hsrc = raw.data();
    }
    host.resize(n);
    if (dtype == AIGV_F32) for (size_t i = 0; i < n; ++i) host[i] = f32_to_bf16_host(((const float*)hsrc)[i]);
    else memcpy(host.data(), hsrc, n * 2);
    if (is_patch) {  // [Hv, C, P, P] -> [Hv, Kp] zero padded
      const size_t kk = (size_t)k.num_channels * k.patch_size * k.patch_size;
      if (n != (size_t)k.vit_hidden * kk) return fail(c, AIGV_ERR_ARG, "patch_embedding.weight has the wrong size");
      std::vector<uint16_t> padded((size_t)k.vit_hidden * c->Kp, 0);
      for (int r = 0; r < k.vit_hidden; ++r) memcpy(&padded[(size_t)r * c->Kp], &host[(size_t)r * kk], kk * 2);
      host.swap(padded);
      n = host.size();
    }
    src = host.data();
    src_dev = false;
  } else if (dtype != AIGV_BF16) {
    return fail(c, AIGV_ERR_ARG, "aigv_load_weight(%s): unknown dtype %d", name, dtype);
  }

  if (is_w1 || is_w3) {
    // w1 / w3 [I, H] are stored interleaved in 16-row blocks (even block = w1, odd = w3) for the SwiGLU epilogue
    if (ndim != 2 || shape[0] != k.llm_inter || shape[1] != k.llm_hidden)
      return fail(c, AIGV_ERR_ARG, "aigv_load_weight(%s): expected [%d,%d]", name, k.llm_inter, k.llm_hidden);
    std::string fused = key.substr(0, key.find("feed_forward.")) + "feed_forward.w13.weight";
    auto it = c->w.find(fused);
    if (it == c->w.end()) {
      DevBuf b;
      b.bytes = (size_t)2 * k.llm_inter * k.llm_hidden * 2;
      hipError_t e = hipMalloc(&b.p, b.bytes);
      if (e != hipSuccess) return fail(c, AIGV_ERR_ALLOC, "hipMalloc(%zu) for %s: %s", b.bytes, fused.c_str(), hipGetErrorString(e));
      it = c->w.emplace(fused, b).first;
    }
    const size_t blk = (size_t)16 * k.llm_hidden * 2;  // bytes of one 16-row block
    char* dst = (char*)it->second.p + (is_w3 ? blk : 0);
    HIPCHK(c, hipMemcpy2D(dst, 2 * blk, src, blk, blk, k.llm_inter / 16, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    c->w[key + "#seen"] = DevBuf{};  // marker (no storage)
    c->finalized = false;
    c->llm_lin_dirty = true;
    return 0;
  }

  auto it = c->w.find(key);
  if (it != c->w.end() && it->second.bytes != n * 2) {
    hipFree(it->second.p);
    c->w.erase(it);
    it = c->w.end();
  }
  if (it == c->w.end()) {
    DevBuf b;
    b.bytes = n * 2;
    hipError_t e = hipMalloc(&b.p, b.bytes);
    if (e != hipSuccess) return fail(c, AIGV_ERR_ALLOC, "hipMalloc(%zu) for %s: %s", b.bytes, name, hipGetErrorString(e));
    it = c->w.emplace(key, b).first;
  }
  HIPCHK(c, hipMemcpy(it->second.p, src, n * 2, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  c->finalized = false;
  if (key.find("language_model.model.layers.") == 0 &&
      (key.find(".attention.wqkv.weight") != std::string::npos || key.find(".attention.wo.weight") != std::string::npos ||
       key.find(".feed_forward.w2.weight") != std::string::npos))
    c->llm_lin_dirty = true;
  return 0;
}

int aigv_finalize_weights(aigv_ctx* c) {
  if (!c) return fail(c, AIGV_ERR_ARG, "null ctx");
  HIPCHK(c, hipSetDevice(c->device));
  // The e4m3 copies follow the bf16 InternLM2 linears: they are dropped (and the context returns to bf16) only when one of those was
  // reloaded since they were made.  Any other reload - rotary tables after a capacity change, a new score head - keeps them and the mode.
  const bool keep_fp8 = !c->llm8.empty() && !c->llm_lin_dirty && c->q8 != nullptr;
  if (!c->llm8.empty() && !keep_fp8) {   // weights were (re)loaded: the e4m3 copies are stale - drop them; aigv_set_precision quantises again
    HIPCHK(c, hipDeviceSynchronize());
    for (auto& q : c->llm8)
      for (void* p : {(void*)q.wqkv, (void*)q.wo, (void*)q.w13, (void*)q.w2, (void*)q.s_wqkv, (void*)q.s_wo, (void*)q.s_w13, (void*)q.s_w2}) drop_alloc(c, p);
    drop_alloc(c, c->q8); drop_alloc(c, c->q8_scale);
    c->q8 = nullptr; c->q8_scale = nullptr;
    c->llm8.clear();
  }
  if (!keep_fp8) c->fp8_llm = false;
  c->llm_lin_dirty = false;
  const aigv_config& k = c->cfg;
  const size_t Hv = k.vit_hidden, Iv = k.vit_inter, H = k.llm_hidden, I = k.llm_inter;
  const std::string e = "vision_model.embeddings.";
  TRY(need(c, e + "patch_embedding.weight", Hv * c->Kp, &c->patch_w));
  TRY(need(c, e + "patch_embedding.bias", Hv, &c->patch_b));
  TRY(need(c, e + "position_embedding", (size_t)c->S * Hv, &c->pos));
  const bf16_t* cls = nullptr;
  TRY(need(c, e + "class_embedding", Hv, &cls));
  {  // class token row = bf16(cls + pos[0])  (modeling_intern_vit.py:100-106)
    std::vector<uint16_t> a(Hv), b(Hv), o(Hv);
    HIPCHK(c, hipMemcpy(a.data(), cls, Hv * 2, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(b.data(), c->pos, Hv * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < Hv; ++i) o[i] = f32_to_bf16_host(bf16_to_f32_host(a[i]) + bf16_to_f32_host(b[i]));
    const int64_t shp[1] = {(int64_t)Hv};
    TRY(aigv_load_weight(c, "derived.cls_pos", o.data(), shp, 1, AIGV_BF16, 0));
    TRY(need(c, "derived.cls_pos", Hv, &c->cls_pos));
  }
  c->vit.assign(k.vit_layers, VitLayer{});
  for (int i = 0; i < k.vit_layers; ++i) {
    const std::string p = "vision_model.encoder.layers." + std::to_string(i) + ".";
    VitLayer& L = c->vit[i];
    TRY(need(c, p + "ls1", Hv, &L.ls1));
    TRY(need(c, p + "ls2", Hv, &L.ls2));
    TRY(need(c, p + "attn.qkv.weight", 3 * Hv * Hv, &L.qkv_w));
    if (k.vit_qkv_bias) TRY(need(c, p + "attn.qkv.bias", 3 * Hv, &L.qkv_b));
    if (k.vit_qk_norm) {
      TRY(need(c, p + "attn.q_norm.weight", Hv, &L.qn));
      TRY(need(c, p + "attn.k_norm.weight", Hv, &L.kn));
    }
    TRY(need(c, p + "attn.proj.weight", Hv * Hv, &L.proj_w));
    TRY(need(c, p + "attn.proj.bias", Hv, &L.proj_b));
    TRY(need(c, p + "mlp.fc1.weight", Iv * Hv, &L.fc1_w));
    TRY(need(c, p + "mlp.fc1.bias", Iv, &L.fc1_b));
    TRY(need(c, p + "mlp.fc2.weight", Hv * Iv, &L.fc2_w));
    TRY(need(c, p + "mlp.fc2.bias", Hv, &L.fc2_b));
    TRY(need(c, p + "norm1.weight", Hv, &L.n1w));
    TRY(need(c, p + "norm2.weight", Hv, &L.n2w));
    if (!k.vit_norm_rms) {
      TRY(need(c, p + "norm1.bias", Hv, &L.n1b));
      TRY(need(c, p + "norm2.bias", Hv, &L.n2b));
    }
  }
  TRY(need(c, "language_model.model.tok_embeddings.weight", (size_t)k.vocab * H, &c->tok_emb));
  TRY(need(c, "language_model.model.norm.weight", H, &c->final_norm));
  TRY(need(c, "language_model.output.weight", (size_t)k.vocab * H, &c->lm_head));
  TRY(need(c, "rope.cos", (size_t)k.max_positions * c->head_dim / 2, &c->rope_cos));
  TRY(need(c, "rope.sin", (size_t)k.max_positions * c->head_dim / 2, &c->rope_sin));
  c->llm.assign(k.llm_layers, LlmLayer{});
  for (int i = 0; i < k.llm_layers; ++i) {
    const std::string p = "language_model.model.layers." + std::to_string(i) + ".";
    LlmLayer& L = c->llm[i];
    TRY(need(c, p + "attention.wqkv.weight", (size_t)c->qkv_out * H, &L.wqkv));
    TRY(need(c, p + "attention.wo.weight", H * H, &L.wo));
    if (!c->w.count(p + "feed_forward.w1.weight#seen") || !c->w.count(p + "feed_forward.w3.weight#seen"))
      return fail(c, AIGV_ERR_STATE, "layer %d: feed_forward.w1/w3 were not both loaded", i);
    TRY(need(c, p + "feed_forward.w13.weight", 2 * I * H, &L.w13));
    TRY(need(c, p + "feed_forward.w2.weight", H * I, &L.w2));
    TRY(need(c, p + "attention_norm.weight", H, &L.an));
    TRY(need(c, p + "ffn_norm.weight", H, &L.fn));
  }
  const char* pn[2] = {"mlp1", "motion_mlp"};
  const size_t pin[2] = {(size_t)c->proj_in, (size_t)k.motion_dim};
  for (int j = 0; j < 2; ++j) {
    const std::string p = std::string(pn[j]) + ".";
    TRY(need(c, p + "0.weight", pin[j], &c->p_ln_w[j]));
    TRY(need(c, p + "0.bias", pin[j], &c->p_ln_b[j]));
    TRY(need(c, p + "1.weight", H * pin[j], &c->p_w1[j]));
    TRY(need(c, p + "1.bias", H, &c->p_b1[j]));
    TRY(need(c, p + "3.weight", H * H, &c->p_w2[j]));
    TRY(need(c, p + "3.bias", H, &c->p_b2[j]));
  }
  c->score = ScoreHeadArgs{};
  c->score.n_layers = k.n_score_layers;
  c->score.dims[0] = (int)H;
  for (int j = 0; j < k.n_score_layers; ++j) {
    c->score.dims[j + 1] = k.score_dims[j];
    const std::string p = "mlpscore.fc" + std::to_string(j + 1) + ".";
    TRY(need(c, p + "weight", (size_t)c->score.dims[j + 1] * c->score.dims[j], &c->score.w[j]));
    TRY(need(c, p + "bias", (size_t)c->score.dims[j + 1], &c->score.b[j]));
  }
  c->finalized = true;
  return 0;
}

int aigv_set_precision(aigv_ctx* c, int mode) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_set_precision: null context");
  if (mode != AIGV_PRECISION_BF16 && mode != AIGV_PRECISION_FP8_LLM) return fail(c, AIGV_ERR_ARG, "aigv_set_precision: unknown mode %d", mode);
  if (mode == AIGV_PRECISION_BF16) { c->fp8_llm = false; return 0; }
  if (c->llm.empty()) return fail(c, AIGV_ERR_STATE, "aigv_set_precision: call aigv_finalize_weights first");
  const aigv_config& k = c->cfg;
  const int H = k.llm_hidden, I = k.llm_inter, Q = c->qkv_out;
  if (H % 256 || Q % 256 || (2 * I) % 256 || H % 128 || I % 128)
    return fail(c, AIGV_ERR_ARG, "aigv_set_precision: the fp8 kernel needs output widths in multiples of 256 and depths in multiples of 128 (H=%d I=%d qkv=%d)", H, I, Q);
  HIPCHK(c, hipSetDevice(c->device));
  if (c->llm8.empty()) {   // quantise once: one row of W[N, K] = one output channel
    std::vector<LlmLayerFp8> q(k.llm_layers);
    TRY(dalloc(c, &c->q8, (size_t)k.max_tokens * (size_t)std::max(H, I)));
    TRY(dalloc(c, &c->q8_scale, (size_t)k.max_tokens));
    for (int li = 0; li < k.llm_layers; ++li) {
      const LlmLayer& L = c->llm[li];
      struct { const bf16_t* w; int n, kk; uint8_t** q; float** sc; } items[4] = {
          {L.wqkv, Q, H, &q[li].wqkv, &q[li].s_wqkv}, {L.wo, H, H, &q[li].wo, &q[li].s_wo},
          {L.w13, 2 * I, H, &q[li].w13, &q[li].s_w13}, {L.w2, H, I, &q[li].w2, &q[li].s_w2}};
      for (auto& it : items) {
        TRY(dalloc(c, it.q, (size_t)it.n * it.kk));
        TRY(dalloc(c, it.sc, (size_t)it.n));
        hipError_t e = aigv_launch_quant_fp8_rows(it.w, it.kk, it.n, it.kk, *it.q, it.kk, *it.sc, nullptr);
        if (e != hipSuccess) return fail(c, AIGV_ERR_HIP, "weight quantisation failed: %s", hipGetErrorString(e));
      }
    }
    HIPCHK(c, hipDeviceSynchronize());
    c->llm8 = std::move(q);
  }
  c->fp8_llm = true;
  return 0;
}

}  // extern "C"
