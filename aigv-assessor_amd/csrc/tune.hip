// The tuning knobs of the C ABI (include/aigv_amd.h: tests and experiments only) as one table, the per-context mode setters and the
// profiler read-out.  Host-side C++ only.
#include "ctx.h"

using namespace aigv;

namespace {

constexpr bool in_waves(int v) { return v == 0 || v == 4 || v == 8; }
constexpr bool in_forms(int v) { return v == 0 || v == 1 || v == 2 || v == 4; }
constexpr bool in_forms_packed(int v) { return in_forms(v) || (v >= 1000 && v < 1000 + 4096); }   // 1000 + 3 bits per decode GEMV
constexpr bool in_kmax(int v) { return v >= 0 && v <= 65536 && v % 64 == 0; }

// One row per AIGV_TUNE_* knob, in the enum's order (what the values mean: the enum's comments).  A value is valid if it is in 0..hi or,
// for the knobs whose values are a set, if `in_set` says so; aigv_ctx_tune takes -1 (follow the process default) besides.
struct Knob {
  int def;                // library default
  int hi;
  bool (*in_set)(int);
  bool process_default;   // aigv_tune_default sets it (the others: aigv_tune_gemm / _attention / _skinny)
};
constexpr Knob KNOBS[AIGV_TUNE_COUNT] = {
    {0, 4, nullptr, false},              // GEMM_MODE
    {0, 15, nullptr, false},             // GEMM256_ORDER
    {0, 7, nullptr, false},              // GEMM256_VARIANT
    {0, 0, in_waves, false},             // ATTN_WAVES
    {0, 0, in_forms_packed, false},      // SKINNY_P
    {0, 2, nullptr, false},              // BODY_TILE
    {0, 0, in_kmax, true},               // CO_KMAX: 0 = the co-resident kernel is never chosen (measured: profiles/r5_gemmco.txt)
    {0, 16, nullptr, true},              // TAIL_SLICES
    {0, 1, nullptr, true},               // ATTN_LEAD_KEY
    {1, 1, nullptr, false},              // DECODE_FUSED
    {1, 1, nullptr, false},              // DECODE_FP8
    {0, 0, in_forms, false},             // SKINNY_P8
    {0, 2, nullptr, true},               // FUSE_TAILS
    {1, 4, nullptr, true},               // LONE_BODY: never (no in-step gain measured)
};
static_assert(AIGV_TUNE_GEMM_MODE == 0 && AIGV_TUNE_CO_KMAX == 6 && AIGV_TUNE_LONE_BODY == 13 && AIGV_TUNE_COUNT == 14, "KNOBS follows the enum's order");

constexpr Tune library_defaults() {
  Tune t{};
  for (int k = 0; k < AIGV_TUNE_COUNT; ++k) t.v[k] = KNOBS[k].def;
  return t;
}

bool known(int knob) { return knob >= 0 && knob < AIGV_TUNE_COUNT; }
bool valid(int knob, int value) { return KNOBS[knob].in_set ? KNOBS[knob].in_set(value) : value >= 0 && value <= KNOBS[knob].hi; }

}  // namespace

Tune aigv::g_tune = library_defaults();

extern "C" {

int aigv_set_row_trimming(aigv_ctx* c, int on) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_set_row_trimming: null context");
  c->trim_last_layer = on != 0;
  return 0;
}

int aigv_get_attention_numerics(const aigv_ctx* c) { return c ? c->attn_round_scores : AIGV_ATTENTION_NUMERICS_DEFAULT; }

int aigv_set_attention_numerics(aigv_ctx* c, int mode) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_set_attention_numerics: null context");
  if (mode != 0 && mode != 1) return fail(c, AIGV_ERR_ARG, "aigv_set_attention_numerics: 0 (fp32 scores) or 1 (the reference's bf16 score matrix)");
  c->attn_round_scores = mode;
  return 0;
}

int aigv_set_gemm_mode(aigv_ctx* c, int mode) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_set_gemm_mode: null context");
  if (mode != -1 && !valid(AIGV_TUNE_GEMM_MODE, mode)) return fail(c, AIGV_ERR_ARG, "aigv_set_gemm_mode: mode must be -1 (process default), 0 (row plans), 1 (128 tile), 2 (256 tile), 3 (batch-level dispatch) or 4 (co-resident 256x128 tile)");
  c->tune[AIGV_TUNE_GEMM_MODE] = mode;
  return 0;
}

int aigv_ctx_tune(aigv_ctx* c, int knob, int value) {
  if (!c) return fail(c, AIGV_ERR_ARG, "aigv_ctx_tune: null context");
  if (knob == AIGV_TUNE_GEMM_MODE) return aigv_set_gemm_mode(c, value);
  if (!known(knob)) return fail(c, AIGV_ERR_ARG, "aigv_ctx_tune: unknown knob %d", knob);
  if (value != -1 && !valid(knob, value)) return fail(c, AIGV_ERR_ARG, "aigv_ctx_tune: value %d out of range for knob %d", value, knob);
  c->tune[knob] = value;
  return 0;
}

// process default of a context-only knob (the context-free aigv_op_* entry points and contexts that left it at -1 follow it): tests and A/B scripts
int aigv_tune_default(int knob, int value) {
  if (knob == AIGV_TUNE_CO_KMAX) return aigv_tune_co_gemm(value);
  if (!known(knob) || !KNOBS[knob].process_default)
    return fail(nullptr, AIGV_ERR_ARG, "aigv_tune_default: knob %d has no process default here (aigv_tune_gemm / _attention / _skinny set the others)", knob);
  if (!valid(knob, value)) return fail(nullptr, AIGV_ERR_ARG, "aigv_tune_default: value %d out of range for knob %d", value, knob);
  g_tune.v[knob] = value;
  return 0;
}

int aigv_tune_co_gemm(int kmax) {
  if (!valid(AIGV_TUNE_CO_KMAX, kmax)) return fail(nullptr, AIGV_ERR_ARG, "aigv_tune_co_gemm: K threshold must be 0 (off) or a multiple of 64");
  g_tune.v[AIGV_TUNE_CO_KMAX] = kmax;
  return 0;
}

int aigv_tune_skinny(int p) {   // (one form for all four decode GEMVs: the packed per-GEMV words are aigv_ctx_tune's)
  if (!in_forms(p)) return fail(nullptr, AIGV_ERR_ARG, "aigv_tune_skinny: 0 (default), 1, 2 or 4, got %d", p);
  g_tune.v[AIGV_TUNE_SKINNY_P] = p;
  return 0;
}

int aigv_tune_attention(int waves) {
  if (!valid(AIGV_TUNE_ATTN_WAVES, waves))
    return fail(nullptr, AIGV_ERR_ARG, "aigv_tune_attention: 0 (default), 4 or 8 waves per workgroup, got %d", waves);
  g_tune.v[AIGV_TUNE_ATTN_WAVES] = waves;
  return 0;
}

int aigv_tune_gemm(int mode, double rate256) {
  // mode = kernel choice (0 auto, 1 128-tile, 2 256-tile) + 16 * (256-kernel schedule variant 0..3, experiments)
  // mode bits 4..6: 0 = keep the default schedule, 1 + v = select 256-kernel schedule variant v (0..3)
  // bits 10..13: tile order of the 256 kernel for every shape (default 0: by weight size, gemm256.hip): 1 = row groups, 1 + g = groups of g column tiles
  // bits 14..15: tile kernel of a row plan's body: 0 by fill (default), 1 = 256 tiles, 2 = 128 tiles
  // (the body tile and the tile order are written BEFORE the mode word is validated: a refused call still changes them.  Kept as it always was.)
  g_tune.v[AIGV_TUNE_BODY_TILE] = (mode >> 14) & 3;
  g_tune.v[AIGV_TUNE_GEMM256_ORDER] = (mode >> 10) & 15;
  mode &= 1023;
  const int vsel = mode >> 4;
  mode &= 15;
  if (!valid(AIGV_TUNE_GEMM_MODE, mode) || !valid(AIGV_TUNE_GEMM256_VARIANT, vsel))
    return fail(nullptr, AIGV_ERR_ARG, "aigv_tune_gemm: mode must be 0 (auto), 1 (128 tile), 2 (256 tile), 3 (batch-level dispatch in the scoring pass) or 4 (co-resident 256x128 tile)");
  if (vsel > 0) g_tune.v[AIGV_TUNE_GEMM256_VARIANT] = vsel;
  g_tune.v[AIGV_TUNE_GEMM_MODE] = mode;
  if (rate256 > 0) g_rate256 = rate256;
  return 0;
}

int aigv_prof_enable(aigv_ctx* c, int on) {
  if (!c) return fail(c, AIGV_ERR_ARG, "null ctx");
  c->prof = on != 0;
  return 0;
}

int aigv_prof_read(aigv_ctx* c, int cls, int64_t* launches, double* total_ms, double* flops, double* bytes) {
  if (!c || cls < 0 || cls >= AIGV_PROF_COUNT) return fail(c, AIGV_ERR_ARG, "aigv_prof_read: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int64_t n = 0;
  double ms = 0, fl = 0, by = 0;
  std::vector<ProfRec> keep;
  for (auto& r : c->recs) {
    if (r.cls != cls) { keep.push_back(r); continue; }
    HIPCHK(c, hipEventSynchronize(r.b));
    float t = 0;
    HIPCHK(c, hipEventElapsedTime(&t, r.a, r.b));
    ms += t; fl += r.flops; by += r.bytes; ++n;
    c->ev_pool.push_back(r.a);
    c->ev_pool.push_back(r.b);
  }
  c->recs.swap(keep);
  if (launches) *launches = n;
  if (total_ms) *total_ms = ms;
  if (flops) *flops = fl;
  if (bytes) *bytes = by;
  return 0;
}

}  // extern "C"
