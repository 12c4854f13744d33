// The GEMM dispatcher of the C ABI: which tile kernel (gemm.hip / gemm256.hip / gemmco.hip / head.hip) runs which rows of a GEMM - the
// wave-quantisation cost model of the batch-level dispatch, the per-sequence row plans of the scoring pass, split-K scratch.  Host-side
// C++ only.  Interface: ctx.h.
#include <atomic>
#include <mutex>

#include "ctx.h"

namespace aigv {

// ---- GEMM dispatch: split the rows over the tile kernels by a wave-quantisation cost model -----------------------
// (gemm_mode 0 = row plans in the scoring pass / cost model at op level, 1 / 2 / 4 = one tile kernel, 3 = batch-level cost model: aigv_amd.h)
static GemmArgs tuned(const aigv_ctx* c, const GemmArgs& a) {
  GemmArgs b = a;
  b.order_sel = tune_knob(c, AIGV_TUNE_GEMM256_ORDER); b.variant_sel = tune_knob(c, AIGV_TUNE_GEMM256_VARIANT);
  return b;
}
// Model constants, microseconds on one MI355X (scripts/gemm_overhead.py: time vs K at fixed M, N):
//   a full round of the 256 kernel (256 tiles, one per CU) takes nk * kt256 + fix256; a full round of the 128 kernel
//   (512 tiles, two co-resident workgroups per CU) nk * KT128 + FIX128, a last round of <= 256 tiles LONE128 of that.
double g_rate256 = 1.46;                 // throughput of the 256 kernel relative to the 128 kernel: kt256 = 2 * KT128 / rate
constexpr double KT128 = 0.95, FIX128 = 6.0, LONE128 = 0.70, FIX256 = 9.0, LAUNCH_GAP = 2.0;

// Which launches the dispatcher has made since the record was last cleared (aigv_gemm_route: AIGV_ROUTE_* bits, one per kind of launch).
// Written where the launch is issued, so a test that forces a route reads back the route that RAN, not a restatement of the conditions.
static std::atomic<unsigned> g_route{0};
static inline void took(unsigned bit) { g_route.fetch_or(bit, std::memory_order_relaxed); }

static double kt256() { return 2.0 * KT128 / g_rate256; }

static double t256(long row_tiles, int N, int nk) {
  if (row_tiles <= 0) return 0;
  const long tiles = row_tiles * (N / 256);
  return (double)((tiles + 255) / 256) * (nk * kt256() + FIX256);
}
static double t128_blocks(long blocks, double nk_each) {
  const double rt = nk_each * KT128 + FIX128;
  const long full = blocks / 512, part = blocks % 512;
  return full * rt + (part == 0 ? 0.0 : part <= 256 ? LONE128 * rt : rt);
}
static double t128(int rows, int N, int nk) { return rows <= 0 ? 0 : t128_blocks((long)((rows + 127) / 128) * (N / 128), nk); }
// slabs read once + the bf16 result (and residual) at ~3 TB/s, plus the launch
static double t_finalize(long rows, int N, int S) { return (double)rows * N * (4.0 * S + 4.0) / 3.0e6 + 3.0; }

// fp32 scratch for split-K slices.  A context owns its own (allocated at aigv_ctx_create on the context's device, SPLITK_MAX_FLOATS:
// the planner never asks for more).  The context-free single-operator entry points (aigv_op_gemm: tests, benches) use one scratch
// per DEVICE, created on first use under a lock and kept for the process lifetime - never freed or regrown, so no launch ever
// waits on a device synchronisation, and a second device never sees memory of the first.
constexpr int MAX_DEVICES = 64;
static float* g_op_splitk_ws[MAX_DEVICES] = {};
static std::mutex g_op_splitk_lock;

int splitk_scratch(aigv_ctx* c, size_t need_floats, float** out) {
  if (need_floats > SPLITK_MAX_FLOATS) return fail(c, AIGV_ERR_ARG, "split-K scratch: %zu floats exceed the planner's cap", need_floats);
  if (c) {
    if (need_floats > c->splitk_floats) return fail(c, AIGV_ERR_STATE, "split-K scratch: %zu floats exceed the context's %zu", need_floats, c->splitk_floats);
    *out = c->on_vit_front ? c->splitk_ws_vit : c->splitk_ws;
    return 0;
  }
  int dev = 0;
  HIPCHK(c, hipGetDevice(&dev));
  if (dev < 0 || dev >= MAX_DEVICES) return fail(c, AIGV_ERR_ARG, "device %d out of range", dev);
  std::lock_guard<std::mutex> g(g_op_splitk_lock);
  if (!g_op_splitk_ws[dev]) HIPCHK(c, hipMalloc((void**)&g_op_splitk_ws[dev], SPLITK_MAX_FLOATS * sizeof(float)));
  *out = g_op_splitk_ws[dev];
  return 0;
}
constexpr int SPLITS[] = {2, 3, 4, 6, 8};

// rows that do not fill whole rounds are latency-bound on their K loop: split K over S workgroups per tile (fp32 slabs +
// a fixed-order finalize pass).  Best S for the 128 kernel / for `row_tiles` x 256 rows on the 256 kernel; S = 1: no split.
static double best_split128(int rows, int N, int nk, int epi, int* S_out) {
  *S_out = 1;
  double best = t128(rows, N, nk);
  if (epi == EPI_PATCH) return best;
  const long tiles = (long)((rows + 127) / 128) * (N / 128);
  for (int S : SPLITS) {
    if (nk % S || nk / S < 4 || (size_t)S * rows * N > SPLITK_MAX_FLOATS) continue;
    const double t = t128_blocks(tiles * S, (double)nk / S) + t_finalize(rows, N, S) + LAUNCH_GAP;
    if (t < best) { best = t; *S_out = S; }
  }
  return best;
}
static double best_split256(long row_tiles, int N, int nk, int* S_out) {
  *S_out = 0;
  double best = 1e30;
  for (int S : SPLITS) {
    if (nk % S || nk / S < 4 || (size_t)S * row_tiles * 256 * N > SPLITK_MAX_FLOATS) continue;
    const long blocks = row_tiles * (N / 256) * S;
    const double t = (double)((blocks + 255) / 256) * ((double)nk / S * kt256() + FIX256) + t_finalize(row_tiles * 256, N, S) + LAUNCH_GAP;
    if (t < best) { best = t; *S_out = S; }
  }
  return best;
}

static int skinny_epi(int epi) {   // GEMM epilogue -> skinny-kernel epilogue (same rounding points); -1 if none
  switch (epi) {
    case EPI_STORE: return SK_STORE;
    case EPI_GELU: return SK_GELU;
    case EPI_LS_RESID: return SK_LS_RESID;
    case EPI_RESID: return SK_RESID;
    case EPI_SWIGLU: return SK_SWIGLU;
  }
  return -1;
}
// a <= 64-row remainder streamed through the skinny kernel costs ~ the weight bytes at HBM rate
static double t_skinny(int rows, int N, int K) {
  if (rows <= 0) return 0;
  if (rows > 64 || K % 128) return 1e30;
  return (double)N * K * 2.0 / 4.5e6 + 4.0;
}

// profile record of a GEMM launch that really computes `rows` rows of `a`
#define GEMM_PROF_ROWS(c, a, rows, s) ProfScope ps(c, (c) ? (c)->gemm_cls : AIGV_PROF_GEMM, 2.0 * (rows) * (double)(a).N * (a).K, \
                                                   2.0 * ((double)(rows) * (a).K + (double)(a).N * (a).K + (double)(rows) * (a).N), s)
#define GEMM_PROF(c, a, s) GEMM_PROF_ROWS(c, a, (a).M, s)

int launch_one(aigv_ctx* c, const GemmArgs& a, int epi, bool use256, hipStream_t s) {
  GEMM_PROF(c, a, s);
  took(use256 ? AIGV_ROUTE_256 : AIGV_ROUTE_128);
  HIPCHK(c, use256 ? aigv_launch_gemm256(tuned(c, a), epi, s) : aigv_launch_gemm(a, epi, s));
  return 0;
}

// the co-resident 256x128 kernel (gemmco.hip): every row in full K, ragged row counts and half-tile tables included
static int launch_co(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s) {
  GEMM_PROF(c, a, s);
  took(AIGV_ROUTE_CO);
  HIPCHK(c, aigv_launch_gemmco(tuned(c, a), epi, s));
  return 0;
}
// does this GEMM run on the co-resident kernel?  A function of the mode and of K only.
static bool use_co(const aigv_ctx* c, const GemmArgs& a, int mode) {
  if (!aigv_gemmco_supported(a)) return false;
  return mode == 4 || ((mode == 0 || mode == 3) && a.K <= tune_knob(c, AIGV_TUNE_CO_KMAX));
}

static int launch_splitk(aigv_ctx* c, const GemmArgs& a, int epi, int S, bool tile256, hipStream_t s) {
  float* ws = nullptr;
  TRY(splitk_scratch(c, (size_t)S * a.M * a.N, &ws));
  GEMM_PROF(c, a, s);
  took(tile256 ? AIGV_ROUTE_SPLITK_256 : AIGV_ROUTE_SPLITK_128);
  HIPCHK(c, aigv_launch_gemm_splitk(tuned(c, a), epi, S, ws, s, tile256));
  return 0;
}

static GemmArgs row_slice(const GemmArgs& a, int row0, int rows) {
  GemmArgs b = a;
  b.M = rows;
  b.A = a.A + (size_t)row0 * a.lda;
  b.C = a.C + (size_t)row0 * a.ldc;
  if (a.resid) b.resid = a.resid + (size_t)row0 * a.ldr;
  return b;
}

// Rows are independent, so the GEMM is cut into up to three row bands, each on the kernel that wastes least:
//   top:  R x 256 rows on the 256x256 kernel, R chosen so that it runs whole rounds
//   mid:  Q x 256 rows on the 256x256 kernel with split-K (a partial round made of K slices)
//   last: the remaining rows on the weight-streaming skinny kernel (<= 64 rows) or the 128x128 kernel (plain or split-K)
struct GemmPlan {
  int top_tiles = 0;      // R; -1: the whole problem (ragged last tile included) in one launch of the 256 kernel
  int mid_tiles = 0;      // Q
  int mid_slices = 0;     // split-K factor of the mid band
  int last_rows = 0;
  int last_kind = 0;      // 0 none, 1 skinny, 2 the 128 kernel
  int last_slices = 1;    // split-K factor of the last band on the 128 kernel (1: plain)
  double est_us = 0;
};

static GemmPlan plan_gemm(int M, int N, int K, int epi, int mode) {
  GemmPlan pl;
  const int nk = K / 64, sk = skinny_epi(epi);
  const bool ok256 = (N % 256 == 0);
  if (mode == 1 || !ok256) { pl.last_rows = M; pl.last_kind = 2; pl.est_us = t128(M, N, nk); return pl; }
  pl.top_tiles = -1;
  pl.est_us = t256((M + 255) / 256, N, nk);
  if (mode == 2) return pl;
  if (epi == EPI_PATCH) {
    if (t128(M, N, nk) < pl.est_us) { pl = GemmPlan(); pl.last_rows = M; pl.last_kind = 2; pl.est_us = t128(M, N, nk); }
    return pl;
  }
  const int full_tiles = M / 256;
  for (int R = 0; R <= full_tiles; ++R) {
    for (int Q = 0; Q <= 8 && R + Q <= full_tiles; ++Q) {
      const int rem = M - (R + Q) * 256;
      int S256 = 0, S128 = 1, last = 0;
      double t = t256(R, N, nk);
      if (Q > 0) {
        const double tm = best_split256(Q, N, nk, &S256);
        if (!S256) continue;
        t += tm;
      }
      if (rem > 0) {
        const double tk = best_split128(rem, N, nk, epi, &S128);
        const double ts = sk >= 0 ? t_skinny(rem, N, K) : 1e30;
        last = ts < tk ? 1 : 2;
        if (last == 1) S128 = 1;
        t += ts < tk ? ts : tk;
      }
      t += LAUNCH_GAP * ((R > 0) + (Q > 0) + (rem > 0) - 1);
      if (t < pl.est_us) {
        pl.est_us = t; pl.top_tiles = R; pl.mid_tiles = Q; pl.mid_slices = S256; pl.last_rows = rem; pl.last_kind = last;
        pl.last_slices = S128;
      }
    }
  }
  return pl;
}

// Columns are independent too: N = 256 j + 128 (InternViT-6B: 3200, 9600) would put the whole GEMM on the 128 kernel; instead the
// first 256 j columns take the row-band plan and only the last 128 columns run on the 128 kernel.
static int split_columns(int M, int N, int K, int epi, int mode) {   // width of the right-hand 128-kernel band, 0 = no column split
  if (mode != 0 || N % 256 != 128 || N < 384 || epi == EPI_PATCH || epi == EPI_SWIGLU) return 0;
  const int nk = K / 64;
  const double whole = t128(M, N, nk);
  const double split = plan_gemm(M, N - 128, K, epi, mode).est_us + t128(M, 128, nk) + LAUNCH_GAP;
  return split < whole ? 128 : 0;
}

static GemmArgs col_slice(const GemmArgs& a, int n0, int n) {
  GemmArgs b = a;
  b.N = n;
  b.W = a.W + (size_t)n0 * a.ldw;
  b.C = a.C + n0;
  if (a.bias) b.bias = a.bias + n0;
  if (a.ls) b.ls = a.ls + n0;
  if (a.resid) b.resid = a.resid + n0;
  return b;
}

int run_gemm(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s) {
  if (const char* m = aigv_gemm_check(a, epi)) return fail(c, AIGV_ERR_ARG, "%s (M=%d N=%d K=%d epi=%d)", m, a.M, a.N, a.K, epi);
  if (use_co(c, a, resolved_gemm_mode(c))) return launch_co(c, a, epi, s);
  const int mode = resolved_gemm_mode(c) == 3 || resolved_gemm_mode(c) == 4 ? 0 : resolved_gemm_mode(c);
  if (const int right = split_columns(a.M, a.N, a.K, epi, mode)) {
    took(AIGV_ROUTE_COLUMN_BAND);
    TRY(run_gemm(c, col_slice(a, 0, a.N - right), epi, s));
    return launch_one(c, col_slice(a, a.N - right, right), epi, false, s);
  }
  const GemmPlan pl = plan_gemm(a.M, a.N, a.K, epi, mode);
  if (pl.top_tiles < 0) return launch_one(c, a, epi, true, s);
  int row = 0;
  if (pl.top_tiles > 0) {
    TRY(launch_one(c, row_slice(a, 0, pl.top_tiles * 256), epi, true, s));
    row = pl.top_tiles * 256;
  }
  if (pl.mid_tiles > 0) {
    TRY(launch_splitk(c, row_slice(a, row, pl.mid_tiles * 256), epi, pl.mid_slices, true, s));
    row += pl.mid_tiles * 256;
  }
  if (row < a.M) {
    const GemmArgs bot = row_slice(a, row, a.M - row);
    if (pl.last_kind == 1) {
      const int sk = skinny_epi(epi);
      ProfScope ps(c, c ? c->gemm_cls : AIGV_PROF_GEMM, 2.0 * bot.M * (double)a.N * a.K, 2.0 * (double)a.N * a.K, s);
      took(AIGV_ROUTE_SKINNY);
      hipError_t e = aigv_launch_skinny_gemm(bot.A, bot.lda, bot.M, bot.W, bot.ldw, bot.N, bot.K, bot.bias, bot.resid, bot.ldr,
                                            bot.C, bot.ldc, sk, s, bot.ls);
      if (e != hipSuccess) return fail(c, AIGV_ERR_HIP, "skinny remainder (M=%d N=%d K=%d): %s", bot.M, bot.N, bot.K, hipGetErrorString(e));
      return 0;
    }
    if (pl.last_slices > 1) return launch_splitk(c, bot, epi, pl.last_slices, false, s);
    return launch_one(c, bot, epi, false, s);
  }
  return 0;
}

// ---- per-sequence row plans (struct RowPlan above) ------------------------------------------------------------------------------------
constexpr int TINY_TAIL = 4;

// cu[0..n_seq]: row offsets of the sequences inside the activation matrices.  Builds the plan and uploads its table (kernel-argument
// writes on `s`: no host synchronisation).  The table is written by EVERY pass, never skipped for a plan "already on the device": a pass
// captured into a HIP graph must carry its own table writes (a replay after a pass of another shape would otherwise run on that pass's table),
// and a replayed graph rewrites the device table behind the host's back - so there is no host-side notion of what the device table holds.
int build_row_plan(aigv_ctx* c, RowPlan& rp, const int32_t* cu, int n_seq, hipStream_t s) {
  rp.tiny.clear();
  std::vector<int32_t> body, tail;
  bool uniform = true;
  for (int b = 1; b < n_seq; ++b) uniform = uniform && (cu[b + 1] - cu[b] == cu[1] - cu[0]);
  rp.tail_rows = 0;
  for (int b = 0; b < n_seq; ++b) {
    const int L = cu[b + 1] - cu[b], nb = L / 256, rem = L % 256, r0 = cu[b] + nb * 256;
    for (int j = 0; j < 2 * nb; ++j) { body.push_back(cu[b] + j * 128); body.push_back(128); }
    if (rem == 0) continue;
    if (rem <= TINY_TAIL) {
      if (!uniform) rp.tiny.push_back({r0, 1, rem});
      else if (b == 0)
        for (int j = 0; j < rem; ++j) rp.tiny.push_back({r0 + j, L, n_seq});
      continue;
    }
    tail.push_back(r0); tail.push_back(std::min(rem, 128));
    if (rem > 128) { tail.push_back(r0 + 128); tail.push_back(rem - 128); }
    rp.tail_rows += rem;
  }
  rp.body_halves = (int)body.size() / 2;
  rp.tail_halves = (int)tail.size() / 2;
  rp.rows = cu[n_seq];
  if (rp.body_halves + rp.tail_halves > rp.cap_halves)
    return fail(c, AIGV_ERR_STATE, "row plan: %d half tiles exceed the table's %d", rp.body_halves + rp.tail_halves, rp.cap_halves);
  body.insert(body.end(), tail.begin(), tail.end());
  if (!body.empty()) HIPCHK(c, aigv_launch_write_ints(body.data(), (int)body.size(), rp.d_tab, s));
  return 0;
}

// Split-K factor of the TAIL half tiles of a GEMM: a function of (N, K) only - never of the batch or of the number of clips: the largest
// S in {2, 4, 8} that leaves every slice >= 8 K-tiles and keeps ONE tail row tile's slices (N / 256 x S workgroups) within half a round of
// the chip (two tail row tiles - four clips' 128-row remainders - then come to about one round; eight clips to two).  1 = the tail rides in
// the body's launch.  `forced` > 0 (AIGV_TUNE_TAIL_SLICES, experiments): one factor for every shape it divides.
static int tail_slices(int N, int K, int forced) {
  const int tn = N / 256, nk = K / 64;
  int best = 1;
  for (int S : {2, 4, 8})
    if (nk % S == 0 && nk / S >= 8 && 2 * tn * S <= 256) best = S;
  if (forced == 1 || (forced > 1 && nk % forced == 0 && nk / forced >= 4)) best = forced;
  return best;
}

static int launch_tab(aigv_ctx* c, const GemmArgs& a, int epi, const int32_t* tab, int halves, int rows, int S, hipStream_t s) {
  if (halves <= 0) return 0;
  GemmArgs b = tuned(c, a);
  b.row_tab = tab; b.tab_halves = halves;
  GEMM_PROF_ROWS(c, a, rows, s);
  if (S <= 1) {
    took(AIGV_ROUTE_TAB_256);
    HIPCHK(c, aigv_launch_gemm256(b, epi, s));
    return 0;
  }
  float* ws = nullptr;
  TRY(splitk_scratch(c, (size_t)S * ((halves + 1) / 2) * 256 * a.N, &ws));
  took(AIGV_ROUTE_TAB_SPLITK);
  HIPCHK(c, aigv_launch_gemm_splitk(b, epi, S, ws, s, true));
  return 0;
}

// tails of <= TINY_TAIL rows (InternViT: 1025 = 4 * 256 + 1) on the weight-streaming skinny kernel in its fixed 4-slice form
static int run_tiny_tails(aigv_ctx* c, const GemmArgs& a, int epi, const RowPlan& rp, hipStream_t s) {
  const int sk = skinny_epi(epi);
  for (const RowPlan::Tiny& t : rp.tiny) {
    if (sk < 0 || a.K % 128) return fail(c, AIGV_ERR_STATE, "no skinny form for epilogue %d / K=%d (tiny sequence tails)", epi, a.K);
    const size_t ldx = (size_t)t.stride_rows * a.lda, ldo = (size_t)t.stride_rows * a.ldc, ldr = (size_t)t.stride_rows * a.ldr;
    if (ldx > 0x7fffffffu || ldo > 0x7fffffffu || ldr > 0x7fffffffu) return fail(c, AIGV_ERR_STATE, "tiny-tail row stride overflows");
    for (int i0 = 0; i0 < t.count; i0 += 64) {
      const int R = std::min(64, t.count - i0);
      const size_t r0 = (size_t)t.row0 + (size_t)i0 * t.stride_rows;
      ProfScope ps(c, c ? c->gemm_cls : AIGV_PROF_GEMM, 2.0 * R * (double)a.N * a.K, 2.0 * (double)a.N * a.K, s);
      took(t.stride_rows == 1 ? AIGV_ROUTE_TINY : AIGV_ROUTE_TINY_STRIDED);
      hipError_t e = aigv_launch_skinny_gemm(a.A + r0 * a.lda, (int)ldx, R, a.W, a.ldw, a.N, a.K, a.bias, a.resid ? a.resid + r0 * a.ldr : nullptr,
                                            (int)ldr, a.C + r0 * a.ldc, (int)ldo, sk, s, a.ls, 0);
      if (e != hipSuccess) return fail(c, AIGV_ERR_HIP, "skinny tiny tails (R=%d N=%d K=%d): %s", R, a.N, a.K, hipGetErrorString(e));
    }
  }
  return 0;
}

// A GEMM whose rows follow the row plan `rp` (mode 0); modes 1 / 2 / 4 run every row on one tile kernel in full K (also batch-invariant).
int run_gemm_rows(aigv_ctx* c, const GemmArgs& a, int epi, const RowPlan& rp, hipStream_t s) {
  if (const char* m = aigv_gemm_check(a, epi)) return fail(c, AIGV_ERR_ARG, "%s (M=%d N=%d K=%d epi=%d)", m, a.M, a.N, a.K, epi);
  if (a.M != rp.rows) return fail(c, AIGV_ERR_STATE, "row plan covers %d rows, the GEMM has %d", rp.rows, a.M);
  const int mode = resolved_gemm_mode(c);
  if (mode == 3) return run_gemm(c, a, epi, s);   // rounds 1-3: batch-level cost-model dispatch (A/B only: not batch-invariant)
  if (mode == 4) return use_co(c, a, mode) ? launch_co(c, a, epi, s) : launch_one(c, a, epi, false, s);
  if (use_co(c, a, mode)) {
    // short-K GEMMs (InternViT): body AND tail half tiles in one launch of the co-resident kernel, full K; tiny tails on the skinny kernel as below
    if (rp.body_halves + rp.tail_halves > 0) {
      GemmArgs b = a;
      b.row_tab = rp.d_tab; b.tab_halves = rp.body_halves + rp.tail_halves;
      GEMM_PROF_ROWS(c, a, rp.body_halves * 128 + rp.tail_rows, s);
      took(AIGV_ROUTE_TAB_CO);
      HIPCHK(c, aigv_launch_gemmco(tuned(c, b), epi, s));
    }
    return run_tiny_tails(c, a, epi, rp, s);
  }
  if (mode == 1 || a.N < 256) return launch_one(c, a, epi, false, s);
  if (mode == 2 && a.N % 256 == 0) return launch_one(c, a, epi, true, s);
  if (a.N % 256) {   // N = 256 j + 128 (InternViT-6B: 3200, 9600): the last 128 columns of every row on the 128 kernel, full K
    if (epi == EPI_SWIGLU) return launch_one(c, a, epi, false, s);
    TRY(run_gemm_rows(c, col_slice(a, 0, a.N - 128), epi, rp, s));
    return launch_one(c, col_slice(a, a.N - 128, 128), epi, false, s);
  }
  const int S = tail_slices(a.N, a.K, tune_knob(c, AIGV_TUNE_TAIL_SLICES));
  // The body rows may run on either tile kernel: both sum every output element over the full K in the same order, so not one bit moves
  // (tests/test_gpu_ops.py pins that).  Shipped: always the 256 tiles - for one clip, whose wo / w2 / ViT proj / fc2 bodies are only 128
  // tiles, the 128 kernel (512 tiles, two per CU) was expected to win by the cost model and measured 1-3 % slower per clip
  // (profiles/r4_negatives.txt, 6); body_tile = 2 keeps the 128 form reachable for tests.
  const bool body128 = rp.body_halves > 0 && tune_knob(c, AIGV_TUNE_BODY_TILE) == 2;
  const bool tails_apart = rp.tail_halves > 0 && S > 1;
  // A body of at most 128 tiles (one clip's wo / w2, eight frames' proj / fc2) leaves half the CUs idle: the co-resident kernel's LONE form
  // (gemmco.hip VAR 6: 256 x 128 tiles, one 8-wave workgroup per CU, four of the waves only issue the LDS-DMA requests) gives every CU a
  // tile - the same bits as the 256 kernel, 18-24 % less time on these bodies in isolation (scripts/gemm_body_ab.py) and NOTHING inside the
  // one-clip forward (37.9-38.1 ms per clip either way: profiles/r5_loop_shape.txt; the tail's K slices can no longer ride in the idle half of
  // the chip, and the SlowFast branch's side-stream kernels lose the CUs the half-empty bodies left them).  Off by default (lone_body = 1).
  const long body_tiles = (long)(rp.body_halves / 2) * (a.N / 256);
  const int lone_knob = tune_knob(c, AIGV_TUNE_LONE_BODY);   // 0 = by fill, 1 = never, 2 = whenever the shapes allow
  const bool lone = !body128 && lone_knob != 1 && rp.body_halves > 0 && a.N % 128 == 0 &&
                    (lone_knob == 2 || (body_tiles <= 128 && (!tails_apart || a.K / 64 >= 128) && (lone_knob != 3 || tails_apart) && (lone_knob != 4 || !tails_apart)));
  if (lone) {
    GemmArgs b = tuned(c, a);
    b.row_tab = rp.d_tab; b.tab_halves = tails_apart ? rp.body_halves : rp.body_halves + rp.tail_halves;
    b.variant_sel = 7;
    GEMM_PROF_ROWS(c, a, rp.body_halves * 128 + (tails_apart ? 0 : rp.tail_rows), s);
    took(AIGV_ROUTE_TAB_LONE);
    HIPCHK(c, aigv_launch_gemmco(b, epi, s));
  } else if (body128) {
    {
      GemmArgs b = a;
      b.row_tab = rp.d_tab; b.tab_halves = rp.body_halves;
      GEMM_PROF_ROWS(c, a, rp.body_halves * 128, s);
      took(AIGV_ROUTE_TAB_128);
      HIPCHK(c, aigv_launch_gemm(b, epi, s));
    }
    if (rp.tail_halves > 0 && !tails_apart) TRY(launch_tab(c, a, epi, rp.d_tab + 2 * rp.body_halves, rp.tail_halves, rp.tail_rows, 1, s));
  } else if (!tails_apart) {
    TRY(launch_tab(c, a, epi, rp.d_tab, rp.body_halves + rp.tail_halves, rp.body_halves * 128 + rp.tail_rows, 1, s));
  } else {
    // A body that leaves part of its last round of CUs idle (one or two clips) takes the tail's K slices into its own launch: the same
    // slices, slabs and finalize pass as the two-launch form - not one bit differs, so the choice may follow the fill (fuse_tails).
    const int tn = a.N / 256;
    const long body_wg = (long)(rp.body_halves / 2) * tn, slice_wg = (long)((rp.tail_halves + 1) / 2) * tn * S;
    const size_t need = (size_t)S * ((rp.tail_halves + 1) / 2) * 256 * a.N;
    const int fuse_knob = tune_knob(c, AIGV_TUNE_FUSE_TAILS);   // 0 = by fill, 1 = never, 2 = whenever the shapes allow
    const bool by_fill = body_wg % 256 != 0 && body_wg % 256 + slice_wg <= 320;
    if (!lone && rp.body_halves > 0 && (rp.body_halves & 1) == 0 && need <= (c ? c->splitk_floats : SPLITK_MAX_FLOATS) && fuse_knob != 1 && (by_fill || fuse_knob == 2)) {
      float* ws = nullptr;
      TRY(splitk_scratch(c, need, &ws));
      GemmArgs b = tuned(c, a);
      b.row_tab = rp.d_tab; b.tab_halves = rp.body_halves; b.fuse_tail_halves = rp.tail_halves; b.part = ws; b.k_slices = S;
      GEMM_PROF_ROWS(c, a, rp.body_halves * 128 + rp.tail_halves * 128, s);
      took(AIGV_ROUTE_TAB_FUSED);
      HIPCHK(c, aigv_launch_gemm256_fused(b, epi, s));
      GemmArgs f = a;
      f.row_tab = rp.d_tab + 2 * rp.body_halves; f.tab_halves = rp.tail_halves;
      HIPCHK(c, aigv_launch_gemm_finalize(f, epi, S, ws, s));
      return run_tiny_tails(c, a, epi, rp, s);
    }
    if (!lone) TRY(launch_tab(c, a, epi, rp.d_tab, rp.body_halves, rp.body_halves * 128, 1, s));
  }
  if (tails_apart) {
    const size_t per_pair = (size_t)S * 256 * a.N;
    const size_t cap = c ? c->splitk_floats : SPLITK_MAX_FLOATS;
    const int max_halves = (int)std::min<size_t>(cap / per_pair, 4096) * 2;
    if (max_halves < 2) return fail(c, AIGV_ERR_STATE, "split-K scratch too small for one tail tile (N=%d, %d slices)", a.N, S);
    for (int h0 = 0; h0 < rp.tail_halves; h0 += max_halves) {
      const int nh = std::min(max_halves, rp.tail_halves - h0);
      TRY(launch_tab(c, a, epi, rp.d_tab + 2 * (rp.body_halves + h0), nh, nh * 128, S, s));   // (profile: ragged halves counted as full)
    }
  }
  return run_tiny_tails(c, a, epi, rp, s);
}

// every row in full K on one tile kernel (the 256 kernel where its shape rules allow): batch-invariant for any row layout
int run_gemm_full(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s) {
  if (const char* m = aigv_gemm_check(a, epi)) return fail(c, AIGV_ERR_ARG, "%s (M=%d N=%d K=%d epi=%d)", m, a.M, a.N, a.K, epi);
  const int mode = resolved_gemm_mode(c);
  if (use_co(c, a, mode)) return launch_co(c, a, epi, s);
  if (mode == 1 || a.N < 256 || (a.N % 256 && epi == EPI_SWIGLU)) return launch_one(c, a, epi, false, s);
  if (a.N % 256) {
    TRY(launch_one(c, col_slice(a, 0, a.N - 128), epi, true, s));
    return launch_one(c, col_slice(a, a.N - 128, 128), epi, false, s);
  }
  return launch_one(c, a, epi, true, s);
}

// InternLM2 linears: under the current pass's row plan (aigv_llm_prefill), else the batch-level dispatch (aigv_llm_extend)
int run_llm_gemm(aigv_ctx* c, const GemmArgs& a, int epi, hipStream_t s) {
  return c->cur_rp ? run_gemm_rows(c, a, epi, *c->cur_rp, s) : run_gemm(c, a, epi, s);
}

GemmArgs gemm_args(const bf16_t* A, int lda, const bf16_t* W, int ldw, bf16_t* C, int ldc, int M, int N, int K) {
  GemmArgs a{};
  a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
  return a;
}

// One InternLM2 linear in fp8 mode: quantise the bf16 activation rows (per-row amax / 448), then the e4m3 form of the 256 kernel with
// the bf16 path's epilogue.  The quantisation pass is outside the profiled launch (it is not GEMM work).
int run_gemm_fp8(aigv_ctx* c, const bf16_t* A, int lda, int K, const uint8_t* W8, const float* w_scale, bf16_t* C, int ldc, int T, int N,
                 int epi, const bf16_t* resid, int ldr, hipStream_t s) {
  hipError_t e = hipSuccess;
  if (A) {   // A == nullptr: c->q8 / c->q8_scale already hold the quantised rows (RMSNorm fused with the quantisation)
    e = aigv_launch_quant_fp8_rows(A, lda, T, K, c->q8, K, c->q8_scale, s);
    if (e != hipSuccess) return fail(c, AIGV_ERR_HIP, "fp8 activation quantisation (T=%d K=%d): %s", T, K, hipGetErrorString(e));
  }
  GemmArgs a = tuned(c, GemmArgs{});
  a.A = (const bf16_t*)c->q8; a.lda = K; a.W = (const bf16_t*)W8; a.ldw = K; a.C = C; a.ldc = ldc; a.M = T; a.N = N; a.K = K;
  a.row_scale = c->q8_scale; a.col_scale = w_scale; a.resid = resid; a.ldr = ldr;
  ProfScope ps(c, AIGV_PROF_GEMM_FP8, 2.0 * T * (double)N * K, (double)T * K + (double)N * K + 2.0 * T * (epi == EPI_SWIGLU ? N / 2 : N), s);
  // ONE launch over all rows, every row in full K on the one e4m3 tile kernel: an output element's sum then runs over K in the same order
  // wherever its row sits, so a clip's bits do not depend on its batch mates - in this mode too (round 6; until round 5 the partial last
  // round of a batch ran as K slices, which tied a row's summation order to the size of the batch).
  e = aigv_launch_gemm256_fp8(a, epi, s);
  if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "fp8 gemm (M=%d N=%d K=%d epi=%d): %s", T, N, K, epi, hipGetErrorString(e));
  return 0;
}


// What the weight-streaming kernel needs of its row strides (head.hip: x and W rows are read 16 bytes at a time; the epilogue stores a
// u16x4 at out + r * ldo + n and reads one at resid + r * ldr + n).  nullptr if they fit.  run_skinny asks it; the skinny remainder of
// run_gemm and run_tiny_tails launch the kernel directly, behind aigv_gemm_check, whose rule (multiples of 8, at least the width)
// implies this one - a multiple of a multiple of 8 included (the tiny tails' row stride).  R > 64 and K % 128 are named here too, so
// that no refusal of run_skinny is left to the launcher's bare hipErrorInvalidValue.
const char* skinny_check(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, const bf16_t* resid, int ldr,
                         const bf16_t* out, int ldo, int epi) {
  if (R < 0 || N <= 0 || K <= 0) return "skinny gemm: empty problem";
  if (R > 64) return "skinny gemm: more than 64 rows";
  if (K % 128) return "skinny gemm: K must be a multiple of 128";
  if (!x || !W || !out) return "skinny gemm: null operand";
  if (ldx < K || ldw < K || (ldx % 8) || (ldw % 8)) return "skinny gemm: bad leading dimension (ldx and ldw: at least K, multiples of 8)";
  const int n_out = epi == SK_SWIGLU ? N / 2 : N;
  if (ldo < n_out) return "skinny gemm: ldo is below the output width (rows would overlap)";
  if (ldo % 4) return "skinny gemm: ldo must be a multiple of 4 (the kernel stores 8 bytes at out + row * ldo + n)";
  if ((epi == SK_RESID || epi == SK_LS_RESID) && !resid) return "skinny gemm: residual epilogue needs resid";
  if (resid && ldr < n_out) return "skinny gemm: ldr is below the width of the residual rows";
  if (resid && (ldr % 4)) return "skinny gemm: ldr must be a multiple of 4 (the kernel reads 8 bytes at resid + row * ldr + n)";
  return nullptr;
}

int run_skinny(aigv_ctx* c, const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, const bf16_t* bias,
               const bf16_t* resid, int ldr, bf16_t* out, int ldo, int epi, hipStream_t s, int p) {
  if (const char* m = skinny_check(x, ldx, R, W, ldw, N, K, resid, ldr, out, ldo, epi))
    return fail(c, AIGV_ERR_ARG, "%s (R=%d N=%d K=%d epi=%d)", m, R, N, K, epi);
  ProfScope ps(c, AIGV_PROF_SKINNY, 2.0 * R * (double)N * K, 2.0 * (double)N * K, s);
  // p = 0 (the scoring pass: last-layer consumed rows, motion_mlp, tiny sequence tails): the fixed 4-slice form whatever the row count, so
  // that a row's bits do not depend on its batch; p = 1 / 2 / 4 are the decode step's forms (decode_forms).
  hipError_t e = aigv_launch_skinny_gemm(x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, epi, s, nullptr, p);
  if (e != hipSuccess) return fail(c, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP,
                                   "skinny gemm (R=%d N=%d K=%d epi=%d): %s", R, N, K, epi, hipGetErrorString(e));
  return 0;
}

}  // namespace aigv

using namespace aigv;

// ---- measurement -----------------------------------------------------------------------------------------------
extern "C" int aigv_plan_gemm(int M, int N, int K, int epi, int* plan, double* est_us) {
  if (!plan || M <= 0 || N <= 0 || K <= 0 || N % 128 || K % 64 || epi < 0 || epi >= EPI_COUNT)
    return fail(nullptr, AIGV_ERR_ARG, "aigv_plan_gemm: bad problem M=%d N=%d K=%d epi=%d", M, N, K, epi);
  const int pmode = g_tune[AIGV_TUNE_GEMM_MODE] == 3 ? 0 : g_tune[AIGV_TUNE_GEMM_MODE];
  const int right = split_columns(M, N, K, epi, pmode);
  const GemmPlan pl = plan_gemm(M, N - right, K, epi, pmode);
  plan[6] = right;
  plan[0] = pl.top_tiles; plan[1] = pl.mid_tiles; plan[2] = pl.mid_slices; plan[3] = pl.last_rows; plan[4] = pl.last_kind;
  plan[5] = pl.last_slices;
  if (est_us) *est_us = pl.est_us + (right ? t128(M, right, K / 64) + LAUNCH_GAP : 0.0);
  return 0;
}

extern "C" int aigv_gemm_route(int clear) {
  return (int)(clear ? g_route.exchange(0, std::memory_order_relaxed) : g_route.load(std::memory_order_relaxed));
}
