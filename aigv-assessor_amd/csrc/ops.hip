// The context-free single-operator entry points of the C ABI (aigv_op_*: tests, benches and A/B scripts) and their argument checks.
// Host-side C++ only.
#include "ctx.h"

using namespace aigv;

extern "C" {

// ---- single operators ----------------------------------------------------------------------------------------
int aigv_op_gemm(const void* A, int lda, const void* W_, int ldw, void* C, int ldc, const void* bias, const void* ls,
                 const void* resid, int ldr, const void* pos, int np, int M, int N, int K, int epi, void* stream) {
  GemmArgs a = gemm_args((const bf16_t*)A, lda, (const bf16_t*)W_, ldw, (bf16_t*)C, ldc, M, N, K);
  a.bias = (const bf16_t*)bias; a.ls = (const bf16_t*)ls; a.resid = (const bf16_t*)resid; a.ldr = ldr;
  a.pos = (const bf16_t*)pos; a.np = np;
  return run_gemm(nullptr, a, epi, (hipStream_t)stream);
}

// The argument check of aigv_op_gemm / _rows / _splitk* and of aigv_op_skinny_gemm alone: host only, nothing is launched and no pointer is
// dereferenced.  0 if the call would reach its launch, else AIGV_ERR_ARG with the refusal in aigv_last_error(NULL).
int aigv_op_gemm_check(const void* A, int lda, const void* W_, int ldw, const void* C, int ldc, const void* bias, const void* ls,
                       const void* resid, int ldr, const void* pos, int np, int M, int N, int K, int epi) {
  GemmArgs a = gemm_args((const bf16_t*)A, lda, (const bf16_t*)W_, ldw, (bf16_t*)C, ldc, M, N, K);
  a.bias = (const bf16_t*)bias; a.ls = (const bf16_t*)ls; a.resid = (const bf16_t*)resid; a.ldr = ldr;
  a.pos = (const bf16_t*)pos; a.np = np;
  if (const char* m = aigv_gemm_check(a, epi)) return fail(nullptr, AIGV_ERR_ARG, "%s (M=%d N=%d K=%d epi=%d)", m, M, N, K, epi);
  return 0;
}

int aigv_op_skinny_gemm_check(const void* x, int ldx, int R, const void* W_, int ldw, int N, int K, const void* resid, int ldr,
                              const void* out, int ldo, int epi) {
  if (const char* m = skinny_check((const bf16_t*)x, ldx, R, (const bf16_t*)W_, ldw, N, K, (const bf16_t*)resid, ldr, (const bf16_t*)out, ldo, epi))
    return fail(nullptr, AIGV_ERR_ARG, "%s (R=%d N=%d K=%d epi=%d)", m, R, N, K, epi);
  return 0;
}

// aigv_op_gemm with the rows divided into independent sequences (cu_host[0..n_seq], cu[0] = 0, cu[n_seq] = M): the dispatch the scoring
// pass uses (struct RowPlan).  Test entry point: allocates the plan's table per call and synchronises the stream before freeing it.
int aigv_op_gemm_rows(const void* A, int lda, const void* W_, int ldw, void* C, int ldc, const void* bias, const void* ls,
                      const void* resid, int ldr, const int32_t* cu_host, int n_seq, int N, int K, int epi, void* stream) {
  if (!cu_host || n_seq < 1 || cu_host[0] != 0) return fail(nullptr, AIGV_ERR_ARG, "aigv_op_gemm_rows: bad cu_seqlens");
  for (int b = 0; b < n_seq; ++b)
    if (cu_host[b + 1] <= cu_host[b]) return fail(nullptr, AIGV_ERR_ARG, "aigv_op_gemm_rows: empty sequence %d", b);
  if (epi == EPI_PATCH) return fail(nullptr, AIGV_ERR_ARG, "aigv_op_gemm_rows: no patch epilogue");
  const int M = cu_host[n_seq];
  GemmArgs a = gemm_args((const bf16_t*)A, lda, (const bf16_t*)W_, ldw, (bf16_t*)C, ldc, M, N, K);
  a.bias = (const bf16_t*)bias; a.ls = (const bf16_t*)ls; a.resid = (const bf16_t*)resid; a.ldr = ldr;
  RowPlan rp;
  rp.cap_halves = M / 128 + 2 * n_seq + 2;
  HIPCHK(nullptr, hipMalloc((void**)&rp.d_tab, (size_t)2 * rp.cap_halves * sizeof(int32_t)));
  int rc = build_row_plan(nullptr, rp, cu_host, n_seq, (hipStream_t)stream);
  if (!rc) rc = run_gemm_rows(nullptr, a, epi, rp, (hipStream_t)stream);
  hipStreamSynchronize((hipStream_t)stream);
  hipFree(rp.d_tab);
  return rc;
}

int aigv_op_gemm_splitk(const void* A, int lda, const void* W_, int ldw, void* C, int ldc, const void* bias, const void* ls,
                        const void* resid, int ldr, int M, int N, int K, int epi, int k_slices, void* ws_f32, void* stream) {
  GemmArgs a = gemm_args((const bf16_t*)A, lda, (const bf16_t*)W_, ldw, (bf16_t*)C, ldc, M, N, K);
  a.bias = (const bf16_t*)bias; a.ls = (const bf16_t*)ls; a.resid = (const bf16_t*)resid; a.ldr = ldr;
  if (const char* m = aigv_gemm_check(a, epi)) return fail(nullptr, AIGV_ERR_ARG, "%s", m);
  hipError_t e = aigv_launch_gemm_splitk(a, epi, k_slices, (float*)ws_f32, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "split-K gemm: %s", hipGetErrorString(e));
  return 0;
}

int aigv_op_gemm_splitk256(const void* A, int lda, const void* W_, int ldw, void* C, int ldc, const void* bias, const void* ls,
                           const void* resid, int ldr, int M, int N, int K, int epi, int k_slices, void* ws_f32, void* stream) {
  GemmArgs a = gemm_args((const bf16_t*)A, lda, (const bf16_t*)W_, ldw, (bf16_t*)C, ldc, M, N, K);
  a.bias = (const bf16_t*)bias; a.ls = (const bf16_t*)ls; a.resid = (const bf16_t*)resid; a.ldr = ldr;
  if (const char* m = aigv_gemm_check(a, epi)) return fail(nullptr, AIGV_ERR_ARG, "%s", m);
  hipError_t e = aigv_launch_gemm_splitk(a, epi, k_slices, (float*)ws_f32, (hipStream_t)stream, true);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "split-K gemm (256 tile): %s", hipGetErrorString(e));
  return 0;
}

int aigv_op_quant_fp8_rows(const void* x_bf16, int ldx, int rows, int K, void* q_e4m3, int ldq, float* row_scale, void* stream) {
  hipError_t e = aigv_launch_quant_fp8_rows((const bf16_t*)x_bf16, ldx, rows, K, (uint8_t*)q_e4m3, ldq, row_scale, (hipStream_t)stream);
  if (e != hipSuccess) return fail(nullptr, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "fp8 row quantisation (rows=%d K=%d): %s", rows, K, hipGetErrorString(e));
  return 0;
}

int aigv_op_gemm_fp8(const void* A_e4m3, int lda, const void* W_e4m3, int ldw, void* C, int ldc, const float* row_scale,
                     const float* col_scale, const void* bias, const void* ls, const void* resid, int ldr, int M, int N, int K, int epi,
                     int k_slices, void* ws_f32, void* stream) {
  GemmArgs a{};
  a.A = (const bf16_t*)A_e4m3; a.lda = lda; a.W = (const bf16_t*)W_e4m3; a.ldw = ldw; a.C = (bf16_t*)C; a.ldc = ldc;
  a.M = M; a.N = N; a.K = K; a.bias = (const bf16_t*)bias; a.row_scale = row_scale; a.col_scale = col_scale;
  a.ls = (const bf16_t*)ls; a.resid = (const bf16_t*)resid; a.ldr = ldr;
  const int n_out = epi == EPI_SWIGLU ? N / 2 : N;
  if (ldc < n_out || (ldc % 8) || lda < K || ldw < K)
    return fail(nullptr, AIGV_ERR_ARG, "aigv_op_gemm_fp8: bad leading dimension (M=%d N=%d K=%d)", M, N, K);
  hipError_t e = k_slices > 1 ? aigv_launch_gemm_splitk_fp8(a, epi, k_slices, (float*)ws_f32, (hipStream_t)stream)
                              : aigv_launch_gemm256_fp8(a, epi, (hipStream_t)stream);
  if (e != hipSuccess)
    return fail(nullptr, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP,
                "fp8 gemm (M=%d N=%d K=%d epi=%d; needs N %% 256 == 0, K %% 128 == 0, 16-byte row strides, both scale vectors, epi in "
                "{store, gelu, ls_resid, resid, swiglu}): %s", M, N, K, epi, hipGetErrorString(e));
  return 0;
}

int aigv_op_skinny_gemm(const void* x, int ldx, int R, const void* W_, int ldw, int N, int K, const void* bias,
                        const void* resid, int ldr, void* out, int ldo, int epi, void* stream) {
  return run_skinny(nullptr, (const bf16_t*)x, ldx, R, (const bf16_t*)W_, ldw, N, K, (const bf16_t*)bias,
                    (const bf16_t*)resid, ldr, (bf16_t*)out, ldo, epi, (hipStream_t)stream, g_tune[AIGV_TUNE_SKINNY_P] ? g_tune[AIGV_TUNE_SKINNY_P] : 1);
}

int aigv_op_skinny_gemm_fp8(const void* x, int ldx, int R, const void* W_e4m3, int ldw, const float* w_scale, int N, int K, const void* resid,
                            int ldr, void* out, int ldo, int epi, const void* norm_w, float eps, int p, void* stream) {
  if (epi != SK_RESID && epi != SK_SWIGLU) return fail(nullptr, AIGV_ERR_ARG, "aigv_op_skinny_gemm_fp8: epi must be 1 (residual) or 2 (swiglu)");
  hipError_t e = aigv_launch_skinny_fp8((const bf16_t*)x, ldx, R, (const uint8_t*)W_e4m3, ldw, w_scale, N, K, (const bf16_t*)resid, ldr, (bf16_t*)out, ldo,
                                        epi, nullptr, (const bf16_t*)norm_w, eps, p, (hipStream_t)stream);
  if (e != hipSuccess)
    return fail(nullptr, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "fp8 skinny gemm (R=%d N=%d K=%d epi=%d p=%d): %s", R, N, K, epi, p, hipGetErrorString(e));
  return 0;
}

// ---- the norm kernels (test entry points; the passes call the launchers): every argument is checked here, before any HIP call ----
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// rows of H bf16 in 16-byte chunks, H <= 16384 (8 chunks per thread of a 256-thread workgroup); b: LayerNorm's bias (has_b)
static int check_norm(const char* op, const void* x, int ldx, const void* w, const void* b, bool has_b, const void* y, int ldy, int rows, int H) {
  if (!x || !w || !y || (has_b && !b)) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (rows < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: rows = %d must not be negative", op, rows);
  if (H < 8 || H % 8 || H > 16384) return fail(nullptr, AIGV_ERR_ARG, "%s: H = %d is not a multiple of 8 in 8..16384", op, H);
  if (ldx < H || ldx % 8 || ldy < H || ldy % 8)
    return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ldx %d, ldy %d: multiples of 8, >= H = %d)", op, ldx, ldy, H);
  if (!aligned16(x) || !aligned16(w) || !aligned16(b) || !aligned16(y)) return fail(nullptr, AIGV_ERR_ARG, "%s: the operands must be 16-byte aligned", op);
  return 0;
}

int aigv_op_layernorm(const void* x, int ldx, const void* w, const void* b, void* y, int ldy, int rows, int H, float eps,
                      void* stream) {
  TRY(check_norm("aigv_op_layernorm", x, ldx, w, b, true, y, ldy, rows, H));
  HIPCHK(nullptr, aigv_launch_layernorm((const bf16_t*)x, ldx, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, ldy, rows, H,
                                        eps, (hipStream_t)stream));
  return 0;
}

// row_idx (DEVICE int32 [rows], may be NULL): row i of y = the norm of row row_idx[i] of x.  y == x is allowed where row i reads row i
// (the InternViT qk-norm runs in place): every thread has read its chunks before any thread writes.
int aigv_op_rmsnorm(const void* x, int ldx, const void* w, void* y, int ldy, int rows, int H, float eps,
                    const int32_t* row_idx, void* stream) {
  TRY(check_norm("aigv_op_rmsnorm", x, ldx, w, nullptr, false, y, ldy, rows, H));
  if ((uintptr_t)row_idx & 3) return fail(nullptr, AIGV_ERR_ARG, "aigv_op_rmsnorm: row_idx must be 4-byte aligned");
  HIPCHK(nullptr, aigv_launch_rmsnorm((const bf16_t*)x, ldx, (const bf16_t*)w, (bf16_t*)y, ldy, rows, H, eps, row_idx,
                                      (hipStream_t)stream));
  return 0;
}

int aigv_op_rope(void* qkv, int ld, const int32_t* pos, const void* cos, const void* sin, int tokens, int n_rot, int slots,
                 int n_groups, int head_dim, void* stream) {
  HIPCHK(nullptr, aigv_launch_rope((bf16_t*)qkv, ld, pos, (const bf16_t*)cos, (const bf16_t*)sin, tokens, n_rot, slots,
                                   n_groups, head_dim, (hipStream_t)stream));
  return 0;
}

int aigv_op_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                      const int32_t* cu, int n_seq, int max_len, int n_heads, int n_kv_heads, int q_group_stride,
                      int kv_head_stride, int head_dim, int causal, float post_div, float q_prescale, void* stream) {
  return aigv_op_attention_rope(q, ldq, k, ldk, v, ldv, o, ldo, cu, n_seq, max_len, n_heads, n_kv_heads, q_group_stride, kv_head_stride, head_dim,
                                causal, post_div, q_prescale, nullptr, nullptr, nullptr, stream);   // (no rotation: the same AttnArgs without rope_*)
}

int aigv_op_attention_rope(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                           const int32_t* cu, int n_seq, int max_len, int n_heads, int n_kv_heads, int q_group_stride,
                           int kv_head_stride, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos,
                           const void* cos, const void* sin, void* stream) {
  AttnArgs a{};
  a.q = (const bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = ldk; a.v = (const bf16_t*)v; a.ldv = ldv;
  a.o = (bf16_t*)o; a.ldo = ldo; a.cu = cu; a.n_seq = n_seq; a.max_len = max_len; a.n_heads = n_heads;
  a.n_kv_heads = n_kv_heads; a.q_group_stride = q_group_stride; a.kv_head_stride = kv_head_stride;
  a.causal = causal & 1; a.uniform_len = (causal >> 1) & 1; a.post_div = post_div; a.q_prescale = q_prescale;
  a.round_scores = (causal >> 2) & 1; a.lead_key = (causal >> 3) & 1; a.waves = g_tune[AIGV_TUNE_ATTN_WAVES];
  a.rope_pos = pos; a.rope_cos = (const bf16_t*)cos; a.rope_sin = (const bf16_t*)sin;
  if (const char* m = aigv_attn_check(a, head_dim)) return fail(nullptr, AIGV_ERR_ARG, "%s", m);
  HIPCHK(nullptr, aigv_launch_attention(a, head_dim, (hipStream_t)stream));
  return 0;
}

// ---- the address and mask forms of the prefill attention that the scoring passes use (test entry points): checked here, before any HIP call ----
// AttnArgs as llm_attn_args + the call sites of aigv_llm_prefill (packed K/V, q_tail) and aigv_llm_extend (K/V in the cache, kv_off) fill them.
static int attention_ex_op(const char* op, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu,
                           int n_seq, int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                           const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                           const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, int ld_drop, void* stream,
                           const uint64_t* row_words = nullptr, bool drop_noncausal = false) {
  if (!q || !k || !v || !o || !cu) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (drop_noncausal && (causal & 1)) return fail(nullptr, AIGV_ERR_ARG, "%s: the non-causal key-drop form, got causal != 0 (aigv_op_attention_drop is the causal one)", op);
  if (drop_noncausal && key_drop && (kv_off || kv_seq_stride))   // (here, in front of the read-back of kv_off below)
    return fail(nullptr, AIGV_ERR_ARG, "%s: key_drop exists for the packed layout only (no kv_off, no kv_seq_stride)", op);
  if (row_words && !key_drop) return fail(nullptr, AIGV_ERR_ARG, "%s: row_words qualify a key_drop mask and need one", op);
  if (row_words && (kv_off || kv_seq_stride)) return fail(nullptr, AIGV_ERR_ARG, "%s: row_words exist for the packed prefill only (no kv_off, no kv_seq_stride)", op);
  if (q_tail < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: q_tail = %d must not be negative", op, q_tail);
  if (kv_seq_stride < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: kv_seq_stride = %lld must not be negative", op, (long long)kv_seq_stride);
  if (kv_off && !kv_seq_stride) return fail(nullptr, AIGV_ERR_ARG, "%s: a key offset needs K/V in cache layout (kv_seq_stride)", op);
  if (pos_is_row && !cos) return fail(nullptr, AIGV_ERR_ARG, "%s: pos_is_row selects how the query RoPE finds its position: it needs cos and sin", op);
  AttnArgs a{};
  a.q = (const bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = ldk; a.v = (const bf16_t*)v; a.ldv = ldv;
  a.o = (bf16_t*)o; a.ldo = ldo; a.cu = cu; a.n_seq = n_seq; a.max_len = max_len; a.n_heads = n_heads;
  a.n_kv_heads = n_kv_heads; a.q_group_stride = q_group_stride; a.kv_head_stride = kv_head_stride;
  a.kv_seq_stride = (size_t)kv_seq_stride; a.kv_off = kv_off;
  a.causal = causal & 1; a.uniform_len = (causal >> 1) & 1; a.post_div = post_div; a.q_prescale = q_prescale;
  a.round_scores = (causal >> 2) & 1; a.lead_key = (causal >> 3) & 1; a.waves = g_tune[AIGV_TUNE_ATTN_WAVES];
  a.rope_pos = pos; a.rope_cos = (const bf16_t*)cos; a.rope_sin = (const bf16_t*)sin;
  a.rope_pos_is_row = pos_is_row ? 1 : 0;
  a.q_tail = q_tail;
  if (key_drop) {
    a.key_drop = key_drop; a.ld_drop = ld_drop; a.drop_rows = row_words;
    if (kv_off) {
      // the check needs the largest key offset, which lives on the device: read back here (a test entry point; the passes know theirs on the host)
      if (n_seq < 1 || n_seq > AIGV_SMALL_INTS) return fail(nullptr, AIGV_ERR_ARG, "%s: key_drop with kv_off takes 1..%d sequences, got %d", op, AIGV_SMALL_INTS, n_seq);
      int32_t off[AIGV_SMALL_INTS];
      HIPCHK(nullptr, hipStreamSynchronize((hipStream_t)stream));
      HIPCHK(nullptr, hipMemcpy(off, kv_off, (size_t)n_seq * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int b = 0; b < n_seq; ++b) {
        if (off[b] < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: kv_off[%d] = %d must not be negative", op, b, off[b]);
        a.kv_len_offset = std::max(a.kv_len_offset, (int)off[b]);
      }
    }
  }
  if (const char* m = aigv_attn_check(a, head_dim, drop_noncausal)) return fail(nullptr, AIGV_ERR_ARG, "%s: %s", op, m);
  HIPCHK(nullptr, aigv_launch_attention(a, head_dim, (hipStream_t)stream));
  return 0;
}

int aigv_op_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                         int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                         const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                         const void* sin, int pos_is_row, int q_tail, void* stream) {
  return attention_ex_op("aigv_op_attention_ex", q, ldq, k, ldk, v, ldv, o, ldo, cu, n_seq, max_len, n_heads, n_kv_heads, q_group_stride, kv_head_stride,
                         kv_seq_stride, kv_off, head_dim, causal, post_div, q_prescale, pos, cos, sin, pos_is_row, q_tail, nullptr, 0, stream);
}

// aigv_op_attention_ex under a key-drop mask (AttnArgs::key_drop; null: the same call as aigv_op_attention_ex)
int aigv_op_attention_drop(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                           int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                           const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                           const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, int ld_drop, void* stream) {
  return attention_ex_op("aigv_op_attention_drop", q, ldq, k, ldk, v, ldv, o, ldo, cu, n_seq, max_len, n_heads, n_kv_heads, q_group_stride, kv_head_stride,
                         kv_seq_stride, kv_off, head_dim, causal, post_div, q_prescale, pos, cos, sin, pos_is_row, q_tail, key_drop, ld_drop, stream);
}

// aigv_op_attention_drop with a row selector (AttnArgs::drop_rows; null: the same call as aigv_op_attention_drop): the packed prefill form only
int aigv_op_attention_drop_rows(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                                int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                                const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                                const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, const uint64_t* row_words, int ld_drop,
                                void* stream) {
  return attention_ex_op("aigv_op_attention_drop_rows", q, ldq, k, ldk, v, ldv, o, ldo, cu, n_seq, max_len, n_heads, n_kv_heads, q_group_stride,
                         kv_head_stride, kv_seq_stride, kv_off, head_dim, causal, post_div, q_prescale, pos, cos, sin, pos_is_row, q_tail, key_drop, ld_drop,
                         stream, row_words);
}

// aigv_op_attention_ex under the NON-causal key-drop mask (InternViT's patch mask; null: the same call as aigv_op_attention_ex with causal == 0)
int aigv_op_attention_nc_drop(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                              int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                              const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                              const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, int ld_drop, void* stream) {
  return attention_ex_op("aigv_op_attention_nc_drop", q, ldq, k, ldk, v, ldv, o, ldo, cu, n_seq, max_len, n_heads, n_kv_heads, q_group_stride,
                         kv_head_stride, kv_seq_stride, kv_off, head_dim, causal, post_div, q_prescale, pos, cos, sin, pos_is_row, q_tail, key_drop, ld_drop,
                         stream, nullptr, true);
}

// K / V slots of fused qkv rows -> the KV cache [seq][kv head][cap][head_dim]: the kernel aigv_llm_prefill (keep_kv) and aigv_llm_extend append with
int aigv_op_kv_store(const void* qkv, int ld, const int32_t* seq, const int32_t* pos, void* kc, void* vc, int tokens, int n_kv, int g,
                     int head_dim, int cap, void* stream) {
  const char* op = "aigv_op_kv_store";
  if (!qkv || !seq || !pos || !kc || !vc) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (tokens < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: tokens = %d must not be negative", op, tokens);
  if (g < 1 || g > 8 || n_kv < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: g = %d query heads per KV head (1..8), n_kv = %d (>= 1)", op, g, n_kv);
  if (head_dim < 8 || head_dim % 8) return fail(nullptr, AIGV_ERR_ARG, "%s: head_dim = %d is not a positive multiple of 8", op, head_dim);
  if (cap < 1 || cap > AIGV_MAX_KV_CAPACITY) return fail(nullptr, AIGV_ERR_ARG, "%s: cap = %d outside 1..%d", op, cap, AIGV_MAX_KV_CAPACITY);
  if (ld % 8 || (int64_t)ld < (int64_t)n_kv * (g + 2) * head_dim)
    return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ld %d, needs a multiple of 8 and >= n_kv (g + 2) head_dim)", op, ld);
  if (((uintptr_t)qkv & 15) || ((uintptr_t)kc & 15) || ((uintptr_t)vc & 15)) return fail(nullptr, AIGV_ERR_ARG, "%s: qkv and the caches must be 16-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_kv_store((const bf16_t*)qkv, ld, seq, pos, (bf16_t*)kc, (bf16_t*)vc, tokens, n_kv, g, head_dim, cap, (hipStream_t)stream));
  return 0;
}

// out [n_frames * (grid / 2)^2, 4 * vit_hidden] = the pixel-shuffled patch tokens of vit_out [n_frames, grid^2 + 1, vit_hidden] (the cls row is dropped)
int aigv_op_pixel_shuffle(const void* vit_out, int grid, int vit_hidden, void* out, int n_frames, void* stream) {
  const char* op = "aigv_op_pixel_shuffle";
  if (!vit_out || !out) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (n_frames < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: %d frames: must not be negative", op, n_frames);
  if (grid < 2 || grid % 2 || grid > 1024) return fail(nullptr, AIGV_ERR_ARG, "%s: grid = %d is not an even number in 2..1024", op, grid);
  if (vit_hidden < 8 || vit_hidden % 8 || vit_hidden > 16384)
    return fail(nullptr, AIGV_ERR_ARG, "%s: vit_hidden = %d is not a multiple of 8 in 8..16384", op, vit_hidden);
  if ((int64_t)n_frames * (grid / 2) * (grid / 2) > INT32_MAX) return fail(nullptr, AIGV_ERR_ARG, "%s: %d frames of a %d grid: too many output rows", op, n_frames, grid);
  if (!aligned16(vit_out) || !aligned16(out)) return fail(nullptr, AIGV_ERR_ARG, "%s: the operands must be 16-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_pixel_shuffle((const bf16_t*)vit_out, grid, vit_hidden, (bf16_t*)out, n_frames, (hipStream_t)stream));
  return 0;
}

// out [n_frames * (image_size / patch)^2, kp] = the patches of frames [n_frames, channels, image_size, image_size]; columns from channels * patch^2 on are zero
int aigv_op_im2col(const void* frames, int n_frames, int channels, int image_size, int patch, int kp, void* out,
                   void* stream) {
  const char* op = "aigv_op_im2col";
  if (!frames || !out) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (n_frames < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: %d frames: must not be negative", op, n_frames);
  if (channels < 1 || patch < 1 || patch > 1024 || image_size < patch || image_size > 16384)
    return fail(nullptr, AIGV_ERR_ARG, "%s: needs channels (%d) >= 1 and 1 <= patch (%d) <= image_size (%d) <= 16384", op, channels, patch, image_size);
  if (image_size % patch) return fail(nullptr, AIGV_ERR_ARG, "%s: image_size = %d is not a multiple of patch = %d", op, image_size, patch);
  if ((int64_t)kp < (int64_t)channels * patch * patch) return fail(nullptr, AIGV_ERR_ARG, "%s: kp = %d below channels * patch^2 = %lld", op, kp, (long long)channels * patch * patch);
  const int64_t g = image_size / patch;
  if ((int64_t)n_frames * g * g > INT32_MAX) return fail(nullptr, AIGV_ERR_ARG, "%s: %d frames of %lld x %lld patches: too many rows", op, n_frames, (long long)g, (long long)g);
  if (!aligned16(frames) || !aligned16(out)) return fail(nullptr, AIGV_ERR_ARG, "%s: the operands must be 16-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_im2col((const bf16_t*)frames, n_frames, channels, image_size, patch, kp, (bf16_t*)out,
                                     (hipStream_t)stream));
  return 0;
}

int aigv_op_lm_head_argmax(const void* h, int rows, int hidden, const void* W_, int vocab, void* scratch_u64, int64_t* idx,
                           float* val, void* stream) {
  HIPCHK(nullptr, aigv_launch_lm_head_argmax((const bf16_t*)h, rows, hidden, (const bf16_t*)W_, vocab,
                                             (unsigned long long*)scratch_u64, idx, val, (hipStream_t)stream));
  return 0;
}

int64_t aigv_op_lm_head_argmax_logprob_scratch_bytes(int rows, int vocab) {
  if (rows < 1 || rows > 64 || vocab < 1) return -1;
  return (int64_t)(64 * sizeof(unsigned long long) + (size_t)rows * aigv_lm_head_lse_slots(vocab) * sizeof(float2));
}

// aigv_op_lm_head_argmax_logprob / aigv_op_lm_head_argmax_cand_logprob (C >= 1) / aigv_op_lm_head_argmax_topk_logprob (k >= 1, C >= 0): every
// argument is checked here, before any HIP call.
// scratch = [64 packed keys | log-sum-exp partials | (16-byte aligned) candidate logits | (k >= 1: 16-byte aligned) the rows' logits]
static int lm_head_logprob_op(const char* op, const void* h, int rows, int hidden, const void* W_, int vocab, const int64_t* cand_ids, int C, void* scratch,
                              int64_t scratch_bytes, int64_t* idx, float* val, float* logprob, float* cand_logprob, void* stream, int k = 0,
                              int64_t* top_ids = nullptr, float* top_logprob = nullptr) {
  if (!h || !W_ || !scratch || !idx || !logprob || (C && (!cand_ids || !cand_logprob)) || (k && (!top_ids || !top_logprob)))
    return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (rows < 1 || rows > 64) return fail(nullptr, AIGV_ERR_ARG, "%s: rows = %d outside 1..64", op, rows);
  if (hidden < 128 || hidden % 128) return fail(nullptr, AIGV_ERR_ARG, "%s: hidden = %d is not a positive multiple of 128", op, hidden);
  if (vocab < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: vocab = %d must be positive", op, vocab);
  if (((uintptr_t)h & 15) || ((uintptr_t)W_ & 15) || ((uintptr_t)scratch & 15)) return fail(nullptr, AIGV_ERR_ARG, "%s: h, W and scratch must be 16-byte aligned", op);
  const int64_t base = aigv_op_lm_head_argmax_logprob_scratch_bytes(rows, vocab);
  const int64_t cbytes = aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(rows, vocab);
  const int64_t need = k ? aigv_op_lm_head_argmax_topk_logprob_scratch_bytes(rows, vocab) : C ? cbytes : base;
  if (scratch_bytes < need) return fail(nullptr, AIGV_ERR_ARG, "%s: scratch of %lld bytes, needs %lld", op, (long long)scratch_bytes, (long long)need);
  unsigned long long* packed = (unsigned long long*)scratch;
  float2* part = (float2*)((char*)scratch + 64 * sizeof(unsigned long long));
  bf16_t* cl = C ? (bf16_t*)((char*)scratch + (base + 15) / 16 * 16) : nullptr;
  bf16_t* rl = k ? (bf16_t*)((char*)scratch + (cbytes + 15) / 16 * 16) : nullptr;
  HIPCHK(nullptr, aigv_launch_lm_head_argmax_logprob((const bf16_t*)h, rows, hidden, (const bf16_t*)W_, vocab, packed, part, idx, val, logprob,
                                                     (hipStream_t)stream, cand_ids, C, cl, cand_logprob, k, rl, (int)aigv_topk_logit_ld(vocab), top_ids,
                                                     top_logprob));
  return 0;
}

int aigv_op_lm_head_argmax_logprob(const void* h, int rows, int hidden, const void* W_, int vocab, void* scratch, int64_t scratch_bytes,
                                   int64_t* idx, float* val, float* logprob, void* stream) {
  return lm_head_logprob_op("aigv_op_lm_head_argmax_logprob", h, rows, hidden, W_, vocab, nullptr, 0, scratch, scratch_bytes, idx, val, logprob, nullptr, stream);
}

int aigv_op_label_logprob(const void* logits_bf16, int rows, int vocab, int ldo, const int64_t* labels, float* out, void* stream) {
  if (rows < 0 || vocab < 1 || ldo < vocab || (rows > 0 && (!logits_bf16 || !labels || !out)))
    return fail(nullptr, AIGV_ERR_ARG, "aigv_op_label_logprob: bad argument (rows %d, vocab %d, ldo %d)", rows, vocab, ldo);
  HIPCHK(nullptr, aigv_launch_label_logprob((const bf16_t*)logits_bf16, rows, vocab, ldo, labels, out, (hipStream_t)stream));
  return 0;
}

int aigv_op_cand_logprob(const void* logits_bf16, int rows, int vocab, int ldo, const int64_t* cand_ids, int C, float* out, void* stream) {
  const char* op = "aigv_op_cand_logprob";
  if (C < 1 || C > AIGV_MAX_CANDIDATES) return fail(nullptr, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d", op, C, AIGV_MAX_CANDIDATES);
  if (!cand_ids || (rows > 0 && (!logits_bf16 || !out))) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (rows < 0 || vocab < 1 || ldo < vocab) return fail(nullptr, AIGV_ERR_ARG, "%s: bad argument (rows %d, vocab %d, ldo %d)", op, rows, vocab, ldo);
  HIPCHK(nullptr, aigv_launch_cand_logprob((const bf16_t*)logits_bf16, rows, vocab, ldo, cand_ids, C, out, (hipStream_t)stream));
  return 0;
}

int64_t aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(int rows, int vocab) {
  const int64_t base = aigv_op_lm_head_argmax_logprob_scratch_bytes(rows, vocab);   // [packed keys | log-sum-exp partials], then the candidate logits
  return base < 0 ? -1 : (base + 15) / 16 * 16 + (int64_t)(aigv_cand_logit_elems(rows) * sizeof(bf16_t));
}

int aigv_op_lm_head_argmax_cand_logprob(const void* h, int rows, int hidden, const void* W_, int vocab, const int64_t* cand_ids, int C,
                                        void* scratch, int64_t scratch_bytes, int64_t* idx, float* val, float* logprob, float* cand_logprob,
                                        void* stream) {
  const char* op = "aigv_op_lm_head_argmax_cand_logprob";
  if (C < 1 || C > AIGV_MAX_CANDIDATES) return fail(nullptr, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d", op, C, AIGV_MAX_CANDIDATES);
  return lm_head_logprob_op(op, h, rows, hidden, W_, vocab, cand_ids, C, scratch, scratch_bytes, idx, val, logprob, cand_logprob, stream);
}

int aigv_op_topk_logprob(const void* logits_bf16, int rows, int vocab, int ldo, int k, int64_t* top_ids, float* top_logprob, void* stream) {
  const char* op = "aigv_op_topk_logprob";
  if (rows < 0 || vocab < 1 || ldo < vocab) return fail(nullptr, AIGV_ERR_ARG, "%s: bad argument (rows %d, vocab %d, ldo %d)", op, rows, vocab, ldo);
  if (k < 1 || k > AIGV_MAX_TOPK || k > vocab) return fail(nullptr, AIGV_ERR_ARG, "%s: k = %d outside 1..min(%d, vocab = %d)", op, k, AIGV_MAX_TOPK, vocab);
  if (rows > 0 && (!logits_bf16 || !top_ids || !top_logprob)) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  HIPCHK(nullptr, aigv_launch_topk_logprob((const bf16_t*)logits_bf16, rows, vocab, ldo, k, top_ids, top_logprob, (hipStream_t)stream));
  return 0;
}

int64_t aigv_op_lm_head_argmax_topk_logprob_scratch_bytes(int rows, int vocab) {
  const int64_t cbytes = aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(rows, vocab);   // candidates are optional: their scratch is always laid out
  return cbytes < 0 ? -1 : (cbytes + 15) / 16 * 16 + (int64_t)((size_t)rows * aigv_topk_logit_ld(vocab) * sizeof(bf16_t));
}

int aigv_op_lm_head_argmax_topk_logprob(const void* h, int rows, int hidden, const void* W_, int vocab, int k, const int64_t* cand_ids, int C,
                                        void* scratch, int64_t scratch_bytes, int64_t* idx, float* val, float* logprob, int64_t* top_ids,
                                        float* top_logprob, float* cand_logprob, void* stream) {
  const char* op = "aigv_op_lm_head_argmax_topk_logprob";
  if (k < 1 || k > AIGV_MAX_TOPK || k > vocab) return fail(nullptr, AIGV_ERR_ARG, "%s: k = %d outside 1..min(%d, vocab = %d)", op, k, AIGV_MAX_TOPK, vocab);
  if (cand_ids ? (C < 1 || C > AIGV_MAX_CANDIDATES) : C != 0) return fail(nullptr, AIGV_ERR_ARG, "%s: C = %d candidates outside 1..%d (0 without cand_ids)", op, C, AIGV_MAX_CANDIDATES);
  return lm_head_logprob_op(op, h, rows, hidden, W_, vocab, cand_ids, C, scratch, scratch_bytes, idx, val, logprob, cand_logprob, stream, k, top_ids, top_logprob);
}

// ---- the decode step's kernels, one by one (test entry points): every argument is checked here, before any HIP call ----
int64_t aigv_op_attention_decode_ws_floats(int n_seq, int n_kv, int g, int cap) {
  if (n_seq < 1 || n_kv < 1 || g < 1 || g > 8 || cap < 1 || cap > AIGV_MAX_KV_CAPACITY) return -1;
  return (int64_t)aigv_attention_decode_ws_floats(n_seq, n_kv, g, cap);
}

static int attention_decode_op(const char* op, const void* q, int ldq, int q_group_stride, const void* kc, const void* vc, const int32_t* kv_lens, int cap,
                               void* o, int ldo, int n_seq, int n_kv, int g, int head_dim, float post_div, int max_kv_len, float* ws,
                               int64_t ws_floats, const uint64_t* key_drop, int ld_drop, void* stream) {
  if (!q || !kc || !vc || !kv_lens || !o || !ws) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (head_dim != 128) return fail(nullptr, AIGV_ERR_ARG, "%s: head_dim must be 128, got %d", op, head_dim);
  if (g < 1 || g > 8) return fail(nullptr, AIGV_ERR_ARG, "%s: g = %d query heads per KV head (1..8)", op, g);
  if (n_seq < 1 || n_kv < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: n_seq %d, n_kv %d must be positive", op, n_seq, n_kv);
  if (cap < 1 || cap > AIGV_MAX_KV_CAPACITY || max_kv_len < 1 || max_kv_len > cap)
    return fail(nullptr, AIGV_ERR_ARG, "%s: needs 1 <= max_kv_len (%d) <= cap (%d) <= %d", op, max_kv_len, cap, AIGV_MAX_KV_CAPACITY);
  if (q_group_stride < g * head_dim || ldq < (n_kv - 1) * q_group_stride + g * head_dim || ldo < n_kv * g * head_dim)
    return fail(nullptr, AIGV_ERR_ARG, "%s: strides too small (ldq %d, q_group_stride %d, ldo %d)", op, ldq, q_group_stride, ldo);
  if (!aligned16(kc) || !aligned16(vc)) return fail(nullptr, AIGV_ERR_ARG, "%s: the caches must be 16-byte aligned", op);
  const int64_t need = aigv_op_attention_decode_ws_floats(n_seq, n_kv, g, cap);
  if (ws_floats < need) return fail(nullptr, AIGV_ERR_ARG, "%s: workspace of %lld floats, needs %lld", op, (long long)ws_floats, (long long)need);
  if (key_drop) {
    if ((uintptr_t)key_drop & 7) return fail(nullptr, AIGV_ERR_ARG, "%s: key_drop must be 8-byte aligned", op);
    if (ld_drop < (max_kv_len + 63) / 64)
      return fail(nullptr, AIGV_ERR_ARG, "%s: ld_drop = %d is below ceil(max_kv_len / 64) = %d words per sequence", op, ld_drop, (max_kv_len + 63) / 64);
  }
  HIPCHK(nullptr, aigv_launch_attention_decode((const bf16_t*)q, ldq, q_group_stride, (const bf16_t*)kc, (const bf16_t*)vc, kv_lens, cap, (bf16_t*)o,
                                               ldo, n_seq, n_kv, g, head_dim, post_div, max_kv_len, ws, (hipStream_t)stream, key_drop, ld_drop));
  return 0;
}

int aigv_op_attention_decode(const void* q, int ldq, int q_group_stride, const void* kc, const void* vc, const int32_t* kv_lens, int cap,
                             void* o, int ldo, int n_seq, int n_kv, int g, int head_dim, float post_div, int max_kv_len, float* ws,
                             int64_t ws_floats, void* stream) {
  return attention_decode_op("aigv_op_attention_decode", q, ldq, q_group_stride, kc, vc, kv_lens, cap, o, ldo, n_seq, n_kv, g, head_dim, post_div, max_kv_len, ws,
                             ws_floats, nullptr, 0, stream);
}

// aigv_op_attention_decode under a key-drop mask (aigv_launch_attention_decode's key_drop; null: the same call as aigv_op_attention_decode)
int aigv_op_attention_decode_drop(const void* q, int ldq, int q_group_stride, const void* kc, const void* vc, const int32_t* kv_lens, int cap,
                                  void* o, int ldo, int n_seq, int n_kv, int g, int head_dim, float post_div, int max_kv_len, float* ws,
                                  int64_t ws_floats, const uint64_t* key_drop, int ld_drop, void* stream) {
  return attention_decode_op("aigv_op_attention_decode_drop", q, ldq, q_group_stride, kc, vc, kv_lens, cap, o, ldo, n_seq, n_kv, g, head_dim, post_div, max_kv_len,
                             ws, ws_floats, key_drop, ld_drop, stream);
}

// shared checks of the RoPE / KV-append GEMVs (bf16 and e4m3 forms)
static int check_rope_kv(const char* op, const void* x, int ldx, int R, const void* W, int ldw, int N, int K, const void* qkv, int ldo,
                         const int32_t* pos, const int32_t* seq, const void* cos, const void* sin, const void* kc, const void* vc, int g,
                         int n_kv, int cap, int p) {
  if (!x || !W || !qkv || !pos || !seq || !cos || !sin || !kc || !vc) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (g < 1 || g > 8 || n_kv < 1 || N != n_kv * (g + 2) * 128)
    return fail(nullptr, AIGV_ERR_ARG, "%s: N = %d is not n_kv (%d) x (g (%d) + 2) x 128 with g in 1..8", op, N, n_kv, g);
  if (p != 1 && p != 2 && p != 4) return fail(nullptr, AIGV_ERR_ARG, "%s: p must be 1, 2 or 4, got %d", op, p);
  if (R < 1 || R > (p == 1 ? 64 : 16 / p)) return fail(nullptr, AIGV_ERR_ARG, "%s: R = %d rows outside 1..%d for p = %d", op, R, p == 1 ? 64 : 16 / p, p);
  if (K < 128 * p || K % (128 * p)) return fail(nullptr, AIGV_ERR_ARG, "%s: K = %d is not a multiple of %d", op, K, 128 * p);
  if (cap < 1 || cap > AIGV_MAX_KV_CAPACITY) return fail(nullptr, AIGV_ERR_ARG, "%s: cap = %d outside 1..%d", op, cap, AIGV_MAX_KV_CAPACITY);
  if (ldx < K || ldx % 8 || ldo < N || ldo % 4) return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ldx %d, ldo %d)", op, ldx, ldo);
  if (!aligned16(x) || !aligned16(W) || !aligned16(kc) || !aligned16(vc) || ((uintptr_t)qkv & 7) || ((uintptr_t)cos & 7) || ((uintptr_t)sin & 7))
    return fail(nullptr, AIGV_ERR_ARG, "%s: misaligned operand", op);
  return 0;
}

int aigv_op_skinny_rope_kv(const void* x, int ldx, int R, const void* W, int ldw, int N, int K, void* qkv, int ldo, const int32_t* pos,
                           const int32_t* seq, const void* cos, const void* sin, void* kc, void* vc, int g, int n_kv, int cap,
                           const void* norm_w, float eps, int p, void* stream) {
  const char* op = "aigv_op_skinny_rope_kv";
  TRY(check_rope_kv(op, x, ldx, R, W, ldw, N, K, qkv, ldo, pos, seq, cos, sin, kc, vc, g, n_kv, cap, p));
  if (ldw < K || ldw % 8) return fail(nullptr, AIGV_ERR_ARG, "%s: bad ldw %d", op, ldw);
  if (norm_w && (R > 4 || !aigv_skinny_norm_fusable(K) || !aligned16(norm_w)))
    return fail(nullptr, AIGV_ERR_ARG, "%s: the fused RMSNorm takes R <= 4 rows (got %d) and K = 4096 or 6144 (got %d)", op, R, K);
  HIPCHK(nullptr, aigv_launch_skinny_rope_kv((const bf16_t*)x, ldx, R, (const bf16_t*)W, ldw, N, K, (bf16_t*)qkv, ldo, pos, seq, (const bf16_t*)cos,
                                             (const bf16_t*)sin, (bf16_t*)kc, (bf16_t*)vc, g, n_kv, cap, 128, (hipStream_t)stream,
                                             (const bf16_t*)norm_w, eps, p));
  return 0;
}

int aigv_op_skinny_swiglu_normed(const void* x, int ldx, int R, const void* W, int ldw, int N, int K, void* out, int ldo,
                                 const void* norm_w, float eps, int p, void* stream) {
  const char* op = "aigv_op_skinny_swiglu_normed";
  if (!x || !W || !out || !norm_w) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand (norm_w is required)", op);
  if (R < 1 || R > 4 || !aigv_skinny_norm_fusable(K))
    return fail(nullptr, AIGV_ERR_ARG, "%s: takes 1..4 rows (got %d) and K = 4096 or 6144 (got %d)", op, R, K);
  if (p != 1 && p != 2 && p != 4) return fail(nullptr, AIGV_ERR_ARG, "%s: p must be 1, 2 or 4, got %d", op, p);
  if (N < 32 || N % 32) return fail(nullptr, AIGV_ERR_ARG, "%s: N = %d is not a multiple of 32", op, N);
  if (ldx < K || ldx % 8 || ldw < K || ldw % 8 || ldo < N / 2 || ldo % 4)
    return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ldx %d, ldw %d, ldo %d)", op, ldx, ldw, ldo);
  if (!aligned16(x) || !aligned16(W) || !aligned16(norm_w) || ((uintptr_t)out & 7)) return fail(nullptr, AIGV_ERR_ARG, "%s: misaligned operand", op);
  HIPCHK(nullptr, aigv_launch_skinny_swiglu_normed((const bf16_t*)x, ldx, R, (const bf16_t*)W, ldw, N, K, (bf16_t*)out, ldo, (const bf16_t*)norm_w, eps,
                                                   (hipStream_t)stream, p));
  return 0;
}

int aigv_op_skinny_rope_kv_fp8(const void* x, int ldx, int R, const void* W_e4m3, int ldw, const float* w_scale, int N, int K, void* qkv,
                               int ldo, const int32_t* pos, const int32_t* seq, const void* cos, const void* sin, void* kc, void* vc, int g,
                               int n_kv, int cap, const void* norm_w, float eps, int p, void* stream) {
  const char* op = "aigv_op_skinny_rope_kv_fp8";
  TRY(check_rope_kv(op, x, ldx, R, W_e4m3, ldw, N, K, qkv, ldo, pos, seq, cos, sin, kc, vc, g, n_kv, cap, p));
  if (!w_scale || ((uintptr_t)w_scale & 15)) return fail(nullptr, AIGV_ERR_ARG, "%s: w_scale missing or misaligned", op);
  if (ldw < K || ldw % 16) return fail(nullptr, AIGV_ERR_ARG, "%s: bad ldw %d (bytes, a multiple of 16)", op, ldw);
  if (!norm_w || R > 4 || !aigv_skinny_fp8_supported(K, true) || !aligned16(norm_w))
    return fail(nullptr, AIGV_ERR_ARG, "%s: needs norm_w, R <= 4 rows (got %d) and K = 4096 or 6144 (got %d)", op, R, K);
  const AigvRopeKv rk{pos, seq, (const bf16_t*)cos, (const bf16_t*)sin, (bf16_t*)kc, (bf16_t*)vc, g, n_kv, cap};
  hipError_t e = aigv_launch_skinny_fp8((const bf16_t*)x, ldx, R, (const uint8_t*)W_e4m3, ldw, w_scale, N, K, nullptr, 0, (bf16_t*)qkv, ldo, SK_ROPE_KV, &rk,
                                        (const bf16_t*)norm_w, eps, p, (hipStream_t)stream);
  if (e != hipSuccess)
    return fail(nullptr, e == hipErrorInvalidValue ? AIGV_ERR_ARG : AIGV_ERR_HIP, "%s (R=%d N=%d K=%d p=%d): %s", op, R, N, K, p, hipGetErrorString(e));
  return 0;
}

// ---- the score head and the row kernels of the passes, one by one (test entry points): every argument is checked here, before any HIP call ----
// The chain as aigv_launch_score_head splits it: layers with fan-in % 128 == 0 and fan-out % 4 == 0 run on the skinny GEMM, from the first
// layer that is not such a layer on everything runs in the tail kernel (dims <= 1024 there); the last layer is always a tail layer.
// (rows: every row the call runs = what the scratch is sized by; B: the rows of one guarded slice)
static int score_head_op_args(const char* op, const void* x, int ldx, int B, int64_t rows, int n_layers, const int32_t* dims_host, const void* const* w_dev,
                              const void* const* b_dev, void* scratch, int64_t scratch_bytes, float* score, ScoreHeadArgs* out) {
  if (!x || !dims_host || !w_dev || !b_dev || !scratch || !score) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (B < 1 || B > 64) return fail(nullptr, AIGV_ERR_ARG, "%s: B = %d outside 1..64", op, B);
  if (n_layers < 1 || n_layers > 8) return fail(nullptr, AIGV_ERR_ARG, "%s: n_layers = %d outside 1..8", op, n_layers);
  int maxd = 0;
  for (int i = 0; i <= n_layers; ++i) {
    if (dims_host[i] < 1 || dims_host[i] > (1 << 20)) return fail(nullptr, AIGV_ERR_ARG, "%s: dims[%d] = %d outside 1..%d", op, i, dims_host[i], 1 << 20);
    maxd = dims_host[i] > maxd ? dims_host[i] : maxd;
  }
  if (ldx < dims_host[0]) return fail(nullptr, AIGV_ERR_ARG, "%s: ldx = %d below dims[0] = %d", op, ldx, dims_host[0]);
  const int64_t need = (int64_t)3 * rows * maxd * (int64_t)sizeof(bf16_t);
  if (scratch_bytes < need) return fail(nullptr, AIGV_ERR_ARG, "%s: scratch of %lld bytes, needs %lld", op, (long long)scratch_bytes, (long long)need);
  int L = 0;
  while (L < n_layers && dims_host[L] % 128 == 0 && dims_host[L + 1] % 4 == 0) ++L;
  if (L == n_layers)
    return fail(nullptr, AIGV_ERR_ARG, "%s: no tail layer: the last layer (fan-out %d) must have a fan-in that is no multiple of 128 or a fan-out that is no multiple of 4", op,
                dims_host[n_layers]);
  for (int i = L; i <= n_layers; ++i)
    if (dims_host[i] > 1024) return fail(nullptr, AIGV_ERR_ARG, "%s: tail dim dims[%d] = %d above 1024 (the tail starts at layer %d)", op, i, dims_host[i], L);
  if (L > 0 && (!aligned16(scratch) || (rows * maxd) % 8))
    return fail(nullptr, AIGV_ERR_ARG, "%s: scratch must be 16-byte aligned and B * max(dims) = %lld a multiple of 8 for the GEMM layers", op, (long long)rows * maxd);
  ScoreHeadArgs a{};
  a.x = (const bf16_t*)x; a.ldx = ldx; a.B = B; a.n_layers = n_layers; a.score = score;
  for (int i = 0; i <= n_layers; ++i) a.dims[i] = dims_host[i];
  for (int i = 0; i < n_layers; ++i) {
    if (!w_dev[i] || !b_dev[i]) return fail(nullptr, AIGV_ERR_ARG, "%s: null weight or bias of layer %d", op, i);
    if (i < L && !aligned16(w_dev[i])) return fail(nullptr, AIGV_ERR_ARG, "%s: the weight of GEMM layer %d must be 16-byte aligned", op, i);
    a.w[i] = (const bf16_t*)w_dev[i]; a.b[i] = (const bf16_t*)b_dev[i];
  }
  *out = a;
  return 0;
}

int aigv_op_score_head(const void* x, int ldx, int B, int n_layers, const int32_t* dims_host, const void* const* w_dev, const void* const* b_dev,
                       void* scratch, int64_t scratch_bytes, float* score, void* stream) {
  ScoreHeadArgs a{};
  TRY(score_head_op_args("aigv_op_score_head", x, ldx, B, B, n_layers, dims_host, w_dev, b_dev, scratch, scratch_bytes, score, &a));
  HIPCHK(nullptr, aigv_launch_score_head(a, (bf16_t*)scratch, (hipStream_t)stream));
  return 0;
}

int aigv_op_score_head_groups(const void* x, int ldx, int G, int64_t group_stride, int B, int n_layers, const int32_t* dims_host,
                              const void* const* w_dev, const void* const* b_dev, void* scratch, int64_t scratch_bytes, float* score, void* stream) {
  const char* op = "aigv_op_score_head_groups";
  if (G < 1 || (B >= 1 && (int64_t)G * B > 4096)) return fail(nullptr, AIGV_ERR_ARG, "%s: G = %d groups of B = %d rows: needs G >= 1 and G * B <= 4096", op, G, B);
  if (group_stride < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: group_stride = %lld must not be negative", op, (long long)group_stride);
  ScoreHeadArgs a{};
  TRY(score_head_op_args(op, x, ldx, B, (int64_t)G * std::max(B, 1), n_layers, dims_host, w_dev, b_dev, scratch, scratch_bytes, score, &a));
  HIPCHK(nullptr, aigv_launch_score_head_groups(a, G, (size_t)group_stride, (bf16_t*)scratch, (hipStream_t)stream));
  return 0;
}

int aigv_op_rmsnorm_quant_fp8(const void* x, int ldx, const void* w, void* q_e4m3, int ldq, float* row_scale, int rows, int H, float eps, void* stream) {
  const char* op = "aigv_op_rmsnorm_quant_fp8";
  if (!x || !w || !q_e4m3 || !row_scale) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (rows < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: rows = %d must not be negative", op, rows);
  if (H < 8 || H % 8 || H > 16384) return fail(nullptr, AIGV_ERR_ARG, "%s: H = %d is not a multiple of 8 in 8..16384", op, H);
  if (ldx < H || ldx % 8 || ldq < H || ldq % 8) return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ldx %d, ldq %d: multiples of 8, >= H)", op, ldx, ldq);
  if (!aligned16(x) || !aligned16(w) || ((uintptr_t)q_e4m3 & 7)) return fail(nullptr, AIGV_ERR_ARG, "%s: misaligned operand", op);
  HIPCHK(nullptr, aigv_launch_rmsnorm_quant_fp8((const bf16_t*)x, ldx, (const bf16_t*)w, (uint8_t*)q_e4m3, ldq, row_scale, rows, H, eps, (hipStream_t)stream));
  return 0;
}

int aigv_op_rope_slots(void* qkv, int ld, const int32_t* pos, const void* cos, const void* sin, int tokens, int first_rot, int n_rot, int slots,
                       int n_groups, int head_dim, void* stream) {
  const char* op = "aigv_op_rope_slots";
  if (!qkv || !pos || !cos || !sin) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (tokens < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: tokens = %d must not be negative", op, tokens);
  if (head_dim < 16 || head_dim % 16) return fail(nullptr, AIGV_ERR_ARG, "%s: head_dim = %d is not a positive multiple of 16", op, head_dim);
  if (n_groups < 1 || slots < 1 || first_rot < 0 || n_rot < 1 || (int64_t)first_rot + n_rot > slots)
    return fail(nullptr, AIGV_ERR_ARG, "%s: needs n_groups (%d) >= 1, n_rot (%d) >= 1 and 0 <= first_rot (%d), first_rot + n_rot <= slots (%d)", op, n_groups, n_rot,
                first_rot, slots);
  if (ld % 8 || (int64_t)ld < (int64_t)n_groups * slots * head_dim)
    return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ld %d, needs a multiple of 8 and >= n_groups slots head_dim)", op, ld);
  if (!aligned16(qkv) || !aligned16(cos) || !aligned16(sin)) return fail(nullptr, AIGV_ERR_ARG, "%s: qkv and the tables must be 16-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_rope((bf16_t*)qkv, ld, pos, (const bf16_t*)cos, (const bf16_t*)sin, tokens, n_rot, slots, n_groups, head_dim, (hipStream_t)stream,
                                   first_rot));
  return 0;
}

int aigv_op_embed(const int64_t* ids, const int32_t* slot, const void* emb, const void* vis, const void* motion, int n_vis, void* out, int tokens, int H,
                  void* stream) {
  const char* op = "aigv_op_embed";
  if (!ids || !slot || !emb || !out) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (tokens < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: tokens = %d must not be negative", op, tokens);
  if (H < 8 || H % 8) return fail(nullptr, AIGV_ERR_ARG, "%s: H = %d is not a positive multiple of 8", op, H);
  if (n_vis < 0 || (n_vis > 0 && !vis)) return fail(nullptr, AIGV_ERR_ARG, "%s: n_vis = %d needs a visual table (and must not be negative)", op, n_vis);
  if (!aligned16(emb) || !aligned16(vis) || !aligned16(motion) || !aligned16(out)) return fail(nullptr, AIGV_ERR_ARG, "%s: the tables and out must be 16-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_embed(ids, slot, (const bf16_t*)emb, (const bf16_t*)vis, (const bf16_t*)motion, n_vis, (bf16_t*)out, tokens, H, (hipStream_t)stream));
  return 0;
}

int aigv_op_seqpos(const int32_t* cu_host, int n_seq, const int32_t* pos_offset_host, int32_t* pos, int32_t* seq, int32_t* cu_dev, int tokens, void* stream) {
  const char* op = "aigv_op_seqpos";
  if (!cu_host || !pos || !seq || !cu_dev) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (n_seq < 1 || n_seq > AIGV_SMALL_INTS / 2 - 1) return fail(nullptr, AIGV_ERR_ARG, "%s: n_seq = %d outside 1..%d", op, n_seq, AIGV_SMALL_INTS / 2 - 1);
  if (tokens < 1 || cu_host[0] != 0 || cu_host[n_seq] != tokens) return fail(nullptr, AIGV_ERR_ARG, "%s: needs cu[0] = 0 and cu[n_seq] = tokens = %d >= 1", op, tokens);
  for (int b = 0; b < n_seq; ++b)
    if (cu_host[b + 1] < cu_host[b]) return fail(nullptr, AIGV_ERR_ARG, "%s: cu decreases at sequence %d", op, b);
  HIPCHK(nullptr, aigv_launch_seqpos(cu_host, n_seq, pos, seq, cu_dev, tokens, (hipStream_t)stream, pos_offset_host));
  return 0;
}

// shared checks of the row movers: rows of H bf16 in 16-byte chunks
static int check_rows(const char* op, const void* a, const void* b, const void* idx, bool need_idx, int n, int H, int ld) {
  if (!a || !b || (need_idx && !idx)) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (n < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: %d rows: must not be negative", op, n);
  if (H < 8 || H % 8) return fail(nullptr, AIGV_ERR_ARG, "%s: H = %d is not a positive multiple of 8", op, H);
  if (ld < H || ld % 8) return fail(nullptr, AIGV_ERR_ARG, "%s: bad leading dimension (ld %d, needs a multiple of 8 and >= H = %d)", op, ld, H);
  if (!aligned16(a) || !aligned16(b)) return fail(nullptr, AIGV_ERR_ARG, "%s: the row buffers must be 16-byte aligned", op);
  return 0;
}

// dst[i, :H] = src[idx[i] * ld ..] for i < n (dst is dense: leading dimension H)
int aigv_op_gather_rows(const void* src, int ld, const int32_t* idx, int n, void* dst, int H, void* stream) {
  TRY(check_rows("aigv_op_gather_rows", src, dst, idx, true, n, H, ld));
  HIPCHK(nullptr, aigv_launch_gather_rows((const bf16_t*)src, ld, idx, n, (bf16_t*)dst, H, (hipStream_t)stream));
  return 0;
}

// raw[i, :H] = src[idx[i] * ld ..] and normed[i, :H] = RMSNorm of that row under w, for i < n (raw and normed are dense): the depth lens' tap
int aigv_op_lens_tap(const void* src, int ld, const int32_t* idx, int n, const void* w, void* raw, void* normed, int H, float eps, void* stream) {
  const char* op = "aigv_op_lens_tap";
  TRY(check_rows(op, src, raw, idx, true, n, H, ld));
  if (!w || !normed) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (H > 16384) return fail(nullptr, AIGV_ERR_ARG, "%s: H = %d above 16384", op, H);
  if (!aligned16(w) || !aligned16(normed)) return fail(nullptr, AIGV_ERR_ARG, "%s: the row buffers must be 16-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_lens_tap((const bf16_t*)src, ld, idx, n, (const bf16_t*)w, (bf16_t*)raw, (bf16_t*)normed, H, eps, (hipStream_t)stream));
  return 0;
}

// dst[idx[i] * ld ..] = src[i, :H] for i < n (src is dense); duplicate indices must carry identical rows
int aigv_op_scatter_rows(const void* src, const int32_t* idx, int n, void* dst, int ld, int H, void* stream) {
  TRY(check_rows("aigv_op_scatter_rows", src, dst, idx, true, n, H, ld));
  HIPCHK(nullptr, aigv_launch_scatter_rows((const bf16_t*)src, idx, n, (bf16_t*)dst, ld, H, (hipStream_t)stream));
  return 0;
}

// One launch of the activation-patching row copy (aigv_stream_capture_arm / aigv_stream_patch_arm), as a pass of T rows and n_depths armed layers makes
// it for its layer `depth` of the window: rows_host - checked as the pass checks them - go to idx_dev (DEVICE int32 [n]) as kernel arguments, then rows
// idx[i] of `stream_rows` (leading dimension ld) are copied to (to_stream = 0) or overwritten from (to_stream = 1) side[(i * n_depths + depth) * H ..]
int aigv_op_stream_rows(void* stream_rows, int ld, int T, const int32_t* rows_host, int n, int32_t* idx_dev, void* side, int n_depths, int depth, int H,
                        int to_stream, void* stream) {
  const char* op = "aigv_op_stream_rows";
  TRY(check_rows(op, stream_rows, side, rows_host, true, n, H, ld));
  if (!idx_dev) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (H > 16384) return fail(nullptr, AIGV_ERR_ARG, "%s: H = %d above 16384", op, H);
  if (T < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: T = %d rows: must not be negative", op, T);
  if (n_depths < 1 || depth < 0 || depth >= n_depths) return fail(nullptr, AIGV_ERR_ARG, "%s: depth %d outside the window of %d depths", op, depth, n_depths);
  TRY(stream_rows_check(nullptr, op, rows_host, n, T, 0, n_depths, n_depths));
  HIPCHK(nullptr, aigv_launch_write_ints(rows_host, n, idx_dev, (hipStream_t)stream));
  HIPCHK(nullptr, aigv_launch_stream_rows((bf16_t*)stream_rows, ld, idx_dev, n, (bf16_t*)side, n_depths, depth, H, to_stream != 0, (hipStream_t)stream));
  return 0;
}

// One launch of the head-rows kernel (aigv_head_capture_arm / aigv_head_patch_arm / aigv_head_scale_arm), as a pass of T rows makes it for slice `layer` of
// a window of n_layers layers: rows_host - checked as the pass checks them - go to idx_dev (DEVICE int32 [n]) as kernel arguments; mode 0 copies the
// selected heads of rows idx[i] of `ao` (leading dimension ld, H = n_heads * D) to side[(i * n_layers + layer) * H ..], mode 1 overwrites them from
// there, mode 2 scales them by scale_host[h] (HOST float [n_heads]; side and n_layers / layer unused; rows_host null: rows 0 .. T - 1, idx_dev unused)
int aigv_op_head_rows(void* ao, int ld, int T, const int32_t* rows_host, int n, int32_t* idx_dev, void* side, int n_layers, int layer, int n_heads, int D, int mode,
                      uint64_t head_bits, const float* scale_host, void* stream) {
  const char* op = "aigv_op_head_rows";
  if (mode != HEAD_CAPTURE && mode != HEAD_PATCH && mode != HEAD_SCALE) return fail(nullptr, AIGV_ERR_ARG, "%s: mode %d is none of 0 (capture), 1 (patch), 2 (scale)", op, mode);
  const bool scale = mode == HEAD_SCALE, every = scale && !rows_host;
  if (n_heads < 1 || n_heads > AIGV_MAX_HEAD_BITS) return fail(nullptr, AIGV_ERR_ARG, "%s: %d heads outside 1..%d, what a head mask holds", op, n_heads, AIGV_MAX_HEAD_BITS);
  if (D != 64 && D != 128) return fail(nullptr, AIGV_ERR_ARG, "%s: head dimension %d is neither 64 nor 128", op, D);
  if (T < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: T = %d rows: must not be negative", op, T);
  if (every) n = T;
  TRY(check_rows(op, ao, scale ? ao : side, rows_host, !every, n, n_heads * D, ld));
  if (!every && !idx_dev) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (scale) {
    if (!scale_host) return fail(nullptr, AIGV_ERR_ARG, "%s: null scale table", op);
    for (int h = 0; h < n_heads; ++h) if (scale_host[h] != scale_host[h]) return fail(nullptr, AIGV_ERR_ARG, "%s: scale[%d] is NaN", op, h);
    n_layers = 1; layer = 0;
  }
  if (n_layers < 1 || layer < 0 || layer >= n_layers) return fail(nullptr, AIGV_ERR_ARG, "%s: layer %d outside the window of %d layers", op, layer, n_layers);
  if (!every) {
    TRY(stream_rows_check(nullptr, op, rows_host, n, T, 0, n_layers, n_layers));
    HIPCHK(nullptr, aigv_launch_write_ints(rows_host, n, idx_dev, (hipStream_t)stream));
  }
  HIPCHK(nullptr, aigv_launch_head_rows((bf16_t*)ao, ld, every ? nullptr : idx_dev, n, (bf16_t*)side, n_layers, layer, n_heads, D, mode, head_bits, scale_host, (hipStream_t)stream));
  return 0;
}

// One launch of the neuron-rows kernel (aigv_neuron_capture_arm / aigv_neuron_patch_arm / aigv_neuron_scale_arm), as a pass of T rows makes it for slice
// `layer` of a window of n_layers layers on act [T][ld] of I columns.  rows_host (checked as the pass checks them; null: rows 0 .. T - 1) go to idx_dev,
// sidx_host (null: side row i; else n side-row numbers inside [0, n_side)) to sidx_dev, cols_host (null: the dense form; else m columns, strictly ascending
// inside [0, I)) to cols_dev, factors_host (the sparse scale: m floats, no NaN) to factors_dev - all as kernel arguments.  mode 0 copies the selected
// columns of the rows to side[(si * n_layers + layer) * W ..] (W = I, or m in the sparse form), mode 1 overwrites them from there, mode 2 scales them by
// dense_factor (dense) or factors_host[j] (sparse); side, the side rows and n_layers / layer are then unused
int aigv_op_neuron_rows(void* act, int ld, int T, const int32_t* rows_host, int n, int32_t* idx_dev, const int32_t* sidx_host, int32_t* sidx_dev, int n_side, void* side,
                        int n_layers, int layer, int I, const int32_t* cols_host, int m, int32_t* cols_dev, int mode, const float* factors_host, float* factors_dev,
                        float dense_factor, void* stream) {
  const char* op = "aigv_op_neuron_rows";
  if (mode != NEURON_CAPTURE && mode != NEURON_PATCH && mode != NEURON_SCALE) return fail(nullptr, AIGV_ERR_ARG, "%s: mode %d is none of 0 (capture), 1 (patch), 2 (scale)", op, mode);
  const bool scale = mode == NEURON_SCALE, every = !rows_host, sparse = cols_host != nullptr;
  if (T < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: T = %d rows: must not be negative", op, T);
  if (every) n = T;
  TRY(check_rows(op, act, scale ? act : side, rows_host, !every, n, I, ld));
  if (!every && !idx_dev) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (scale) { n_layers = 1; layer = 0; sidx_host = nullptr; }
  if (n_layers < 1 || layer < 0 || layer >= n_layers) return fail(nullptr, AIGV_ERR_ARG, "%s: layer %d outside the window of %d layers", op, layer, n_layers);
  if (sparse) {
    if (m < 0 || m > I) return fail(nullptr, AIGV_ERR_ARG, "%s: %d columns outside 0..I = %d", op, m, I);   // (the arm calls' cap is their tables': the op's lists are the caller's)
    if (m > 0 && !cols_dev) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
    for (int j = 0; j < m; ++j) {
      if (cols_host[j] < 0 || cols_host[j] >= I) return fail(nullptr, AIGV_ERR_ARG, "%s: column %d (entry %d) outside 0..%d", op, cols_host[j], j, I - 1);
      if (j && cols_host[j] <= cols_host[j - 1]) return fail(nullptr, AIGV_ERR_ARG, "%s: columns not strictly ascending at entry %d", op, j);
    }
    if (scale) {
      if (!factors_host || (m > 0 && !factors_dev)) return fail(nullptr, AIGV_ERR_ARG, "%s: null factor list", op);
      for (int j = 0; j < m; ++j) if (factors_host[j] != factors_host[j]) return fail(nullptr, AIGV_ERR_ARG, "%s: factor %d is NaN", op, j);
    }
  } else {
    m = 0;
    if (scale && dense_factor != dense_factor) return fail(nullptr, AIGV_ERR_ARG, "%s: the factor is NaN", op);
  }
  if (sidx_host) {
    if (!sidx_dev) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
    for (int i = 0; i < n; ++i) if (sidx_host[i] < 0 || sidx_host[i] >= n_side) return fail(nullptr, AIGV_ERR_ARG, "%s: side row %d (entry %d) outside 0..%d", op, sidx_host[i], i, n_side - 1);
  }
  hipStream_t s = (hipStream_t)stream;
  if (!every) {
    TRY(stream_rows_check(nullptr, op, rows_host, n, T, 0, n_layers, n_layers));
    HIPCHK(nullptr, aigv_launch_write_ints(rows_host, n, idx_dev, s));
  }
  if (sidx_host) HIPCHK(nullptr, aigv_launch_write_ints(sidx_host, n, sidx_dev, s));
  if (sparse && m > 0) HIPCHK(nullptr, aigv_launch_write_ints(cols_host, m, cols_dev, s));
  if (sparse && scale && m > 0) HIPCHK(nullptr, aigv_launch_write_ints((const int32_t*)factors_host, m, (int32_t*)factors_dev, s));
  HIPCHK(nullptr, aigv_launch_neuron_rows((bf16_t*)act, ld, every ? nullptr : idx_dev, sidx_host ? sidx_dev : nullptr, n, (bf16_t*)side, n_layers, layer, I, sparse ? cols_dev : nullptr, m,
                                          mode, sparse ? factors_dev : nullptr, dense_factor, s));
  return 0;
}

// x[f * tokens_per_frame, :H] = cls_pos[:H] for f < n_frames (x is dense [n_frames * tokens_per_frame, H])
int aigv_op_cls_rows(const void* cls_pos, void* x, int n_frames, int tokens_per_frame, int H, void* stream) {
  const char* op = "aigv_op_cls_rows";
  TRY(check_rows(op, cls_pos, x, nullptr, false, n_frames, H, H));
  if (tokens_per_frame < 1) return fail(nullptr, AIGV_ERR_ARG, "%s: tokens_per_frame = %d must be positive", op, tokens_per_frame);
  HIPCHK(nullptr, aigv_launch_cls_rows((const bf16_t*)cls_pos, (bf16_t*)x, n_frames, tokens_per_frame, H, (hipStream_t)stream));
  return 0;
}

// dst[0..n) (DEVICE int32) = host[0..n), passed as kernel arguments in chunks of 256
int aigv_op_write_ints(const int32_t* host, int n, int32_t* dst, void* stream) {
  const char* op = "aigv_op_write_ints";
  if (n < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: n = %d must not be negative", op, n);
  if (n > 0 && (!host || !dst)) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  HIPCHK(nullptr, aigv_launch_write_ints(host, n, dst, (hipStream_t)stream));
  return 0;
}

int aigv_op_frame_ingest(const void* hwc_u8, int n_frames, int height, int width, const float* mean, const float* stdv,
                         void* out_nchw, void* stream) {
  const char* op = "aigv_op_frame_ingest";
  if (n_frames < 0) return fail(nullptr, AIGV_ERR_ARG, "%s: %d frames: must not be negative", op, n_frames);
  if (height < 1 || width < 1 || height > 16384 || width > 16384) return fail(nullptr, AIGV_ERR_ARG, "%s: %d x %d frames outside 1..16384", op, height, width);
  if ((height * width) % 4) return fail(nullptr, AIGV_ERR_ARG, "%s: height * width = %d is not a multiple of 4", op, height * width);
  if (!mean || !stdv) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (n_frames == 0) return 0;   // (an empty batch has no buffers)
  if (!hwc_u8 || !out_nchw) return fail(nullptr, AIGV_ERR_ARG, "%s: null operand", op);
  if (((uintptr_t)hwc_u8 & 3) || ((uintptr_t)out_nchw & 7))
    return fail(nullptr, AIGV_ERR_ARG, "%s: the frames must be 4-byte aligned and out_nchw 8-byte aligned", op);
  HIPCHK(nullptr, aigv_launch_frame_ingest((const uint8_t*)hwc_u8, n_frames, height, width, mean, stdv, (bf16_t*)out_nchw,
                                           (hipStream_t)stream));
  return 0;
}

int aigv_op_frame_resize_ingest(const void* hwc_u8, int n_frames, int in_h, int in_w, int out_h, int out_w, const float* mean,
                                const float* stdv, void* tmp_u8, void* out_u8_hwc, void* out_nchw, void* stream) {
  if (!hwc_u8 || !tmp_u8 || (!out_u8_hwc && !out_nchw) || n_frames < 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0 ||
      (out_nchw && (!mean || !stdv)))
    return fail(nullptr, AIGV_ERR_ARG, "aigv_op_frame_resize_ingest: bad argument (frames %d, %dx%d -> %dx%d)", n_frames, in_h, in_w, out_h, out_w);
  if (in_h > 16384 || in_w > 16384 || out_h > 16384 || out_w > 16384)
    return fail(nullptr, AIGV_ERR_ARG, "aigv_op_frame_resize_ingest: sizes above 16384 are not supported");
  // Pillow (12.2, observed against the live package: tests/manual/fuzz_resize.py) runs the VERTICAL pass first for frames more than 100 times taller than wide
  // that shrink vertically - the intermediate uint8 image, and so the result, differs from the horizontal-first order implemented here.  Not a video
  // geometry: refused rather than answered differently from Pillow.
  if (in_w != out_w && in_h != out_h && in_h > out_h && (long)in_h > 100L * in_w)
    return fail(nullptr, AIGV_ERR_ARG, "aigv_op_frame_resize_ingest: %dx%d frames (more than 100 times taller than wide) are not supported: Pillow orders its passes differently there", in_h, in_w);
  HIPCHK(nullptr, aigv_launch_frame_resize_ingest((const uint8_t*)hwc_u8, n_frames, in_h, in_w, out_h, out_w, mean, stdv,
                                                  (uint8_t*)tmp_u8, (uint8_t*)out_u8_hwc, (bf16_t*)out_nchw, (hipStream_t)stream));
  return 0;
}

// The InternViT attention map's two kernels on plain pointers, no context (tests; vitmap.hip).  Everything is checked before anything is launched.
int aigv_op_vit_attention_map(const void* q, int ldq, const void* k, int ldk, int n_seq, int S, int n_heads, int head_dim, float* out, int per_head,
                              void* stats_scratch, void* stream) {
  const char* op = "aigv_op_vit_attention_map";
  VitMapArgs a{};
  a.q = (const bf16_t*)q; a.ldq = ldq; a.k = (const bf16_t*)k; a.ldk = ldk;
  a.n_seq = n_seq; a.S = S; a.n_heads = n_heads;
  a.post_div = sqrtf((float)(head_dim > 0 ? head_dim : 1));
  a.out = out; a.per_head = per_head ? 1 : 0;
  a.out_frame_stride = (size_t)(per_head ? std::max(n_heads, 0) : 1) * (size_t)std::max(S, 0) * (size_t)std::max(S, 0);
  a.stats = (float2*)stats_scratch;
  if (const char* m = aigv_vit_map_check(a, head_dim)) return fail(nullptr, AIGV_ERR_ARG, "%s: %s", op, m);
  HIPCHK(nullptr, aigv_launch_vit_map(a, head_dim, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
