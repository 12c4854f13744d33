// Internal launcher declarations (C++ side of the library; the public C ABI is include/aigv_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t bf16_t;

// ---- GEMM ---------------------------------------------------------------------------------------
enum GemmEpilogue {
  EPI_STORE = 0,     // C = bf16(acc + bias?)
  EPI_GELU = 1,      // C = bf16(gelu(bf16(acc + bias?)))   erf GELU, common.h gelu_fast
  EPI_LS_RESID = 2,  // C = bf16(resid + bf16(bf16(acc + bias?) * ls))
  EPI_RESID = 3,     // C = bf16(resid + bf16(acc + bias?))
  EPI_SWIGLU = 4,    // W = 16-row interleave of (w1, w3); C[M, N/2] = bf16(bf16(silu(bf16(g))) * bf16(u))
  EPI_PATCH = 5,     // patch-embed: C[m + m/np + 1] = bf16(bf16(acc + bias) + pos[m % np + 1])
  EPI_COUNT = 6,
  EPI_PARTIAL = 6    // internal (split-K tails): fp32 partial sums of K slice blockIdx.y -> part[slice][M][N]
};

struct GemmArgs {
  const bf16_t* A; int lda;     // activations [M, K], row stride lda
  const bf16_t* W; int ldw;     // weights [N, K] (nn.Linear layout), row stride ldw
  bf16_t* C; int ldc;           // output, row stride ldc
  const bf16_t* bias;           // [N] or null
  const bf16_t* ls;             // [N] layer-scale (EPI_LS_RESID)
  const bf16_t* resid; int ldr; // residual [M, N]
  const bf16_t* pos;            // [np+1, N] position table (EPI_PATCH)
  int M, N, K;
  int np;                       // patches per frame (EPI_PATCH)
  float* part;                  // EPI_PARTIAL: fp32 slabs [k_slices][M][N]
  int k_slices;                 // EPI_PARTIAL: grid.y; each slice covers K / k_slices (a multiple of 64)
  // fp8 operands (aigv_launch_gemm256_fp8): A / W hold e4m3 bytes (K, lda, ldw counted in PAIRS of bytes so that the rows are the
  // same 128-byte K-tiles), C = bf16(acc * row_scale[m] * col_scale[n] + bias)
  const float* row_scale;
  const float* col_scale;
  // gemm256 only: the rows of a launch as a table of 128-row HALF tiles, (base row, valid rows 0..128) int32 pairs on the device; row
  // tile i = halves 2i, 2i+1.  M is then only the row count of the buffers (slabs of the split-K form are [k_slices][tiles*256][N]).
  const int32_t* row_tab; int tab_halves;
  // fused body + tail-slice launch (aigv_launch_gemm256_fused): the table continues with fuse_tail_halves tail halves; fuse_body_wg is filled
  // in by the launcher
  int fuse_tail_halves, fuse_body_wg;
  // per-launch tuning selectors (0 = the default; set from the context's / the process's knobs by the dispatcher in dispatch.hip - the kernel files
  // hold no mutable state): order_sel 1 = row groups, 1 + g = groups of g column tiles (0: by weight size); variant_sel 1 + v = schedule
  // variant v of the 256 kernel (0: the shipped one)
  int order_sel, variant_sel;
  int order;                    // gemm256 tile order: 0 = groups of 4 ROW tiles sweep the column tiles (an XCD owns rows), g > 0 = groups of g COLUMN tiles sweep the rows (an XCD owns a slice of W)
};

const char* aigv_gemm_check(const GemmArgs& a, int epi);   // nullptr if the shapes fit the kernel
hipError_t aigv_launch_gemm(const GemmArgs& a, int epi, hipStream_t s);           // 128x128 tile kernel (gemm.hip)
// split-K for latency-bound tails: k_slices x the tiles of the 128 kernel write fp32 slabs, then one pass sums them in a
// fixed order and applies epilogue `epi` (deterministic; ws holds k_slices*M*N floats)
// (tile256: the slices come from the 256x256 kernel - needs N % 256 == 0)
hipError_t aigv_launch_gemm_splitk(const GemmArgs& a, int epi, int k_slices, float* ws, hipStream_t s, bool tile256 = false);
hipError_t aigv_launch_gemm256_partial(const GemmArgs& a, hipStream_t s);   // a.part / a.k_slices filled in
// e4m3 operands on the block-scaled fp8 MFMA (unit block scales; per-row x per-column fp32 scales applied to the accumulator before the
// epilogue proper); epi = STORE, GELU, LS_RESID, RESID or SWIGLU with the bf16 kernel's rounding points
hipError_t aigv_launch_gemm256_fp8(const GemmArgs& a, int epi, hipStream_t s);
hipError_t aigv_launch_gemm256_fp8_partial(const GemmArgs& a, hipStream_t s);   // a.part / a.k_slices filled in; slabs hold scaled sums
hipError_t aigv_launch_gemm_splitk_fp8(const GemmArgs& a, int epi, int k_slices, float* ws, hipStream_t s);
// bf16 rows -> e4m3 bytes + one fp32 scale per row (amax / 448); q = e4m3_rne(x * (448 / amax))
// RMSNorm whose result goes straight to e4m3 rows + row scales (== aigv_launch_rmsnorm then aigv_launch_quant_fp8_rows, bit for bit)
hipError_t aigv_launch_rmsnorm_quant_fp8(const bf16_t* x, int ldx, const bf16_t* w, uint8_t* q, int ldq, float* scale, int rows, int H, float eps,
                                         hipStream_t s);
hipError_t aigv_launch_quant_fp8_rows(const bf16_t* x, int ldx, int rows, int K, uint8_t* q, int ldq, float* scale, hipStream_t s);
bool aigv_gemm256_supported(const GemmArgs& a);
// one launch: the body tiles of a row plan with epilogue `epi` + the split-K slices (fp32 slabs a.part) of its tail tiles; then
// aigv_launch_gemm_finalize over the tail table sums the slabs (the second half of aigv_launch_gemm_splitk)
hipError_t aigv_launch_gemm256_fused(const GemmArgs& a, int epi, hipStream_t s);
hipError_t aigv_launch_gemm_finalize(const GemmArgs& a, int epi, int k_slices, const float* ws, hipStream_t s);
hipError_t aigv_launch_gemm256(const GemmArgs& a, int epi, hipStream_t s);        // 256x256 phase-interleaved kernel
// 256x128 tile, four waves, two co-resident workgroups per CU (gemmco.hip): same bits as the 256 kernel; takes the half-tile table too
bool aigv_gemmco_supported(const GemmArgs& a);
hipError_t aigv_launch_gemmco(const GemmArgs& a, int epi, hipStream_t s);

// ---- attention ------------------------------------------------------------------------------------
// Packed varlen layout: sequence s occupies rows cu[s] .. cu[s+1]-1 of the token-major buffers.
// q/k/v point at column 0 of head 0 of their operand inside a (possibly fused) row:
//   q head hq  at column (hq / g) * q_group_stride + (hq % g) * D        (g = n_heads / n_kv_heads)
//   kv head hk at column hk * kv_head_stride
// (AttnArgsUnmasked: every field but the key-drop pair - the kernel argument of the unmasked kernels, so that their kernarg segment, and with
// it their code, is what it was before AttnArgs gained that pair; AttnArgsKeyDrop: and that pair - the kernel argument of the key-drop kernels,
// what it was before AttnArgs gained the row selector; callers fill an AttnArgs)
struct AttnArgsUnmasked {
  const bf16_t* q; int ldq;
  const bf16_t* k; int ldk;
  const bf16_t* v; int ldv;
  bf16_t* o; int ldo;           // [tokens, n_heads*D]
  const int32_t* cu;            // [n_seq+1] cumulative lengths (device)
  int n_seq, max_len;
  int n_heads, n_kv_heads;
  int q_group_stride, kv_head_stride;
  int kv_len_offset;            // keys that precede the first query row of every sequence (0: plain prefill)
  const int32_t* kv_off;        // per-sequence form of kv_len_offset (device, [n_seq]); overrides it when non-null
  size_t kv_seq_stride;         // 0: K/V rows are packed like the query rows (row0 * ldk); else K/V of sequence s start at
                                // s * kv_seq_stride elements (a KV cache [seq][kv head][capacity][D]: ldk = D, kv_head_stride = cap * D)
  int causal;
  float post_div;               // score = bf16(bf16(q.k) / post_div)  (LLM: sqrt(d); ViT: 1, q is pre-scaled)
  int round_scores;             // != 0: the two bf16 roundings of the line above are applied, as the reference's eager path does; 0: scores stay fp32
  float q_prescale;             // q <- bf16(q * q_prescale)           (ViT: d^-1/2; LLM: 1)
  // RoPE applied to the QUERY rows as they are loaded (same three bf16 roundings as rope_kernel); K must already be rotated.
  // null = queries are used as stored.  rope_pos: position of every packed query row; tables [max_pos, D/2] bf16.
  const int32_t* rope_pos; const bf16_t* rope_cos; const bf16_t* rope_sin;
  int rope_pos_is_row;          // != 0: the position of query row r of a sequence IS kv offset + r (plain prefill / continuation): the kernel computes it
                                // instead of loading rope_pos (one dependent global load fewer in front of the cos / sin rows in every workgroup's prologue)
  int q_tail;                   // > 0: only the last q_tail query rows of every sequence are computed (others left unwritten)
  int uniform_len;              // every sequence has max_len rows (InternViT frames): lets the dispatcher split the query rows between kernels
  // row range of ONE kernel launch (set by aigv_launch_attention when it splits the rows between the two kernels; 0 = no limit):
  int waves;                    // 0 = default (4 waves per workgroup); 4 / 8 forced (A/B: aigv_tune_attention / aigv_ctx_tune)
  int lead_key;                 // != 0: non-causal key counts 64 j + 1 run as full tiles over keys 1.. + key 0 merged in the epilogue (opt-in; attention.hip "lead key")
  int q_begin;                  // the launch computes query rows >= q_begin (a multiple of the workgroup's 128 rows) only; 0 everywhere at present
};
struct AttnArgsKeyDrop : AttnArgsUnmasked {
  // Key drop (causal head_dim 128, and - where the caller asks aigv_attn_check for it - non-causal head_dim 64 / 128; null = no key is dropped, the
  // kernels that have always run): bit j & 63 of word
  // key_drop[seq * ld_drop + (j >> 6)] set = key j of that sequence is invisible to every query row and head.  j is the key's absolute position
  // in its sequence, cached keys first - the packed form and the cache form (kv_off, kv_seq_stride) share the indexing; one word = one 64-key
  // tile.  ld_drop >= ceil((largest key offset + max_len) / 64); with kv_off the caller states that largest offset in kv_len_offset.  A row left
  // without a visible key is written as zeros.  The V rows of dropped keys must be finite (0 x NaN = NaN, as in torch).
  // Non-causal form (InternViT's patch mask, aigv_vit_key_drop_arm): the packed layout only - no kv_off, kv_len_offset, kv_seq_stride, q_tail or drop_rows;
  // ld_drop >= ceil(max_len / 64).  A dropped key is hidden from its own row too.  It runs with the lead key OFF whatever lead_key says (with it the loop's
  // key index is the absolute position minus one and words no longer cover tiles): under a zero mask the output is, bit for bit, that of the unmasked
  // kernel with lead_key = 0, the default - NOT that of the unmasked kernel with the knob on.  Both workgroup sizes (waves) exist.
  const uint64_t* key_drop;     // device
  int ld_drop;                  // words per sequence
};
struct AttnArgs : AttnArgsKeyDrop {
  // Row selector of the key-drop mask (null = every query row is subject to it: the key-drop kernels that have always run): the same word layout,
  // [n_seq][ld_drop], bit i & 63 of word drop_rows[seq * ld_drop + (i >> 6)] set = the query row at position i of that sequence is subject to the
  // mask; a score is hidden iff its key's bit and its row's bit are both set.  Needs key_drop; exists for the packed prefill only (no kv_off, no
  // kv_len_offset), where a row's position is its index in its sequence.  Bits at or past a sequence's length are ignored.
  const uint64_t* drop_rows;    // device
};
// drop_noncausal: the caller asks for the non-causal key-drop form; without it key_drop with causal == 0 (or head_dim 64) is refused as it always was
const char* aigv_attn_check(const AttnArgs& a, int head_dim, bool drop_noncausal = false);
hipError_t aigv_launch_attention(const AttnArgs& a, int head_dim, hipStream_t s);
// decode: one query row per sequence (fused qkv row), KV cache [seq][kv head][cap][D]; split-KV two-pass kernel,
// ws = aigv_attention_decode_ws_floats(...) floats of scratch.  The merge pass holds 16 bytes of LDS per 128-key chunk of the
// capacity: at most AIGV_DECODE_MAX_CHUNKS chunks (= AIGV_MAX_KV_CAPACITY tokens, include/aigv_amd.h)
// key_drop (device, [n_seq][ld_drop] words in AttnArgs::key_drop's layout, 8-byte aligned, ld_drop >= ceil(max_kv_len / 64); null = no key is dropped,
// the kernels that have always run): the masked form of the first pass.  A dropped key's score is never formed from its K row; a 128-key chunk without a
// visible key is written as m = -inf, l = 0, zero sums without a read of K or V, and the merge pass gives it weight 0; a sequence without a visible key is
// written as zeros.  The V rows of dropped keys inside a partly visible chunk must be finite (they are multiplied by an exact 0).  Bits at or past
// kv_lens[seq] are ignored.
constexpr int AIGV_DECODE_KEYS_PER_CHUNK = 128;
constexpr int AIGV_DECODE_MAX_CHUNKS = 2048;
size_t aigv_attention_decode_ws_floats(int n_seq, int n_kv, int g, int cap);
hipError_t aigv_launch_attention_decode(const bf16_t* q, int ldq, int q_group_stride, const bf16_t* kc,
                                        const bf16_t* vc, const int32_t* kv_lens, int cap, bf16_t* o, int ldo,
                                        int n_seq, int n_kv, int g, int head_dim, float post_div, int max_kv_len,
                                        float* ws, hipStream_t s, const uint64_t* key_drop = nullptr, int ld_drop = 0);

// ---- attention probe (attnprobe.hip) ----------------------------------------------------------------
// Where ONE query row of a causal GQA attention looks: out[row][head][seg] = sum of softmax(q . K / post_div) over the keys of segment
// seg, for up to AIGV_MAX_PROBE_ROWS rows per launch.  q: UNROTATED rows of the fused qkv buffer (q head h at column (h / g) *
// q_group_stride + (h % g) * D), rotated by the kernel at the row's position with rope_kernel's arithmetic; K: already rotated, in one of
// AttnArgs' two addressing forms - packed (kv_seq_stride = 0: key j of a sequence is row row0 + j, ldk apart) or the KV cache
// (kv_seq_stride != 0: [seq][kv head][cap][D], ldk = D, kv_head_stride = cap * D; keys [0, off) were cached before the pass, the pass's own
// rows follow).  Scores are fp32 whatever the pass's attention numerics.  seg ids: seg_new[packed row] for the pass's rows,
// seg_cached[seq * ld_cached + j] for cached positions j < off; an id outside [0, n_seg) drops the key from the bins, not from the total.
// Dense form (tok != nullptr, from the same launch): tok[row][head][j] = softmax_j for the key positions j = 0 .. pos of the row's sequence
// (cached keys first), +0.0 for pos < j < ld_tok - the bins' scores, maximum, total and division, so a one-key bin equals its key's value.
// Values form (v and val != nullptr, from the same launch; out and tok keep their bits): val[row][head][s][0..D) = sum over the keys of
// segment s of softmax_j * v_j, s = n_seg collecting the keys outside [0, n_seg) - the head's output split by where it was read from.
#ifndef AIGV_MAX_ATTN_SEGMENTS
#define AIGV_MAX_ATTN_SEGMENTS 64   // = include/aigv_amd.h
#endif
#ifndef AIGV_MAX_PROBE_ROWS
#define AIGV_MAX_PROBE_ROWS 64      // = include/aigv_amd.h
#endif
#ifndef AIGV_MAX_KV_CAPACITY
#define AIGV_MAX_KV_CAPACITY 262144 // = include/aigv_amd.h: the most columns a dense row takes
#endif
struct ProbeRow { int32_t row, row0, seq, off; };   // packed row | first packed row of its sequence | sequence | keys cached in front of the pass
struct ProbeRowTab { ProbeRow r[AIGV_MAX_PROBE_ROWS]; };   // by value: a kernel argument (no copy, no allocation - the pass still captures)
struct ProbeArgs {
  const bf16_t* q; int ldq;
  const bf16_t* k; int ldk;
  int n_heads, n_kv_heads;
  int q_group_stride, kv_head_stride;
  size_t kv_seq_stride;
  float post_div;                        // sqrt(D)
  const bf16_t* rope_cos; const bf16_t* rope_sin;   // [max_pos, D/2]
  const int32_t* seg_new; const int32_t* seg_cached; int ld_cached;
  int n_seg;
  float* out; size_t out_row_stride;     // out[row * out_row_stride + head * n_seg + seg]
  int n_rows;
  ProbeRowTab tab;
  float* tok; int ld_tok; size_t tok_row_stride;   // dense form, or nullptr / 0: tok[row * tok_row_stride + head * ld_tok + j]
  const bf16_t* v; int ldv;              // values form, or nullptr / 0: V in K's addressing form (kv_head_stride, kv_seq_stride; cache: ldv = ldk)
  float* val; size_t val_row_stride;     // val[row * val_row_stride + (head * (n_seg + 1) + seg) * D + c], slot n_seg = the keys outside [0, n_seg)
};
// nullptr if every index the kernel forms stays inside its operand: total_rows = rows of the pass (q, seg_new), max_pos = rows of the RoPE tables
const char* aigv_probe_check(const ProbeArgs& a, int head_dim, int total_rows, int max_pos);
hipError_t aigv_launch_attention_probe(const ProbeArgs& a, int head_dim, hipStream_t s);

// ---- attention flow map (attnmap.hip) ----------------------------------------------------------------
// Where EVERY query row of a causal GQA attention looks, on the matrix cores: rows[t][head][seg] = sum of softmax(q . K / post_div) over the
// keys of segment seg, for all cu[n_seq] packed rows.  Packed layout only: q and K are the probe's packed operands (q UNROTATED, rotated by the
// kernel at the row's position; K rotated), seg one id per packed row, an id outside [0, n_seg) counting for the total only.  Scores and
// weights are fp32 whatever the pass's attention numerics.  seg_out (optional): the fold seg_out[b * seg_out_seq_stride + (head * n_seg + a) *
// n_seg + c] = mean over the query rows of sequence b whose id is a of rows[.][head][c], NaN where a has no row.
constexpr int AIGV_MAP_MAX_SEQS = 127;   // = AIGV_SMALL_INTS / 2 - 1: what one prefill call takes
struct AttnMapArgs {
  const bf16_t* q; int ldq;
  const bf16_t* k; int ldk;
  int n_heads, n_kv_heads;
  int q_group_stride, kv_head_stride;
  float post_div;                        // sqrt(D)
  const bf16_t* rope_cos; const bf16_t* rope_sin;   // [max_pos, D/2], 16-byte aligned
  const int32_t* seg; int n_seg;
  float* rows;                           // [cu[n_seq]][n_heads][n_seg]
  float* seg_out; size_t seg_out_seq_stride;
  int n_seq;
  int32_t cu[AIGV_MAP_MAX_SEQS + 1];     // by value: a kernel argument (no copy, no allocation)
};
// nullptr if every index the two kernels form stays inside its operand: max_pos = rows of the RoPE tables
const char* aigv_attn_map_check(const AttnMapArgs& a, int head_dim, int max_pos);
hipError_t aigv_launch_attention_map(const AttnMapArgs& a, int head_dim, hipStream_t s);

// ---- InternViT attention map (vitmap.hip) ------------------------------------------------------------
// The full, non-causal softmax matrix of every query row of every frame, from the bf16 Q and K of a ViT layer's fused rows.  For frame f,
// head h, query row i, key j, 0 <= i, j < S:
//   acc_ij = the fp32 MFMA accumulation of the exact bf16 products q_i . k_j;  s_ij = acc_ij / sqrtf(D);  m_i = max_j s_ij;
//   e_ij = expf(s_ij - m_i);  total_i = the fp32 sum of the e_ij, in an order fixed by the key index alone;  p_ij = e_ij / total_i
// per head:  out[f * out_frame_stride + (h * S + i) * S + j] = p_ij
// head mean: out[f * out_frame_stride + i * S + j] = (p0_ij + p1_ij + ... in ascending h, starting from +0.0) / n_heads, one fp32 division
// Frames are n_seq runs of S consecutive rows; head h sits at column h * D of a row.  fp32 scores and weights whatever the pass's attention
// numerics; the unscaled bf16 Q (no q_prescale rounding).  stats: [n_seq][n_heads][S] (m, total) pairs, written by the first kernel.
constexpr int AIGV_VIT_MAP_MAX_HEADS = 64, AIGV_VIT_MAP_MAX_FRAMES = 65535, AIGV_VIT_MAP_MAX_ROWS = 32768;
struct VitMapArgs {
  const bf16_t* q; int ldq;
  const bf16_t* k; int ldk;
  int n_seq, S, n_heads;
  float post_div;                        // sqrt(D)
  float* out; size_t out_frame_stride;   // in floats
  int per_head;
  float2* stats;
};
// nullptr if every index the two kernels form stays inside its operand
const char* aigv_vit_map_check(const VitMapArgs& a, int head_dim);
hipError_t aigv_launch_vit_map(const VitMapArgs& a, int head_dim, hipStream_t s);

// ---- row-wise / elementwise ---------------------------------------------------------------------
// LayerNorm over rows of length H (fp32 statistics, bf16 out).
hipError_t aigv_launch_layernorm(const bf16_t* x, int ldx, const bf16_t* w, const bf16_t* b, bf16_t* y, int ldy,
                                 int rows, int H, float eps, hipStream_t s);
// RMSNorm (fp32 normalise -> bf16 -> * weight -> bf16).  row_idx (optional) gathers input rows.
hipError_t aigv_launch_rmsnorm(const bf16_t* x, int ldx, const bf16_t* w, bf16_t* y, int ldy, int rows, int H,
                               float eps, const int32_t* row_idx, hipStream_t s);
// cls drop + pixel-shuffle v2 gather (pre-projector tokens; the frame-DP all-gather payload)
hipError_t aigv_launch_pixel_shuffle(const bf16_t* vit, int grid, int Hv, bf16_t* out, int frames, hipStream_t s);
// im2col for the patch-embed GEMM: frames NCHW bf16 -> [F*g*g, Kp] (k = c*P*P + py*P + px, zero padded)
hipError_t aigv_launch_im2col(const bf16_t* frames, int F, int C, int S, int P, int Kp, bf16_t* out, hipStream_t s);
// x[f*(np+1)] = cls_pos (class token + its position row, precomputed) for every frame
hipError_t aigv_launch_gather_rows(const bf16_t* src, int ld, const int32_t* idx, int n, bf16_t* dst, int H, hipStream_t s);
// the depth lens' tap: raw[i, :H] = src[idx[i] * ld ..] unchanged and normed[i, :H] = RMSNorm(that row) * w with aigv_launch_rmsnorm's bits (raw, normed dense)
hipError_t aigv_launch_lens_tap(const bf16_t* src, int ld, const int32_t* idx, int n, const bf16_t* w, bf16_t* raw, bf16_t* normed, int H, float eps,
                                hipStream_t s);
hipError_t aigv_launch_scatter_rows(const bf16_t* src, const int32_t* idx, int n, bf16_t* dst, int ld, int H, hipStream_t s);   // dst[idx[i]] = src[i]
// activation patching: rows idx[i] (distinct) of `stream` (leading dimension ld) against slice `depth` of a side buffer whose element (i, d) sits at
// side + (i * n_depths + d) * H.  to_stream: stream[idx[i]] = side(i, depth) (the patch), else side(i, depth) = stream[idx[i]] (the capture); a bit
// copy.  H a multiple of 8 in 8..16384, ld a multiple of 8 and >= H, both buffers 16-byte aligned, 0 <= depth < n_depths: else hipErrorInvalidValue
hipError_t aigv_launch_stream_rows(bf16_t* stream, int ld, const int32_t* idx, int n, bf16_t* side, int n_depths, int depth, int H, bool to_stream,
                                   hipStream_t s);
// head knock-out / head patching: rows idx[i] (idx null, HEAD_SCALE only: rows 0 .. n - 1) of the attention output `ao` [.., n_heads * D] (leading
// dimension ld) against slice `layer` of a side buffer whose element (i, l) sits at side + (i * n_layers + l) * n_heads * D.  Only the heads whose bit
// of `heads` is set are read or written.  HEAD_CAPTURE: side = ao; HEAD_PATCH: ao = side (bit copies); HEAD_SCALE: ao = bf16(fp32(ao) * scale[h]) -
// `scale` (HOST, n_heads floats) travels as a kernel argument, `side` is unused.  n_heads in 1..64, D 64 or 128, ld a multiple of 8 and >= n_heads * D,
// the buffers 16-byte aligned, 0 <= layer < n_layers: else hipErrorInvalidValue
#define AIGV_MAX_HEAD_BITS 64
enum { HEAD_CAPTURE = 0, HEAD_PATCH = 1, HEAD_SCALE = 2 };
struct HeadScales { float v[AIGV_MAX_HEAD_BITS]; };
hipError_t aigv_launch_head_rows(bf16_t* ao, int ld, const int32_t* idx, int n, bf16_t* side, int n_layers, int layer, int n_heads, int D, int mode,
                                 uint64_t heads, const float* scale, hipStream_t s);
// MLP neuron knock-out / neuron patching: rows idx[i] (idx null: rows 0 .. n - 1) of the SwiGLU output `act` [.., I] (leading dimension ld) against
// slice `layer` of a side buffer whose element (si, l) sits at side + (si * n_layers + l) * W, si = sidx[i] (sidx null: i).  cols null (m = 0): the dense
// form, W = I, NEURON_SCALE by `dense_factor` (exactly 1: nothing is launched).  cols DEVICE int32 [m], strictly ascending inside [0, I): the sparse form,
// W = m, element j of a side row is column cols[j]; NEURON_SCALE by factors[j] (DEVICE float [m]; exactly 1: the element is not touched).
// NEURON_CAPTURE: side = act; NEURON_PATCH: act = side (bit copies); NEURON_SCALE: act = bf16(fp32(act) * s), `side` and `sidx` unused.  I a multiple of
// 8, ld a multiple of 8 and >= I, the buffers 16-byte aligned, 0 <= layer < n_layers, 0 <= m <= I: else hipErrorInvalidValue
#define AIGV_MAX_NEURON_SEL 4096
enum { NEURON_CAPTURE = 0, NEURON_PATCH = 1, NEURON_SCALE = 2 };
hipError_t aigv_launch_neuron_rows(bf16_t* act, int ld, const int32_t* idx, const int32_t* sidx, int n, bf16_t* side, int n_layers, int layer, int I,
                                   const int32_t* cols, int m, int mode, const float* factors, float dense_factor, hipStream_t s);
hipError_t aigv_launch_cls_rows(const bf16_t* cls_pos, bf16_t* x, int F, int tokens_per_frame, int H, hipStream_t s);
// RoPE in place on the fused qkv rows: per kv group, slots 0..g (q heads and K) are rotated.
// slots [first_rot, first_rot + n_rot) of every group are rotated in place (q heads + K: first_rot 0, n_rot g + 1; K only: g, 1)
hipError_t aigv_launch_rope(bf16_t* qkv, int ld, const int32_t* pos, const bf16_t* cos, const bf16_t* sin,
                            int tokens, int n_rot, int slots, int n_groups, int D, hipStream_t s, int first_rot = 0);
// token embedding + visual/motion scatter: slot[t] < 0 -> tok_emb[ids[t]]; < n_vis -> vis[slot]; else motion
hipError_t aigv_launch_embed(const int64_t* ids, const int32_t* slot, const bf16_t* emb, const bf16_t* vis,
                             const bf16_t* motion, int n_vis, bf16_t* out, int tokens, int H, hipStream_t s);
// skinny (R <= 64) weight-streaming GEMM (head.hip; e4m3 forms: head8.hip; what the two kernels share - slab geometry, K-slice combine, RoPE /
// KV-append epilogue - is skinny_tiles.h) and its epilogues; aigv_launch_skinny_gemm takes SK_STORE (+bias), SK_RESID, SK_SWIGLU, SK_GELU (+bias)
// and SK_LS_RESID
enum { SK_STORE = 0, SK_RESID = 1, SK_SWIGLU = 2, SK_GELU = 3, SK_ARGMAX = 4, SK_RELU = 5, SK_LS_RESID = 6, SK_ROPE_KV = 7, SK_ARGMAX_LSE = 8, SK_ARGMAX_LSE_STORE = 9 };
hipError_t aigv_launch_skinny_gemm(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K,
                                   const bf16_t* bias, const bf16_t* resid, int ldr, bf16_t* out, int ldo, int epi,
                                   hipStream_t s, const bf16_t* ls = nullptr, int p = 1);
// p: 0 = 16-row slabs with FOUR K slices for every row count (the form does not depend on R: batch-invariant bits; aigv_set_gemm_mode 1);
// 1 = 16-row slabs, eight K slices for a one-tile GEMV with at most one slab per CU; 2 / 4 = the sub-slab forms (8 / 4 rows per workgroup and slab, R <= 8 / 4, store / residual / swiglu only):
// same result up to fp32 summation order, 2x / 4x the workgroups - for widths whose 16-row slabs leave CUs unevenly loaded
// e4m3 form of the decode GEMVs (head8.hip; fp8 mode of the InternLM2 linears).  epi: 1 residual, 2 swiglu, 7 wqkv with RoPE + KV append
// (rk); norm_w != null: the RMSNorm in front of the linear is applied by the kernel.  R <= 4 rows; W8 [N][ldw bytes] e4m3, w_scale [N]
struct AigvRopeKv {                            // the RoPE / KV-append arguments of SK_ROPE_KV, bf16 and e4m3 form alike (SKINNY_ROPE_KV_STORE, skinny_tiles.h)
  const int32_t* pos; const int32_t* seq;      // position / cache sequence of every x row (device)
  const bf16_t* cos; const bf16_t* sin;        // [max_pos, 64]
  bf16_t* kc; bf16_t* vc;                      // [seq][kv head][cap][128]
  int g, n_kv, cap;
};
bool aigv_skinny_fp8_supported(int K, bool with_norm);
hipError_t aigv_launch_skinny_fp8(const bf16_t* x, int ldx, int R, const uint8_t* W8, int ldw, const float* w_scale, int N, int K, const bf16_t* resid,
                                  int ldr, bf16_t* out, int ldo, int epi, const AigvRopeKv* rk, const bf16_t* norm_w, float eps, int p, hipStream_t s);
bool aigv_skinny_norm_fusable(int K);   // hidden widths the fused-norm decode GEMVs exist for
// decode: SwiGLU(RMSNorm(x) W13^T) with the norm applied by the GEMV itself (R <= 4 rows, K <= 8192); same bits as rmsnorm + skinny swiglu
hipError_t aigv_launch_skinny_swiglu_normed(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, bf16_t* out, int ldo,
                                            const bf16_t* norm_w, float norm_eps, hipStream_t s, int p = 1);
// decode: wqkv projection of the new tokens with RoPE (q heads, K) and the K / V cache append in the GEMV's epilogue (head_dim 128)
hipError_t aigv_launch_skinny_rope_kv(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, bf16_t* qkv, int ldo,
                                      const int32_t* pos, const int32_t* seq, const bf16_t* cos, const bf16_t* sin, bf16_t* kc, bf16_t* vc,
                                      int g, int n_kv, int cap, int head_dim, hipStream_t s, const bf16_t* norm_w = nullptr, float norm_eps = 0.f, int p = 1);
// lm-head on R gathered rows + argmax over the vocabulary (first maximal index, bf16-rounded logits)
hipError_t aigv_launch_lm_head_argmax(const bf16_t* h, int R, int H, const bf16_t* W, int V,
                                      unsigned long long* packed, int64_t* out_idx, float* out_val, hipStream_t s);
// the same plus the log-probability of the chosen token: logprob[r] = val[r] - logsumexp(bf16-rounded logits of row r) in fp32, the
// sum merged from per-16-column partials part[R][aigv_lm_head_lse_slots(V)] in a fixed order (batch-invariant bits; lse_finish_kernel,
// logprob.hip); idx / val are aigv_launch_lm_head_argmax's bits.  val may be null.
// Candidates are optional (C = 0): with C <= AIGV_MAX_CANDIDATES token ids (DEVICE int64 [C]) out_cand[r, c] = bf16 logit of column cand[c] -
// the row's log-sum-exp, NaN for an id outside [0, V); the C columns come from a GEMV over the C gathered weight rows into cand_logit, a
// scratch of aigv_cand_logit_elems(R) bf16.  The same finisher runs either way: idx / val / logprob do not depend on the candidates.
// Top-k is optional too (k = 0): with 1 <= k <= min(V, AIGV_MAX_TOPK) the lm-head also stores its bf16 logits into row_logit[R][ldl]
// (ldl = aigv_topk_logit_ld(V), 8-byte aligned) and the finisher selects the k largest per row in the order of the packed argmax key -
// logit descending, equal logits by ascending id - into top_ids / top_logprob [R, k]; top_logprob[r, 0] is out_logprob[r], bit for bit.
#ifndef AIGV_MAX_CANDIDATES
#define AIGV_MAX_CANDIDATES 64   // = include/aigv_amd.h
#endif
#ifndef AIGV_MAX_TOPK
#define AIGV_MAX_TOPK 16         // = include/aigv_amd.h
#endif
size_t aigv_lm_head_lse_slots(int V);
size_t aigv_cand_logit_elems(int R);
hipError_t aigv_launch_lm_head_argmax_logprob(const bf16_t* h, int R, int H, const bf16_t* W, int V, unsigned long long* packed, float2* part,
                                              int64_t* out_idx, float* out_val, float* out_logprob, hipStream_t s, const int64_t* cand = nullptr,
                                              int C = 0, bf16_t* cand_logit = nullptr, float* out_cand = nullptr, int k = 0,
                                              bf16_t* row_logit = nullptr, int ldl = 0, int64_t* top_ids = nullptr, float* top_logprob = nullptr);
size_t aigv_topk_logit_ld(int V);
// the first half of aigv_launch_lm_head_argmax_logprob: the lm-head's packed argmax keys and log-sum-exp partials, no finisher
// logits != nullptr: also the bf16-rounded logits the partials were reduced from, into logits[R][ldl] (ldl % 4 == 0, ldl >= roundup(V, 4),
// 8-byte aligned; columns >= V of a row are padding) - the rows the decode step's top-k selection reads
hipError_t aigv_launch_lm_head_lse_partials(const bf16_t* h, int R, int H, const bf16_t* W, int V, unsigned long long* packed, float2* part,
                                            hipStream_t s, bf16_t* logits = nullptr, int ldl = 0);
// lm-head logits (bf16, the matmul output the reference upcasts) of R rows into out[R, ldo], ldo >= roundup(V, 4)
// one_form: the 4-slice form for every row count (that of the fused argmax), so that a row's logits do not depend on how many rows
// share the launch; otherwise <= 16 rows of a vocabulary <= 4096 take the 8-slice GEMV form
// ldh: leading dimension of the rows of h (0: H)
hipError_t aigv_launch_lm_head_logits(const bf16_t* h, int R, int H, const bf16_t* W, int V, bf16_t* out, int ldo, hipStream_t s,
                                      bool one_form = false, int ldh = 0);
// log-probabilities of bf16 logits rows [rows, ldo >= V] in fp32 (row_logprob_kernel, logprob.hip): one workgroup per row, a lane -> column
// mapping and a reduction tree fixed by V alone (batch-invariant bits); an id outside [0, V) gives NaN.
//   label:      out[r] = logits[r, labels[r]] - logsumexp(logits[r, :V]), labels DEVICE int64 [rows]
//   candidates: out[r, c] = logits[r, cand[c]] - logsumexp(logits[r, :V]), cand DEVICE int64 [C], 1 <= C <= AIGV_MAX_CANDIDATES, out [rows, C]
// Both are the one kernel, so column c of the second holds the first's bits for labels = cand[c].
hipError_t aigv_launch_label_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* labels, float* out, hipStream_t s);
hipError_t aigv_launch_cand_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* cand, int C, float* out, hipStream_t s);
//   top-k:      top_ids[r, j] = column of the j-th largest logit of row r (equal logits by ascending column: the packed argmax key's order),
//               top_logprob[r, j] = that logit - logsumexp(logits[r, :V]); 1 <= k <= min(V, AIGV_MAX_TOPK), both [rows, k].  The same fold and
//               tree as the two above: column j holds their bits for the id it names.
hipError_t aigv_launch_topk_logprob(const bf16_t* logits, int rows, int V, int ldo, int k, int64_t* top_ids, float* top_logprob, hipStream_t s);
// score head: x[B,H] -> chain of Linear+ReLU (bf16 rounding after each Linear), NaN/Inf guard on x
struct ScoreHeadArgs {
  const bf16_t* x; int ldx; int B;
  int n_layers; int dims[9];            // dims[0] = H, dims[i+1] = out of layer i
  const bf16_t* w[8]; const bf16_t* b[8];
  float* score;                         // [B] (the bf16 result widened to fp32)
};
// scratch: 3 * B * max(dims) bf16; B <= 64 per call
hipError_t aigv_launch_score_head(const ScoreHeadArgs& a, bf16_t* scratch, hipStream_t s);
// G batch slices of a.B <= 64 rows each, slice g at a.x + g * group_stride elements, every slice under its own NaN guard; a.score [G * a.B];
// scratch: 3 * G * a.B * max(dims) bf16.  Slice for slice the bits of aigv_launch_score_head (the depth lens: one slice per depth)
hipError_t aigv_launch_score_head_groups(const ScoreHeadArgs& a, int G, size_t group_stride, bf16_t* scratch, hipStream_t s);
// KV-cache append: copies the K/V slots of fused qkv rows into [n_seq, n_kv, cap, D] caches
hipError_t aigv_launch_kv_store(const bf16_t* qkv, int ld, const int32_t* seq_of_tok, const int32_t* pos,
                                bf16_t* kc, bf16_t* vc, int tokens, int n_groups, int g, int D, int cap,
                                hipStream_t s);
// frame ingest: uint8 HWC RGB -> (u/255 - mean)/std -> bf16 NCHW (torchvision ToTensor + Normalize + bf16 cast)
hipError_t aigv_launch_frame_ingest(const uint8_t* hwc, int n_frames, int H, int W, const float* mean, const float* stdv,
                                    bf16_t* out, hipStream_t s);
// uint8 HWC frames at any resolution -> Pillow-exact BICUBIC resize -> uint8 HWC (out_u8, may be null) and / or normalised
// bf16 NCHW (out_nchw, may be null); tmp_u8 holds the horizontal pass: n_frames * in_h * out_w * 3 bytes
hipError_t aigv_launch_frame_resize_ingest(const uint8_t* hwc, int n_frames, int in_h, int in_w, int out_h, int out_w,
                                           const float* mean, const float* stdv, uint8_t* tmp_u8, uint8_t* out_u8, bf16_t* out_nchw,
                                           hipStream_t s);
// records a message for aigv_last_error(NULL) from translation units other than context.hip (thread-local, like every handle-less error)
void aigv_set_error(const char* msg);
// a[i] += 1, b[i] += 1 for i < n (decode bookkeeping kept on the device: positions and visible KV lengths)
hipError_t aigv_launch_advance(int32_t* a, int32_t* b, int n, hipStream_t s);
hipError_t aigv_launch_decode_eos(int64_t* tok, int32_t* state, int n, const int64_t* eos_host, int n_eos, int64_t pad, hipStream_t s);
// small host int arrays passed by value as kernel arguments (no memcpy, no implicit host/stream sync)
#define AIGV_SMALL_INTS 256
struct SmallInts { int32_t v[AIGV_SMALL_INTS]; };
static_assert(AIGV_MAP_MAX_SEQS == AIGV_SMALL_INTS / 2 - 1, "the attention map takes the sequences one prefill call takes");
// pos[t] = t - cu[seq(t)] (+ pos_offset[seq(t)]), seq[t], and a device copy of cu[0..n_seq]; at most 127 sequences
hipError_t aigv_launch_seqpos(const int32_t* cu_host, int n_seq, int32_t* pos, int32_t* seq, int32_t* cu_dev, int tokens,
                              hipStream_t s, const int32_t* pos_offset_host = nullptr);
hipError_t aigv_launch_write_ints(const int32_t* host, int n, int32_t* dst, hipStream_t s);
// beam search: new KV cache slot i = the first lens[i] positions of slot parent[i] of the current cache (all layers, all kv heads); dst != src
hipError_t aigv_launch_kv_reorder(const bf16_t* sk, const bf16_t* sv, bf16_t* dk, bf16_t* dv, const int32_t* parent, const int32_t* lens, int n,
                                  int layers, int nkv, int cap, int D, size_t kv_layer, int max_len, hipStream_t s);
// the KV cache's key-drop mask: dst row i [ld_dst words] = src row parent[i] (null: i) [ld_src words] cut to its first len(i) keys, zero behind them;
// len(i) = lens[i], or (lens_are_cu) lens[i + 1] - lens[i]; every pointer on the device, dst != src
hipError_t aigv_launch_kv_drop_rows(const uint64_t* src, int ld_src, const int32_t* parent, const int32_t* lens, int lens_are_cu, uint64_t* dst, int ld_dst,
                                    int n, hipStream_t s);
