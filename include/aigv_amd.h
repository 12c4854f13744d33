/* aigv_amd.h — C ABI of libaigv_amd.so: the MI355X (gfx950) forward path of the AIGV-Assessor scorer.
 *
 * The reference has no FFI: its hot path sits behind the Python class InternVLChatModel
 * (internvl/model/internvl_chat_eval2/modeling_internvl_chat.py).  This header is the boundary a
 * maintainer binds instead (ctypes stub in INTEGRATION.md); each entry point names the reference
 * code it replaces.  Plain pointers and sizes only — no torch types.  All tensor pointers are DEVICE
 * pointers (bf16 = raw uint16 bits) unless marked host; outputs are caller-allocated; work is enqueued
 * on the caller's HIP stream and nothing synchronises except where noted.  Every function returns
 * 0 on success or a negative aigv_status; aigv_last_error() gives the message.  Never throws.
 *
 * Packed sequence convention: the B clips of a batch are concatenated without padding; clip b owns
 * token rows cu_seqlens[b] .. cu_seqlens[b+1]-1 and its positions restart at 0 — what the reference
 * computes for un-padded rows (modeling_internlm2.py:907-912) and for left/right padded batches
 * (:1141-1147).
 *
 * Threading: the intended deployment is one process per GPU (the reference's eval loop is single-threaded too).  A context is
 * not re-entrant - HOST calls on one context must not overlap - but it owns all the device state it uses (weights, workspaces,
 * split-K slab scratch), so several contexts, also on different devices of one process, are independent.
 * Streams: a context's device state comes in two halves.  aigv_vit_forward uses the InternViT workspaces, the InternViT row-plan
 * table and an InternViT split-K scratch of its own; every other entry point (aigv_project, aigv_motion_project, aigv_llm_prefill /
 * _extend, decode) uses the rest.  So ONE aigv_vit_forward may be in flight on one stream beside ONE pass of the other half on another
 * stream (the next clip's visual front beside this clip's InternLM2 pass); within a half, work must be stream-ordered (one launch
 * stream at a time, or the caller's events between them).
 * The context-free aigv_op_* entry points share one split-K scratch per DEVICE (created on first use, never regrown): overlap
 * them only from one stream per device.  Frame-resize coefficient tables are cached per (device, size pair) and immutable.
 */
#ifndef AIGV_AMD_H
#define AIGV_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIGV_ABI_VERSION 3   /* 2: aigv_out_row_logprob, aigv_op_label_logprob; 3: the decode-step operators (aigv_op_attention_decode ...),
                                later joined by aigv_decode_step_logprob and aigv_op_lm_head_argmax_logprob, then by the candidate-token
                                log-probabilities (aigv_out_row_cand_logprob, aigv_decode_step_cand_logprob, aigv_op_cand_logprob,
                                aigv_op_lm_head_argmax_cand_logprob), then by the test entry points aigv_op_attention_ex and aigv_op_kv_store,
                                then by the top-k log-probabilities (aigv_out_row_topk_logprob, aigv_decode_step_topk_logprob,
                                aigv_op_topk_logprob, aigv_op_lm_head_argmax_topk_logprob), then by the SlowFast plan walk for tests
                                (aigv_slowfast_plan_size / _plan_op / _run_ops / _buffer_read / _buffer_write and the host functions
                                aigv_slowfast_slow_indices / _pool_weights / _conv_k_slices), then by the test entry points of the score head
                                and the row kernels (aigv_op_score_head, aigv_op_rmsnorm_quant_fp8, aigv_op_rope_slots, aigv_op_embed,
                                aigv_op_seqpos, aigv_op_gather_rows, aigv_op_scatter_rows, aigv_op_cls_rows, aigv_op_write_ints), then by the
                                score-row attention probe (aigv_score_attention_arm, aigv_op_attention_probe), then by its dense per-key
                                form (aigv_score_attention_arm_tokens, aigv_op_attention_probe_tokens), then by the key-drop mask of the
                                prefill attention (aigv_key_drop_arm, aigv_op_attention_drop), then by the key-drop form of the decode attention
                                (aigv_op_attention_decode_drop; the mask now travels with the KV cache: aigv_key_drop_arm), then by the
                                key-drop mask by query row and layer window (aigv_key_drop_arm_ex, aigv_op_attention_drop_rows), then by the
                                depth lens (aigv_depth_lens_arm, aigv_depth_lens_token_readout, aigv_op_lens_tap, aigv_op_score_head_groups),
                                then by activation patching (aigv_stream_capture_arm, aigv_stream_patch_arm, aigv_op_stream_rows),
                                then by head knock-out and head patching (aigv_head_capture_arm, aigv_head_patch_arm, aigv_head_scale_arm,
                                aigv_op_head_rows), then by MLP neuron knock-out and neuron patching (aigv_neuron_capture_arm,
                                aigv_neuron_patch_arm, aigv_neuron_scale_arm, aigv_op_neuron_rows), then by the probe's value flow
                                (aigv_score_attention_arm_values, aigv_op_attention_probe_values), then by the attention flow map of
                                every query row (aigv_attention_map_arm, aigv_op_attention_map), then by the InternViT attention map
                                (aigv_vit_attention_arm, aigv_op_vit_attention_map), then by the InternViT patch mask - key-drop for the
                                non-causal attention (aigv_vit_key_drop_arm, aigv_op_attention_nc_drop)
                                - added symbols only: a library without them is refused at load
                                time, "missing <name>" */

/* Most candidate token ids one candidate log-probability call takes. */
#define AIGV_MAX_CANDIDATES 64
/* Largest k one top-k log-probability call takes. */
#define AIGV_MAX_TOPK 16

/* Score-row attention probe: most key segments (bins) and most probe rows one armed pass / one aigv_op_attention_probe call takes. */
#define AIGV_MAX_ATTN_SEGMENTS 64
#define AIGV_MAX_PROBE_ROWS 64

/* Largest aigv_config.kv_capacity a context accepts (tokens per clip): the decode attention's merge pass holds 16 bytes of LDS per
 * 128-key chunk of the capacity (32 KB at this bound). */
#define AIGV_MAX_KV_CAPACITY 262144

typedef struct aigv_ctx aigv_ctx;

enum aigv_status {
  AIGV_OK = 0,
  AIGV_ERR_ARG = -1,      /* bad argument / shape the kernels do not cover */
  AIGV_ERR_HIP = -2,      /* a HIP call failed */
  AIGV_ERR_STATE = -3,    /* weights missing, capacity exceeded, no KV state ... */
  AIGV_ERR_ALLOC = -4
};

enum aigv_dtype { AIGV_BF16 = 0, AIGV_F32 = 1 };

/* Model + capacity description.  Field meanings follow the reference's config classes
 * (configuration_intern_vit.py:20-119, configuration_internlm2.py:26-150, configuration_internvl_chat.py). */
typedef struct aigv_config {
  /* InternViT */
  int32_t vit_hidden, vit_inter, vit_heads, vit_layers;
  int32_t image_size, patch_size, num_channels;
  int32_t vit_norm_rms;      /* 0: nn.LayerNorm (ViT-300M), 1: InternRMSNorm (ViT-6B) */
  int32_t vit_qk_norm;       /* full-width QK RMSNorm (modeling_intern_vit.py:148-151) */
  int32_t vit_qkv_bias;
  float vit_eps;
  int32_t select_layer;      /* -1 = last (modeling_internvl_chat.py:509-518) */
  int32_t shuffle;           /* 1/downsample_ratio (2) */
  /* InternLM2 */
  int32_t llm_hidden, llm_inter, llm_heads, llm_kv_heads, llm_layers, vocab;   /* head width 128; 1..8 query heads per KV head (8B: 4, 20B: 6); widths multiples of 128 */
  float rms_eps;
  int32_t max_positions;     /* rows of the RoPE tables the host uploads */
  /* heads */
  int32_t motion_dim;        /* SlowFast feature width (2304) */
  int32_t n_score_layers;    /* 5 */
  int32_t score_dims[8];     /* 1024,256,64,16,1 */
  /* capacity (workspaces are allocated once, in aigv_ctx_create) */
  int32_t max_frames;        /* frames per aigv_vit_forward call (processed in chunks of vit_chunk) */
  int32_t vit_chunk;         /* frames per ViT pass (workspace size) */
  int32_t max_tokens;        /* packed tokens per aigv_llm_prefill call */
  int32_t max_seqs;          /* clips per call */
  int32_t max_out_rows;      /* lm-head rows per call (answer rows), <= 64 per launch, looped */
  int32_t kv_capacity;       /* per-clip KV-cache length for decode (0 = no decode support; at most AIGV_MAX_KV_CAPACITY) */
} aigv_config;

/* ---- lifetime ------------------------------------------------------------------------------------ */
int aigv_abi_version(void);
int aigv_sizeof_config(void);                        /* sizeof(aigv_config): binding self-check */
int aigv_ctx_create(int device, const aigv_config* cfg, aigv_ctx** out);
void aigv_ctx_destroy(aigv_ctx* ctx);
/* Change the CAPACITIES of a context (max_frames, vit_chunk, max_tokens, max_seqs, max_out_rows, kv_capacity, max_positions; every
 * other field of `cfg` must equal the context's): the workspaces are re-allocated, the loaded weights - and in fp8 mode their e4m3
 * copies and the mode itself - stay where they are.  Kept KV state is dropped.  When max_positions changed the rotary tables
 * ("rope.cos" / "rope.sin") must be loaded again at the new length and aigv_finalize_weights called before the next pass; that
 * finalize keeps the fp8 mode (see aigv_set_precision).  Synchronises the device.  A failed resize (out of memory) leaves the
 * context unusable: destroy it. */
int aigv_ctx_resize(aigv_ctx* ctx, const aigv_config* cfg);
const char* aigv_last_error(const aigv_ctx* ctx);     /* ctx may be NULL (creation errors) */
/* Read and clear the HIP runtime's sticky last-error state of the calling thread.  The launchers report hipGetLastError() after every launch, so an error
 * left behind by something ELSE - a stream capture the caller's framework abandoned (hipErrorStreamCaptureInvalidated stays pending after the failed
 * hipStreamEndCapture) - would be blamed on the next launch of this library.  A host that falls back from a failed capture to eager launches calls this first. */
void aigv_clear_hip_error(void);

/* Weight upload.  `name` is the reference state-dict key, e.g.
 * "vision_model.encoder.layers.3.attn.qkv.weight", "language_model.model.layers.0.attention.wqkv.weight",
 * "mlp1.1.bias", "mlpscore.fc1.weight"; plus two host-precomputed tables "rope.cos" / "rope.sin"
 * [max_positions, head_dim/2] (modeling_internlm2.py:176-194) and the position table already resized to this
 * ctx's image size (modeling_intern_vit.py:87-93).  Data is bf16 (or f32, converted); `on_device` says where
 * `data` lives.  The ctx keeps its own repacked copy (padded patch kernel, interleaved w1|w3).  Synchronous. */
int aigv_load_weight(aigv_ctx* ctx, const char* name, const void* data, const int64_t* shape, int ndim,
                     int dtype, int on_device);
int aigv_finalize_weights(aigv_ctx* ctx);             /* checks that every tensor the config needs is present */

/* ---- hot path ------------------------------------------------------------------------------------ */
/* InternVisionModel.forward + cls drop + pixel_shuffle(v2)  (modeling_intern_vit.py:95-107,216-228,324-362;
 * modeling_internvl_chat.py:492-527).  frames: [F,3,S,S] bf16 NCHW.  out: [F*ntok, shuffle^2*vit_hidden] bf16
 * pre-projector tokens — the payload of the frame-DP all-gather. */
int aigv_vit_forward(aigv_ctx* ctx, const void* frames, int n_frames, void* out_tokens, void* stream);
/* InternViT attention map: the full, NON-causal softmax matrix of every query row of every frame, per layer - what the flash kernel never
 * forms.  Arms exactly the next aigv_vit_forward on the context (that call disarms on every way out), which launches two stand-alone kernels
 * between the QK-norm and the flash attention of every layer layer_lo <= l < layer_hi; a layer outside the window launches nothing.  They
 * read the bf16 Q and K of the layer's fused qkv rows (after the full-width QK RMSNorm where the config has one) and write the caller's
 * buffer and a stats scratch the context owns (sized at create / resize from vit_chunk: nothing is allocated in the pass) - nothing the pass
 * reads afterwards: armed or not, out_tokens keeps its bits.
 * Mapped quantity, for frame f, head h, query row i, key j, 0 <= i, j < S = patches + 1:
 *   acc_ij  = the fp32 MFMA accumulation of the exact bf16 products q_i . k_j
 *   s_ij    = acc_ij / sqrtf(D)
 *   m_i     = max_j s_ij
 *   e_ij    = expf(s_ij - m_i)
 *   total_i = the fp32 sum of the e_ij, in an order fixed by the key index alone
 *   p_ij    = e_ij / total_i
 * per head (per_head != 0): out[f][l - layer_lo][h][i][j] = p_ij
 * head mean (per_head == 0): out[f][l - layer_lo][i][j] = (p0_ij + p1_ij + ... in ascending h, starting from +0.0) / n_heads, one fp32 division
 * Scores and weights are ALWAYS fp32, whatever aigv_set_attention_numerics says, and the UNSCALED bf16 Q is used: the flash kernel's bf16
 * q_prescale rounding (exact only for D = 64) is not reproduced.  No atomics; a row's bits depend on its own frame's Q and K alone (not on
 * the batch mates, the chunk or the window); keys past the frame's end never enter arithmetic.
 * out_dev: the caller's fp32 device buffer [n_frames][layer_hi - layer_lo][S][S] (per_head: [n_frames][layer_hi - layer_lo][vit_heads][S][S]),
 * indexed by the absolute frame number across vit_chunk chunks; every element is written and nothing outside is.
 * Refused by the pass, AIGV_ERR_ARG with a message, before it launches anything: a window outside 0 <= layer_lo < layer_hi <= the number of
 * layers the pass RUNS (select_layer's count, not vit_layers). */
int aigv_vit_attention_arm(aigv_ctx* ctx, float* out_dev, int layer_lo, int layer_hi, int per_head);
/* Patch occlusion inside the tower: arms exactly the NEXT aigv_vit_forward, whose flash attention of every layer layer_lo <= l < layer_hi (of the layers
 * the pass runs) hides keys from every query row and head of their frame - the non-causal key-drop form of the attention kernel.  The armament is
 * consumed on EVERY way out of that call.  words_dev: DEVICE uint64 [n_frames][ld_words], 8-byte aligned, ld_words >= ceil(S / 64), indexed by the
 * absolute frame number across vit_chunk chunks; bit (j & 63) of word f * ld_words + (j >> 6) set = key j of frame f is hidden.  Key 0 is cls, key
 * 1 + grid * y + x is patch (y, x).  Bits at or past S are ignored.  A dropped key is hidden from its own row too; its row still runs (as a query),
 * so its patch reaches its own token through the residual stream.  A frame whose every key is hidden has zero attention output rows.  The layers
 * outside the window, and an unarmed pass, run the unmasked kernel.  The masked kernel runs with the lead-key tune knob off whatever it is set to.
 * Refused by the pass, AIGV_ERR_ARG with a message, before it launches anything: a window outside 0 <= layer_lo < layer_hi <= the layers the pass
 * RUNS, and a pass armed with both aigv_vit_attention_arm and a mask (the map kernel does not know the mask). */
int aigv_vit_key_drop_arm(aigv_ctx* ctx, const uint64_t* words_dev, int ld_words, int layer_lo, int layer_hi);
/* mlp1: LayerNorm -> Linear -> GELU -> Linear (modeling_internvl_chat.py:238-243,529). rows x proj_in -> rows x llm_hidden */
int aigv_project(aigv_ctx* ctx, const void* tokens, int rows, void* out, void* stream);
/* motion_mlp on the SlowFast feature (modeling_internvl_chat.py:244-249,345). [B, motion_dim] -> [B, llm_hidden] */
int aigv_motion_project(aigv_ctx* ctx, const void* motion_feature, int n_clips, void* out, void* stream);

/* InternVLChatModel.forward from the embedding scatter onwards (modeling_internvl_chat.py:324-488,
 * modeling_internlm2.py:868-998,1094-1096):
 *   ids[T] int64 packed token ids; slot[T] int32: -1 = text token (embedding row ids[t]); 0..n_vis-1 = row of
 *   `vis`; n_vis + b = row b of `motion`.  cu_seqlens: HOST int32[B+1].
 *   score_rows[B]  (HOST int32, packed row index of hidden[:, -4] per clip) -> score[B] float (device), may be NULL
 *   logit_rows[R]  (HOST int32, packed row indices whose next-token argmax is wanted) -> argmax[R] int64 (device)
 *   keep_kv != 0 stores K/V of every layer into the ctx KV cache for aigv_decode_step.                      */
int aigv_llm_prefill(aigv_ctx* ctx, const int64_t* ids, const int32_t* slot, const int32_t* cu_seqlens, int n_clips,
                     const void* vis, int n_vis, const void* motion, const int32_t* score_rows, float* score,
                     const int32_t* logit_rows, int n_logit_rows, int64_t* argmax, int keep_kv, void* stream);
/* Continue the sequences kept by aigv_llm_prefill(keep_kv = 1) with new TEXT tokens (no visual slots): ids = DEVICE int64 of the
 * packed new tokens, cu = HOST int32[n_clips + 1] over the new tokens only; rows index the packed new tokens.  The new rows attend
 * causally to the cached keys and to themselves (positions continue after the cache).  commit = 0 leaves the cache lengths
 * unchanged, so several continuations of ONE prefix - the four quality-perspective questions behind the same video tokens
 *  - can be scored one after the other; commit = 1 appends them (a longer chat turn before aigv_decode_step).
 * Replaces re-running modeling_internvl_chat.py:306-488 from the first token for every question. */
int aigv_llm_extend(aigv_ctx* ctx, const int64_t* ids, const int32_t* cu, int n_clips, const int32_t* score_rows, float* score,
                    const int32_t* logit_rows, int n_logit_rows, int64_t* argmax, int commit, void* stream);

/* Score-row attention by segment: WHERE a few rows of the next scoring pass look.  Arms exactly the next aigv_llm_prefill or
 * aigv_llm_extend on this context: that pass launches one small stand-alone kernel per decoder layer, right behind the layer's wqkv + RoPE
 * (and, in aigv_llm_extend, behind its KV-cache append), which recomputes the causal softmax of the n_rows probe rows per query head from
 * the layer's Q and K and folds it into n_segments bins:
 *   out_dev[row][layer][head][seg] = sum over the visible keys j with segment id seg of softmax_j(q . k_j / sqrt(head_dim))      (fp32, DEVICE)
 * for ALL layers - a row-trimmed last layer included (the probe reads Q and K, not the attention output).  The pass then disarms, also
 * when it fails.  rows_host: HOST int32[n_rows] packed row indices of that pass, 1 <= n_rows <= AIGV_MAX_PROBE_ROWS.  Segment ids, DEVICE
 * int32, read when the pass runs: seg_new_dev[packed row of the pass] and - aigv_llm_extend only, where it is required; NULL for a prefill -
 * seg_cached_dev[sequence * ld_cached + position] for the keys cached before the pass (ld_cached >= the longest cached length).  An id
 * outside [0, n_segments) drops its key from the bins but not from the softmax total, so a row's bins sum to 1 minus the dropped mass;
 * 1 <= n_segments <= AIGV_MAX_ATTN_SEGMENTS.
 * Numerics: the probe is a report, not part of the pass.  Its scores are ALWAYS fp32, whatever aigv_set_attention_numerics says; q is rotated
 * with the RoPE kernel's own arithmetic (the bf16 bits aigv_op_rope would store); every bin and the total are summed in an order fixed by the
 * key index alone (no atomics), and out = bin / total is one fp32 division - a row's bits do not depend on the other rows, the batch mates or
 * the launch grid.  The existing kernels are not touched: armed or not, every other output of the pass keeps its bits.  Nothing is allocated,
 * so an armed pass still captures into a HIP graph (rows_host is baked into the capture; the tables and out_dev are read / written through
 * their addresses).  Limits and rows are checked when the pass runs: AIGV_ERR_ARG from the pass, with a message.
 * Out of scope: aigv_decode_step ignores the feature (an armed context stays armed across decode steps). */
int aigv_score_attention_arm(aigv_ctx* ctx, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev,
                             int ld_cached, int n_segments, float* out_dev);
/* Score-row attention per KEY: aigv_score_attention_arm's arguments and contract (it arms exactly the next aigv_llm_prefill / aigv_llm_extend,
 * which disarms on every way out; out_dev is filled as above, bit for bit), plus a dense output filled by the SAME launch per layer:
 *   tok_out_dev[row][layer][head][j] = softmax_j(q . k_j / sqrt(head_dim))   for the key positions j = 0 .. pos of the row's own sequence
 *                                                                             (the cached keys first, then the rows of this pass)
 *   tok_out_dev[row][layer][head][j] = +0.0                                  for pos < j < ld_tok
 * fp32, DEVICE, [n_rows][layers][n_heads][ld_tok]: every column is written, nothing outside them.  The scores, the row maximum, the total
 * and the one division are the bins': a bin that holds exactly one key carries that key's dense bits, and a row's bits are its own.
 * ld_tok must be at least the largest pos + 1 over the probe rows and at most AIGV_MAX_KV_CAPACITY: AIGV_ERR_ARG from the pass, with a
 * message, before its first layer.  Nothing is allocated (the armed pass still captures); aigv_decode_step ignores the feature. */
int aigv_score_attention_arm_tokens(aigv_ctx* ctx, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev,
                                    int ld_cached, int n_segments, float* out_dev, float* tok_out_dev, int ld_tok);
/* Score-row VALUE flow: aigv_score_attention_arm_tokens' arguments and contract (out_dev and tok_out_dev are filled as above, bit for bit;
 * tok_out_dev may be NULL with ld_tok = 0: the bins only), plus WHAT the row takes from every segment, filled by the SAME launch per layer:
 *   val_out_dev[row][layer][head][s][c] = sum over the visible keys j of segment s of softmax_j * v_j[c]     s = 0 .. n_segments, c < head_dim
 * fp32, DEVICE, [n_rows][layers][n_heads][n_segments + 1][head_dim]: slot s = n_segments collects the keys whose id lies outside
 * [0, n_segments) - the keys the bins drop and the total keeps - so the n_segments + 1 vectors of a head sum to that head's attention output
 * at the row (the row its wo consumes), split by where it was read from.  v_j: the bf16 V the pass's own attention reads - the V columns of
 * the layer's fused qkv rows in aigv_llm_prefill, the V cache in aigv_llm_extend - of kv head (head / g).
 * Numerics: e_j = expf(s_j - max) are the bins' own; every element is accumulated UNNORMALISED in fp32, one fmaf per key, in an order fixed
 * by the key index alone (the keys j = l mod KL, KL = 256 / head_dim, ascending, form chain l; the KL chains are added in order l = 0, 1, ..),
 * then divided ONCE by the bins' total.  No atomics; a row's bits do not depend on the other rows, the batch mates or the grid.  0 x Inf is
 * NaN, as in the attention kernels: a non-finite V row of a visible key makes its segment NaN even where the key's weight underflowed to 0.
 * The kernel keeps (2 (n_segments + 1) + 2) KiB of LDS per workgroup (135 KiB at 64 segments).  Nothing is allocated; limits are checked when
 * the pass runs.  An unarmed pass, or one armed through the two functions above, launches exactly what it always launched. */
int aigv_score_attention_arm_values(aigv_ctx* ctx, const int32_t* rows_host, int n_rows, const int32_t* seg_new_dev, const int32_t* seg_cached_dev,
                                    int ld_cached, int n_segments, float* out_dev, float* tok_out_dev, int ld_tok, float* val_out_dev);
/* Attention flow map: where EVERY query row of the pass looks, per layer and head, folded into key segments - the observational sibling of the
 * probe above, for all T packed rows instead of a few.  Arms exactly the next aigv_llm_prefill on this context, which launches a stand-alone
 * MFMA kernel after the fused wqkv GEMM + RoPE of EVERY layer - a row-trimmed last layer included (it reads Q and K, which exist for all rows) -
 * and disarms on every way out.  For the packed row t at position p of its clip and query head h:
 *   rows[t][h][s] = (sum over the keys j <= p of the same clip with seg_dev[j] == s of e_j) / (sum over the keys j <= p of e_j),
 *   e_j = expf(s_j - max_j s_j),  s_j = (q . k_j) / sqrt(head_dim) in fp32, q rotated with the RoPE kernel's own arithmetic.
 * seg_dev: DEVICE int32 [T], read when the pass runs; an id outside [0, n_segments) counts for the total only.  1 <= n_segments <=
 * AIGV_MAX_ATTN_SEGMENTS.  Outputs, fp32, DEVICE, the caller's, each optional (at least one):
 *   rows_out_dev [layer_hi - layer_lo][T][n_heads][n_segments]: the rows of the layers layer_lo <= l < layer_hi (0 <= lo <= hi <= layers; pass
 *     NULL with lo = hi); every element is written, nothing outside;
 *   seg_out_dev [n_clips][layers][n_heads][n_segments][n_segments]: seg_out[b][l][h][a][c] = the mean over the query rows of clip b whose id is
 *     a of rows[.][h][c] - the rows added in ascending order in fp32, ONE division by their number; NaN where clip b has no row of segment a.
 * scratch_dev [T][n_heads][n_segments]: where the rows of a layer outside the window go in front of the fold; required with seg_out_dev unless
 * the window covers every layer.  A layer whose rows nobody reads (outside the window, no seg_out_dev) launches nothing.
 * Numerics: scores and weights are ALWAYS fp32, whatever aigv_set_attention_numerics says; the bf16 products of a score are exact, a bin is a
 * chain of fp32 additions in an order fixed by the key index alone (no atomics), the last step is one fp32 division bin / total - a row's
 * bits depend on its own keys, its position and the table, not on the other rows, the batch mates or the grid.  The existing kernels are not
 * touched: armed or not, every other output of the pass keeps its bits.  Nothing is allocated.
 * Refused by the pass, AIGV_ERR_ARG with a message, before it launches anything: an armed key-drop mask (the map does not know the mask),
 * keep_kv, limits and a missing scratch.  aigv_llm_extend refuses an armed map (there is no cache form). */
int aigv_attention_map_arm(aigv_ctx* ctx, const int32_t* seg_dev, int n_segments, float* scratch_dev, float* seg_out_dev, float* rows_out_dev,
                           int layer_lo, int layer_hi);

/* Key-drop mask: run the clips with some tokens HIDDEN from the LLM - what the reference computes for attention_mask zeros in the middle of a
 * sequence (positions stay as they are; the additive mask hides those keys from every query row).  Arms exactly the next aigv_llm_prefill on
 * this context: the prefill attention of EVERY layer of that pass, the row-trimmed last layer included, runs in its key-drop form, and every
 * output of the pass (score, argmax, the aigv_out_row_* read-outs) is that of the masked pass.  The pass then disarms, also when it fails.
 *   words_dev  DEVICE uint64 [n_clips][ld_words], read when the pass runs: bit (j & 63) of word [clip][j >> 6] set = token j of that clip (its
 *              position inside the clip, 0 = first token) is invisible, as a key, to every query row and head of its clip.  One word is one
 *              64-key tile of the kernel; bits past a clip's length are ignored.
 *   ld_words   words per clip, >= ceil(longest clip / 64): AIGV_ERR_ARG from the pass, with a message, otherwise.
 * With keep_kv != 0 the mask becomes part of the KV state: the pass copies every clip's words (cut to the clip's length, zero behind it) into a
 * mask the context owns beside the caches - uint64 [max_seqs][ceil(kv_capacity / 64)], by absolute position, allocated, resized and invalidated
 * with them; nothing is allocated in the pass - and from then on aigv_llm_extend (the key-drop form of the prefill kernel) and every
 * aigv_decode_step* (the key-drop form of the decode attention) run under it: what was hidden from the prompt stays hidden from every later
 * token, while the keys those passes append are visible.  aigv_kv_fork replicates the mask rows with the slots, aigv_kv_reorder gathers them
 * by parent.  The cache stays masked until the next aigv_llm_prefill: an unmasked keep_kv prefill (or aigv_ctx_resize) drops the mask.
 * A query row left without a visible key has an all-zero attention output (the reference's softmax over a fully masked row is uniform
 * instead): keep every clip's first token visible.  The V rows of dropped keys must be FINITE: the kernels multiply them by an exact 0, and
 * 0 x NaN is NaN, as it is in torch.  Tiles / chunks without a dropped key run the unmasked arithmetic; an unarmed pass on an unmasked cache
 * enters no new code.
 * Refused with AIGV_ERR_ARG and a message: an ARMED aigv_llm_extend (the continuation takes no mask of its own: it inherits the cache's), a pass
 * that is also armed with the score-attention probe, and the probe armed in front of aigv_llm_extend on a masked cache (the probe does not
 * know the mask). */
int aigv_key_drop_arm(aigv_ctx* ctx, const uint64_t* words_dev, int ld_words);
/* The key-drop mask by query row and layer window - the attention knock-out: cut the edges from a set of query rows to a set of keys inside a
 * window of layers.  aigv_key_drop_arm(ctx, w, ld) = aigv_key_drop_arm_ex(ctx, w, NULL, ld, 0, llm_layers).  Arms exactly the next
 * aigv_llm_prefill, which disarms on every way out.
 *   row_words_dev  DEVICE uint64 [n_clips][ld_words] in words_dev's layout, or NULL = every row: bit (i & 63) of word [clip][i >> 6] set = the
 *                  query row at position i of that clip is subject to the mask.  A score is hidden iff its key's bit and its row's bit are both
 *                  set; every other row sees what the causal mask leaves it.  Bits past a clip's length are ignored.
 *   layer_begin, layer_end   only the layers layer_begin <= l < layer_end run the masked attention (the row-selective form of the prefill kernel
 *                  with row words, its key-drop form without); every other layer runs the unmasked launch it always ran.  An empty window is
 *                  the plain pass.
 * What the reference computes when the additive attention mask of those layers also holds finfo.min at every (row, key) both words select.
 * Refused with AIGV_ERR_ARG and a message, nothing armed: a window outside 0 <= layer_begin <= layer_end <= llm_layers, words that are null
 * (words_dev) or not 8-byte aligned, ld_words < 1.  Refused by the pass, before any launch: ld_words below ceil(longest clip / 64); keep_kv
 * together with row words or a window other than [0, llm_layers) - the mask kept beside the KV cache has neither; the probe armed as well.
 * aigv_llm_extend refuses an armed context as it does after aigv_key_drop_arm. */
int aigv_key_drop_arm_ex(aigv_ctx* ctx, const uint64_t* words_dev, const uint64_t* row_words_dev, int ld_words, int layer_begin, int layer_end);

/* Most score rows, and most token rows, one depth-lens pass takes. */
#define AIGV_MAX_LENS_ROWS 64
/* The depth lens: read the residual stream of a few rows after EVERY layer.  Arms exactly the next aigv_llm_prefill, which disarms on every way
 * out.  With L = llm_layers, depth d = 0 is the embedding, depth d the stream after d layers, depth L what the final norm consumes.
 *   score_rows_host  HOST int32 [n_score], token_rows_host HOST int32 [n_token]: packed row indices in score_rows' convention (copied here: the
 *                    arrays need not outlive the call); 0 <= n_score, n_token <= AIGV_MAX_LENS_ROWS, at least one row in all.  Every row must be
 *                    one of that pass's consumed rows (a score row or a logit row): the last layer finishes only those.
 *   hidden_out_bf16  DEVICE bf16 [L + 1][n_score + n_token][H]: the rows as they are, score rows first;
 *   normed_out_bf16  DEVICE bf16, same layout: the model's final RMSNorm of each - the bits the pass's own final norm gives such a row;
 *   score_out        DEVICE fp32 [L + 1][n_score] (NULL when n_score = 0): the score head on normed_out[d][:n_score], the NaN guard taken over
 *                    those n_score rows of that depth; score_out[L] holds the bits of the pass's own `score` for the same rows.
 * The buffers are the caller's (16-byte aligned; score_out 4-byte) and must stay alive until the pass has run; nothing is allocated in the pass,
 * so it still captures.  The pass adds one launch per depth (the tap) and, after its own heads, the score head over all depths' score rows at
 * once; nothing it computed before changes a bit, and an unarmed pass enters no new code.  Combines with aigv_key_drop_arm / _ex and the
 * score-attention probe: it reads the stream, not the attention.
 * Refused with AIGV_ERR_ARG and a message, nothing armed: a row list longer than AIGV_MAX_LENS_ROWS or no row at all, a null row list, a null or
 * misaligned buffer.  Refused by the pass, before any launch: a lens row that is not among its consumed rows, score rows when the pass has
 * score == NULL, a pass without output rows; aigv_llm_extend refuses an armed context. */
int aigv_depth_lens_arm(aigv_ctx* ctx, const int32_t* score_rows_host, int n_score, const int32_t* token_rows_host, int n_token,
                        void* hidden_out_bf16, void* normed_out_bf16, float* score_out);
/* The lm-head read-out of normed rows such as normed_out_bf16's token rows: n_rows >= 1 DEVICE bf16 rows of H elements, leading dimension ld
 * (a multiple of 8, >= H), 64 rows at a time through the logits scratch of aigv_out_row_logprob in its one form (a row's bits do not depend on
 * its chunk) - one pass over the lm-head weights per chunk, both read-outs from the same fill:
 *   top_id [n_rows] int64 / top_logprob [n_rows] fp32   the largest bf16 logit (equal logits: the lower id) and its full-vocabulary
 *                    log-probability - aigv_out_row_topk_logprob's bits with k = 1;
 *   cand_logprob [n_rows, C] fp32 (cand_ids DEVICE int64 [C], 1 <= C <= AIGV_MAX_CANDIDATES; both NULL and C = 0: not read)
 *                    aigv_out_row_cand_logprob's bits. */
int aigv_depth_lens_token_readout(aigv_ctx* ctx, const void* normed_rows_dev, int ld, int n_rows, const int64_t* cand_ids, int C, int64_t* top_id,
                                  float* top_logprob, float* cand_logprob, void* stream);

/* Activation patching: copy rows of the residual stream out of a pass (capture) or overwrite them in it (patch), by depth.  Each arms exactly the
 * next aigv_llm_prefill, which disarms on every way out.  With L = llm_layers, depth d, 0 <= d < L, is the stream layer d CONSUMES - d = 0 the
 * embedding with the visual and motion tokens in place, depth d the stream after d layers: the depth lens' numbering.  Depth L is not offered.
 *   rows_host   HOST int32 [n]: packed row numbers in score_rows' convention, copied here (the array need not outlive the call).  The pass checks
 *               them: each inside [0, T) of its T packed rows, strictly ascending (so a patch's rows are unique); 0 <= n <= max_tokens.
 *   lo, hi      the window: depths lo <= d < hi, 0 <= lo <= hi <= L (checked by the pass).
 *   out_bf16_dev / values_bf16_dev   DEVICE bf16 [n][hi - lo][H], 16-byte aligned, the caller's, alive until the pass has run: element (i, d - lo)
 *               holds row rows_host[i] at depth d.  May be NULL when n = 0 or the window is empty (nothing is then launched).
 * At the top of layer d the pass first writes the patch's rows over the stream - a bit copy, no arithmetic: NaN and Inf payloads travel unchanged,
 * and every later layer, read-out and head sees the patched stream - then reads the capture's rows from it, so a capture armed beside a patch
 * returns the stream as the layer consumes it.  One launch each per armed layer; the row numbers go to a buffer the context owns (sized by
 * max_tokens): nothing is allocated in the pass.  An unarmed pass takes two untaken branches per layer and enters no new code.  Both combine with
 * aigv_key_drop_arm / _ex, the score-attention probe, aigv_depth_lens_arm and fp8 mode.
 * Refused with AIGV_ERR_ARG and a message, nothing armed: a null context, n outside 0..max_tokens, a null row list, a null or misaligned buffer.
 * Refused by the pass, before any launch: a row outside [0, T), rows not strictly ascending, a window outside [0, L], keep_kv; aigv_llm_extend
 * refuses an armed context. */
int aigv_stream_capture_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, int lo, int hi, void* out_bf16_dev);
int aigv_stream_patch_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, int lo, int hi, const void* values_bf16_dev);

/* Head knock-out and head patching: the per-head attention outputs of a layer - the row its wo consumes, bf16 [n_heads][D] per token, head h in columns
 * [h D, (h + 1) D) - copied out of a pass (capture), overwritten in it (patch) or multiplied by a factor per head (scale).  Each arms exactly the next
 * aigv_llm_prefill, which disarms on every way out.  Inside layer l the order is: attention, scale, patch, capture, wo - so a capture armed beside the
 * other two returns what wo consumes, and every later layer, the lens, a stream capture and all heads see the modified pass.
 *   rows_host   HOST int32 [n]: packed row numbers, copied here; checked by the pass like a stream capture's (inside [0, T), strictly ascending);
 *               0 <= n <= max_tokens.  aigv_head_scale_arm: NULL = every row the pass runs (n is then ignored).
 *   lo, hi      the window: layers lo <= l < hi, 0 <= lo <= hi <= L (checked by the pass).
 *   out_bf16_dev / values_bf16_dev   DEVICE bf16 [n][hi - lo][n_heads * D], 16-byte aligned, the caller's, alive until the pass has run: element
 *               (i, l - lo) holds row rows_host[i] at layer l.  May be NULL when n = 0 or the window is empty.
 *   head_bits_host   HOST uint64 [hi - lo], copied here: bit h of word l - lo selects head h at layer l; NULL = every head.  Only the selected heads'
 *               columns are overwritten - a bit copy, NaN payloads travel unchanged; an unselected head's bytes are neither read nor written.
 *   scale_host  HOST float [L][n_heads], copied here: the new value is bf16(fp32(x) * s), round to nearest even (0 * Inf = NaN).  An entry that is
 *               exactly 1.0 leaves its head untouched (no read, no write); a layer whose row is all ones launches nothing.  Scale 0 knocks a head out.
 * At most one launch each per armed layer; the row numbers go to a buffer the context owns, the factors travel as kernel arguments: nothing is
 * allocated or copied in the pass.  An unarmed pass takes three untaken branches per layer.  A capture whose window holds layer L - 1 makes the
 * row-trimmed last attention launch cover every row (the consumed rows keep their bits); a patch or scale of a row the trimmed layer does not consume
 * has no consumer and is allowed.  All three combine with each other, aigv_key_drop_arm / _ex, the score-attention probe (it reads Q and K),
 * aigv_depth_lens_arm, the stream capture / patch and fp8 mode (the ops act on the bf16 rows the e4m3 wo consumes).
 * Refused with AIGV_ERR_ARG and a message, nothing armed: a null context, n outside 0..max_tokens, a null row list (capture, patch), a null or
 * misaligned buffer, a model of more than 64 query heads, a null scale table, a NaN scale.  Refused by the pass, before any launch: a row outside
 * [0, T), rows not strictly ascending, a window outside [0, L], keep_kv, a head dimension other than 64 or 128, a window (a scale row with a factor
 * other than 1) that reaches layer L - 1 in a pass without output rows (its last attention does not run); aigv_llm_extend refuses an armed context. */
int aigv_head_capture_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, int lo, int hi, void* out_bf16_dev);
int aigv_head_patch_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, int lo, int hi, const uint64_t* head_bits_host, const void* values_bf16_dev);
int aigv_head_scale_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, const float* scale_host);

/* MLP neuron knock-out and neuron patching: the neurons of a layer - the row its w2 (down_proj) consumes, the output of the fused SwiGLU epilogue, bf16
 * [I] per token - copied out of a pass (capture), overwritten in it (patch) or multiplied by a factor (scale).  Each arms exactly the next
 * aigv_llm_prefill, which disarms on every way out.  Inside layer l the order is: w1|w3 + SwiGLU, scale, patch, capture, w2 - so a capture armed beside
 * the other two returns what w2 consumes, and every later layer, the lens, a stream capture and a head capture see the modified pass.
 *   rows_host   HOST int32 [n]: packed row numbers, copied here; checked by the pass like a stream capture's (inside [0, T), strictly ascending);
 *               0 <= n <= max_tokens.  aigv_neuron_scale_arm: NULL = every row the pass runs (n is then ignored).
 *   lo, hi      the window: layers lo <= l < hi, 0 <= lo <= hi <= L (checked by the pass).
 *   cols_host   HOST int32 [m], copied here: the neurons, strictly ascending inside [0, I), m <= AIGV_MAX_NEURON_SEL = 4096 - the sparse form; NULL: the
 *               dense form, every neuron (m is then ignored).
 *   out_bf16_dev / values_bf16_dev   DEVICE bf16 [n][hi - lo][W], W = I (dense) or m (sparse; element j is neuron cols_host[j]), 16-byte aligned, the
 *               caller's, alive until the pass has run: element (i, l - lo) holds row rows_host[i] at layer l.  May be NULL when nothing is selected.
 *   layer_scale_host   HOST float [L] or NULL, copied here: every neuron of layer l is multiplied by layer_scale_host[l]; 0 knocks the MLP block out.
 *   sel_layers_host / sel_cols_host / sel_factors_host   HOST [m] each (m may be 0), copied here: neuron sel_cols_host[j] of layer sel_layers_host[j] is
 *               multiplied by sel_factors_host[j]; the (layer, column) pairs strictly ascending, layer first.  Applied after the per-layer factor.
 *               The new value is bf16(fp32(x) * s), round to nearest even (0 * Inf = NaN).  A factor that is exactly 1.0 leaves its elements
 *               untouched (no read, no write); a layer whose factors are all 1 launches nothing.
 * One launch per option, form and armed layer; rows, columns and factors go to tables the context owns, on the pass's stream: nothing is allocated in
 * the pass.  An unarmed pass takes one untaken branch per MLP.  THE ROW-TRIMMED LAST LAYER: the value captured, patched or scaled for a row is the input
 * of the w2 launch whose output the pass keeps for that row - for the consumed rows of small clips that is the weight-streaming path's 64-row buffer,
 * for every other row of a mixed batch the tile path's.  When the last layer runs for the consumed rows only, a selected row it does not consume has no
 * MLP activation there: a patch or scale of it does nothing, and a capture does NOT write its (row, L - 1) slice - the caller fills it beforehand (the
 * Python host: NaN).  The last layer is not un-trimmed: the consumed rows' bits and every other output stay those of the plain pass.  All three combine
 * with each other, aigv_key_drop_arm / _ex, the score-attention probe, aigv_depth_lens_arm, the stream and head options and fp8 mode (the ops act on the
 * bf16 rows the e4m3 w2 consumes, before they are quantised).
 * Refused with AIGV_ERR_ARG and a message, nothing armed: a null context, n outside 0..max_tokens, a null row list (capture, patch), a null or
 * misaligned buffer, a column outside [0, I), a list that is not strictly ascending or longer than 4096, a NaN factor, a scale with neither form.
 * Refused by the pass, before any launch: a row outside [0, T), rows not strictly ascending, a window outside [0, L], keep_kv, an option that reaches
 * layer L - 1 in a pass without output rows (its last MLP does not run); aigv_llm_extend refuses an armed context. */
int aigv_neuron_capture_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, int lo, int hi, const int32_t* cols_host, int m, void* out_bf16_dev);
int aigv_neuron_patch_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, int lo, int hi, const int32_t* cols_host, int m, const void* values_bf16_dev);
int aigv_neuron_scale_arm(aigv_ctx* ctx, const int32_t* rows_host, int n, const float* layer_scale_host, const int32_t* sel_layers_host,
                          const int32_t* sel_cols_host, const float* sel_factors_host, int m);

/* Replicate the n kept sequences `copies` times (cache slots [0, n) -> [n, 2n), ...; needs n * copies <= max_seqs): the copies can
 * then take DIFFERENT continuations in one aigv_llm_extend call over n * copies sequences (sequence c * n + b continues clip b),
 * which streams the decoder weights once for all of them. */
int aigv_kv_fork(aigv_ctx* ctx, int copies, void* stream);
/* Beam search (HF generate(num_beams > 1): the cache reorder of GenerationMixin._beam_search, transformers/generation/utils.py; the
 * reference inherits it through language_model.generate, modeling_internvl_chat.py:798-809).  After this call kept sequence i holds
 * what sequence parent[i] had cached - its first len[i] positions - in every layer; parent / len are HOST arrays of n = the number of
 * kept sequences (aigv_llm_prefill(keep_kv) x aigv_kv_fork).  The positions aigv_decode_step keeps on the device are not touched: the
 * beams of one search all have the same length.  The first call allocates a second KV cache of the context's size (the gather is never
 * in place; the two caches swap). */
int aigv_kv_reorder(aigv_ctx* ctx, const int32_t* parent, const int32_t* len, int n, void* stream);

/* Arithmetic of the InternLM2 linears (aigv_llm_prefill, aigv_llm_extend, aigv_decode_step; BASELINE config 5).  AIGV_PRECISION_BF16 (default) is the reference's
 * dtype flow.  AIGV_PRECISION_FP8_LLM: wqkv, wo, w1|w3, w2 of every decoder layer - except wo / w1|w3 / w2 of the LAST layer, which act on
 * the few consumed rows - run on the e4m3 MFMA: weights quantised once per output channel (scale = amax / 448), activations per token row
 * on the fly (aigv_op_quant_fp8_rows), fp32 accumulation, the bf16 path's epilogues and rounding points after the scaled accumulator.
 * Attention, norms, RoPE, residual stream, lm-head and score head stay bf16.  aigv_llm_extend runs the same e4m3 linears as the
 * prefill (a continuation scores like the same tokens inside one prefill of this mode); aigv_decode_step streams the e4m3 copies too
 * (same rule: all but the post-attention half of the last layer; the token rows are normalised and quantised inside the GEMVs) for up
 * to 4 sequences and hidden / intermediate widths of 2048 j (j = 2, 3 / 2, 3, 7, 8), else it decodes from the bf16 weights.  The reference
 * has no fp8 path: results move by the quantisation noise (oracle/fp8.py restates this mode).  EXPERIMENTAL: over the 37 clips recorded from the
 * reference the mode's SCORES correlate with the reference's at SRCC 0.72 (bf16 path: 0.985) - not usable as scores on that evidence.
 * Every e4m3 linear of a pass is ONE launch in full K (round 6), so in this mode too a clip's bits do not depend on its batch mates.  First call
 * quantises the weights (extra memory: one byte per InternLM2 linear weight).  Needs H, qkv width, 2*I multiples of 256.
 * aigv_finalize_weights after a reload of an InternLM2 linear (wqkv / wo / w1 / w3 / w2 of any layer) drops the e4m3 copies and returns the
 * context to bf16: set the mode again after it.  A finalize that follows other uploads only (the rotary tables after aigv_ctx_resize, a
 * score head, ViT weights) keeps the copies and the mode. */
enum aigv_precision { AIGV_PRECISION_BF16 = 0, AIGV_PRECISION_FP8_LLM = 1 };
int aigv_set_precision(aigv_ctx* ctx, int mode);
/* Last-layer row trimming in aigv_llm_prefill (default on): when at most 16 rows per clip are consumed (score rows + logit rows), the
 * last decoder layer computes attention only for the query blocks holding them and finishes wo / MLP / final norm on a compact
 * copy of those rows.  Rows are independent after attention, so the outputs are those of the untrimmed pass (up to the fp32
 * summation order of the kernel that runs the few rows); off = every row through every layer, as the reference does. */
int aigv_set_row_trimming(aigv_ctx* ctx, int on);
/* Numerics of the prefill attention (InternViT and InternLM2): 0 (default) = the score matrix stays fp32 up to the softmax; 1 = it carries
 * the reference's rounding points - s = bf16(q k^T), InternLM2 also bf16(s / sqrt(d)) (modeling_internlm2.py:417,
 * modeling_intern_vit.py:153).  At op level form 1 sits 4x closer to the reference's eager bf16 result; END TO END, over the 37 clips the
 * imported reference was recorded on, it is NOT closer to the reference's scores (3.09 against 2.80 bf16 ulps mean; the reference moves
 * 2.56 against itself with the host's thread count), it is farther from the reference's fp32 scores (3.59 against 2.01) and it costs
 * 1.9 ms of a 116 ms step: profiles/r5_parity_stats.txt.  P is rounded un-normalised in both forms (no measurable effect). */
#define AIGV_ATTENTION_NUMERICS_DEFAULT 0
int aigv_set_attention_numerics(aigv_ctx* ctx, int mode);
/* The mode in force for `ctx`; ctx == NULL: the mode a fresh context starts in (AIGV_ATTENTION_NUMERICS_DEFAULT; needs no GPU - the host
 * tests hold INTEGRATION.md's "default" sentence against it). */
int aigv_get_attention_numerics(const aigv_ctx* ctx);
/* GEMM tile choice of THIS context: -1 = follow the process default set by aigv_tune_gemm (the state after aigv_ctx_create),
 * 0 = the per-sequence row plan (aigv_op_gemm_rows: the default; a clip's / frame's bits do not depend on its batch mates),
 * 1 = every row on the 128x128 kernel, 2 = every row on the 256x256 kernel wherever its shape rules allow, 4 = every row on the
 * co-resident 256x128 kernel (all three in full K, so batch-invariant too and bit-identical with one another: test aliases).  The
 * co-resident kernel is otherwise NOT used: AIGV_TUNE_CO_KMAX defaults to 0 (it lost the in-step A/B, profiles/r5_gemmco.txt); an experiment
 * that raises the knob sends the GEMMs with K <= its value there in modes 0 and 3.  Split-K scratch is per context too.  aigv_llm_extend (continuations of a kept
 * prefix) still uses the batch-level cost-model dispatch of aigv_op_gemm. */
int aigv_set_gemm_mode(aigv_ctx* ctx, int mode);

/* One greedy decode step for every clip of the last keep_kv prefill (generate(): modeling_internvl_chat.py:769-811,
 * modeling_internlm2.py:1126-1163).  ids[B] int64 device (the previous tokens) -> next[B] int64 device. */
int aigv_decode_step(aigv_ctx* ctx, const int64_t* ids, int64_t* next, void* stream);
/* aigv_decode_step plus the log-probability of each raw token it emits: logprob[b] = log_softmax(logits.float())[next[b]] of the bf16
 * lm-head logits (DEVICE fp32 [B]).  The lm-head GEMV computes the log-sum-exp in the same pass as its argmax (per-16-column partials in a
 * context workspace, merged in a fixed order: a sequence's bits do not depend on its batch mates); next is aigv_decode_step's, bit for bit.
 * Nothing is allocated here, so the call may be captured. */
int aigv_decode_step_logprob(aigv_ctx* ctx, const int64_t* ids, int64_t* next, float* logprob, void* stream);
/* aigv_decode_step_logprob plus the log-probabilities of C chosen tokens at every step: cand_logprob[b, c] = log_softmax(logits.float())
 * [cand_ids[c]] over the FULL vocabulary (DEVICE fp32 [B, C]; cand_ids: DEVICE int64 [C], 1 <= C <= AIGV_MAX_CANDIDATES; an id outside
 * [0, vocab) gives a NaN column).  The log-sum-exp is the one `logprob` uses; the C logits come from a second, tiny GEMV over just those C
 * rows of the lm-head weight (ceil16(C) x hidden x 2 extra weight bytes per step) whose arithmetic gives each column the bits the lm-head
 * itself rounds for it - a candidate that is the step's argmax carries logprob[b], bit for bit.  next / logprob are
 * aigv_decode_step_logprob's bits.  Nothing is allocated here, so the call may be captured. */
int aigv_decode_step_cand_logprob(aigv_ctx* ctx, const int64_t* ids, int64_t* next, float* logprob, const int64_t* cand_ids, int C,
                                  float* cand_logprob, void* stream);
/* aigv_decode_step_logprob plus the k most likely tokens of every step: top_ids[b, j] (DEVICE int64 [B, k]) is the id of the j-th largest
 * bf16 lm-head logit of sequence b - equal logits by ascending id, the order of the fused argmax, so top_ids[b, 0] == next[b] - and
 * top_logprob[b, j] (DEVICE fp32 [B, k]) = log_softmax(logits.float())[top_ids[b, j]] under the log-sum-exp `logprob` uses:
 * top_logprob[b, 0] is logprob[b], bit for bit.  1 <= k <= min(AIGV_MAX_TOPK, vocab).  The lm-head weights are read once: the GEMV that
 * reduces the logits also stores them (bf16, a context-owned scratch) and the finisher selects from that row.  Candidates are optional:
 * cand_ids == NULL with C == 0, or aigv_decode_step_cand_logprob's arguments and bits.  next / logprob are aigv_decode_step_logprob's
 * bits; a sequence's results do not depend on its batch mates nor on k.  Nothing is allocated here, so the call may be captured. */
int aigv_decode_step_topk_logprob(aigv_ctx* ctx, const int64_t* ids, int64_t* next, float* logprob, int k, int64_t* top_ids,
                                  float* top_logprob, const int64_t* cand_ids, int C, float* cand_logprob, void* stream);
/* The full next-token distribution of the rows the last aigv_llm_prefill / aigv_llm_extend / aigv_decode_step consumed: lm-head
 * logits of their final hidden states (kept in the context, in the order [score rows | logit rows]; a decode step keeps its
 * n_clips rows) as the bf16 values the reference upcasts with .float() (modeling_internlm2.py:1095-1096).
 * logits: DEVICE bf16 [n_rows, ldo], ldo >= vocab rounded up to a multiple of 4 (columns >= vocab are padding).  For
 * generate() with do_sample (HF sampling needs the distribution; the greedy paths use the fused argmax and never call this). */
int aigv_out_row_logits(aigv_ctx* ctx, int first_row, int n_rows, void* logits_bf16, int ldo, void* stream);
/* The final hidden states (after the last RMSNorm, modeling_internlm2.py:984) of the same rows, bf16 [n_rows, ldo >= llm_hidden]: for the
 * score rows this is the reference's hidden_states[-1][:, -4, :], the input of its score head (modeling_internvl_chat.py:469-481) - the
 * slice of `output_hidden_states=True` the eval path consumes.  Rows in the order [score rows | logit rows]. */
int aigv_out_row_hidden(aigv_ctx* ctx, int first_row, int n_rows, void* hidden_bf16, int ldo, void* stream);
/* Label log-probabilities of the same rows: logprob[i] = log_softmax(logits.float())[labels[i]] of row first_row + i, the per-token term of
 * the reference's CrossEntropyLoss over the answer tokens (internvl_chat_eval2/modeling_internvl_chat.py:452-463; stage-1 training
 * minimises its mean, internvl_chat_stage1_lora/modeling_internvl_chat.py:386-398).  logits: the bf16 lm-head output that the reference
 * upcasts (modeling_internlm2.py:1095-1096), computed again per 64 rows into a context-owned scratch (allocated with the workspaces:
 * nothing is allocated here, so the call may be captured into a graph) - the 4-slice form of the fused argmax for every row count, so a
 * row's value does not depend on its batch mates.  The softmax runs in fp32: online max and sum of exponentials per lane, reduced in a
 * fixed order.  labels: DEVICE int64 [n_rows]; a label outside [0, vocab) (-100 included) gives NaN.  logprob: DEVICE fp32 [n_rows].
 * Rows in the order [score rows | logit rows], as aigv_out_row_logits. */
int aigv_out_row_logprob(aigv_ctx* ctx, int first_row, int n_rows, const int64_t* labels, float* logprob, void* stream);
/* Candidate-token log-probabilities of the same rows: cand_logprob[i, c] = log_softmax(logits.float())[cand_ids[c]] of row first_row + i
 * over the FULL vocabulary - aigv_out_row_logprob's logits, scratch, arithmetic and log-sum-exp, read at C columns, so column c holds the
 * bits aigv_out_row_logprob gives with labels = cand_ids[c] and a row's bits depend on neither n_rows nor C.  cand_ids: DEVICE int64 [C],
 * 1 <= C <= AIGV_MAX_CANDIDATES (the first answer tokens of the quality-level words: softmax over the C columns is the closed-set
 * level distribution); an id outside [0, vocab) gives a NaN column.  cand_logprob: DEVICE fp32 [n_rows, C].  Nothing is allocated here. */
int aigv_out_row_cand_logprob(aigv_ctx* ctx, int first_row, int n_rows, const int64_t* cand_ids, int C, float* cand_logprob, void* stream);
/* The k most likely tokens of the same rows: top_ids[i, j] (DEVICE int64 [n_rows, k]) is the id of the j-th largest bf16 logit of row
 * first_row + i, equal logits by ascending id (torch.sort(logits.float(), descending=True, stable=True) states the rule; entry 0 is
 * the fused argmax's token), and top_logprob[i, j] (DEVICE fp32 [n_rows, k]) = log_softmax(logits.float())[top_ids[i, j]] -
 * aigv_out_row_logprob's logits, scratch, arithmetic and log-sum-exp, so column j holds the bits aigv_out_row_logprob /
 * aigv_out_row_cand_logprob give for that id and a row's results depend on neither n_rows nor k (the first columns of a larger k are the
 * smaller k's).  1 <= k <= min(AIGV_MAX_TOPK, vocab).  Nothing is allocated here. */
int aigv_out_row_topk_logprob(aigv_ctx* ctx, int first_row, int n_rows, int k, int64_t* top_ids, float* top_logprob, void* stream);
/* End-of-sequence bookkeeping of generate()'s token loop on the device (the reference defers to HF's loop: next = next * unfinished +
 * pad * (1 - unfinished); unfinished &= next not in eos_token_id; stop when every sequence has finished - modeling_internvl_chat.py:
 * 798-809).  tokens: DEVICE int64[n] (n = sequences of the kept KV state), in: the step's raw tokens (aigv_decode_step's `next`, or the
 * prefill's argmax), out: the tokens the loop emits (pad_id for finished sequences).  state: DEVICE int32[n + 1], zeroed by the caller
 * before the first token: state[b] = 1 once sequence b has emitted an end token, state[n] = number of emitted columns in which some
 * sequence was still live (the output length HF returns).  eos_ids: HOST, at most 8.  The host reads `state` only every few tokens,
 * so the loop runs without a per-token host synchronisation. */
int aigv_decode_eos(aigv_ctx* ctx, int64_t* tokens, int32_t* state, const int64_t* eos_ids, int n_eos, int64_t pad_id, void* stream);

/* ---- single operators (parity tests call these through the same ABI) --------------------------------- */
/* C = epilogue(A[M,K] . W[N,K]^T); epi: 0 store, 1 gelu, 2 layerscale+residual, 3 residual, 4 swiglu, 5 patch
 * Row strides, in bf16 elements, for aigv_op_gemm, _gemm_rows, _gemm_splitk and _gemm_splitk256 alike (refused with AIGV_ERR_ARG before
 * any launch otherwise): lda, ldw >= K; ldc >= the output width (N, or N / 2 for swiglu); ldr >= that width whenever resid is given;
 * all four multiples of 8 - the dispatcher may run any rows of a call on any tile kernel, and the 256x256 and the co-resident kernels
 * move 16 bytes at C + row * ldc + n and at resid + row * ldr + n.  resid may alias C (then ldr == ldc). */
int aigv_op_gemm(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* ls,
                 const void* resid, int ldr, const void* pos, int np, int M, int N, int K, int epi, void* stream);
/* That argument check alone (host only: nothing is launched, no pointer is dereferenced): 0, or AIGV_ERR_ARG and the refusal in
 * aigv_last_error(NULL).  aigv_op_skinny_gemm_check is the same for aigv_op_skinny_gemm. */
int aigv_op_gemm_check(const void* A, int lda, const void* W, int ldw, const void* C, int ldc, const void* bias, const void* ls,
                       const void* resid, int ldr, const void* pos, int np, int M, int N, int K, int epi);
int aigv_op_skinny_gemm_check(const void* x, int ldx, int R, const void* W, int ldw, int N, int K, const void* resid, int ldr,
                              const void* out, int ldo, int epi);
/* The same GEMM with its M = cu_host[n_seq] rows divided into n_seq independent sequences (HOST int32 cu_host[0..n_seq], cu[0] = 0; epi
 * 0..4): the dispatch of the scoring pass.  Every sequence's rows [0, 256 * floor(L / 256)) run in full K as whole tiles addressed
 * through a half-tile table on the 256x256 kernel (AIGV_TUNE_BODY_TILE = 2: on the 128x128 kernel, which sums every element in the same
 * order - same bits, a test alias), its remaining rows as (ragged) half tiles with a split-K factor that depends on (N, K)
 * only, remainders of <= 4 rows on the weight-streaming kernel in its fixed form - a row's result depends on its own sequence alone,
 * never on the other sequences of the call.  Synchronises the stream (test entry point). */
int aigv_op_gemm_rows(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* ls,
                      const void* resid, int ldr, const int32_t* cu_host, int n_seq, int N, int K, int epi, void* stream);
/* the split-K form used for latency-bound row tails: k_slices x tiles write fp32 slabs into ws_f32 (k_slices*M*N floats),
 * one pass sums them in slice order and applies the epilogue (epi 0..4) */
int aigv_op_gemm_splitk(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* ls,
                        const void* resid, int ldr, int M, int N, int K, int epi, int k_slices, void* ws_f32, void* stream);
/* the same with the slices computed by the 256x256 kernel (N % 256 == 0): whole row tiles that would not fill a round */
int aigv_op_gemm_splitk256(const void* A, int lda, const void* W, int ldw, void* C, int ldc, const void* bias, const void* ls,
                           const void* resid, int ldr, int M, int N, int K, int epi, int k_slices, void* ws_f32, void* stream);
/* fp8 groundwork for BASELINE config 5 (NOT used by the bf16 scoring path; the reference has no fp8 path, so these two are defined by
 * their own arithmetic and tested against a torch restatement of it):
 *   aigv_op_quant_fp8_rows: bf16 [rows, K] -> OCP e4m3 bytes [rows, K] + row_scale[rows] = amax / 448 (1 for an all-zero row);
 *                           q = e4m3_rne(x * (448 / amax)), three fp32 operations, round-to-nearest-even.  K % 8 == 0.
 *   aigv_op_gemm_fp8:       C[M, N] = bf16((sum_k A[m,k] W[n,k]) * row_scale[m] * col_scale[n] + bias[n]) with e4m3 A [M, K] and
 *                           W [N, K] (K contiguous), products exact and accumulated in fp32 on v_mfma_scale_f32_16x16x128_f8f6f4
 *                           (unit block scales) with the 256x256 schedule of the bf16 kernel.  N % 256 == 0, K % 128 == 0,
 *                           lda / ldw in bytes and multiples of 16; row_scale / col_scale DEVICE float.  epi = AIGV_EPI_STORE, _GELU,
 *                           _LS_RESID, _RESID or _SWIGLU: the scaled accumulator takes the place of the bf16 kernel's accumulator,
 *                           every later rounding point is that of aigv_op_gemm. */
int aigv_op_quant_fp8_rows(const void* x_bf16, int ldx, int rows, int K, void* q_e4m3, int ldq, float* row_scale, void* stream);
int aigv_op_gemm_fp8(const void* A_e4m3, int lda, const void* W_e4m3, int ldw, void* C, int ldc, const float* row_scale,
                     const float* col_scale, const void* bias, const void* ls, const void* resid, int ldr, int M, int N, int K, int epi,
                     int k_slices, void* ws_f32, void* stream);   /* k_slices > 1: split-K, ws_f32 = k_slices * M * N floats, K/128 % k_slices == 0 */
/* The weight-streaming GEMM of R <= 64 rows.  Row strides in bf16 elements (refused with AIGV_ERR_ARG before any launch otherwise): ldx,
 * ldw >= K and multiples of 8; ldo >= the output width (N, or N / 2 for swiglu) and a multiple of 4; ldr the same whenever resid is given
 * (the kernel moves 8 bytes at out + row * ldo + n and at resid + row * ldr + n). */
int aigv_op_skinny_gemm(const void* x, int ldx, int R, const void* W, int ldw, int N, int K, const void* bias,
                        const void* resid, int ldr, void* out, int ldo, int epi, void* stream);
/* The e4m3 form of a decode GEMV (fp8 mode; what aigv_decode_step runs per linear after aigv_set_precision(fp8)): R <= 4 bf16 rows x
 * [R, K] are (optionally RMS-normalised with norm_w / eps, then) quantised per row inside the kernel, W_e4m3 [N, ldw bytes] with one
 * fp32 scale per output channel, out = epilogue(bf16((acc * row scale) * channel scale)).  epi: 1 residual, 2 swiglu (w1|w3 in 16-row
 * blocks; needs norm_w).  K = 2048 j, j in {2, 3} with a norm, {2, 3, 7, 8} without; p = 1 / 2 / 4: 16 / 8 / 4 rows of W per workgroup
 * (R <= 16 / p). */
int aigv_op_skinny_gemm_fp8(const void* x, int ldx, int R, const void* W_e4m3, int ldw, const float* w_scale, int N, int K, const void* resid,
                            int ldr, void* out, int ldo, int epi, const void* norm_w, float eps, int p, void* stream);
/* The norm kernels, rows of H bf16 (H a multiple of 8, 8..16384; ldx, ldy >= H, multiples of 8; every operand 16-byte aligned):
 *   layernorm  y = bf16((x - mean) * rstd * w + b), fp32 statistics, one rounding
 *   rmsnorm    y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))); row_idx (DEVICE int32[rows], may be NULL): row i of y from row row_idx[i] of x.
 *              y == x with ldy == ldx and no row_idx is allowed (the InternViT qk-norm runs in place on the middle third of its qkv rows).
 * Checked on the host (AIGV_ERR_ARG) before anything is launched. */
int aigv_op_layernorm(const void* x, int ldx, const void* w, const void* b, void* y, int ldy, int rows, int H,
                      float eps, void* stream);
int aigv_op_rmsnorm(const void* x, int ldx, const void* w, void* y, int ldy, int rows, int H, float eps,
                    const int32_t* row_idx, void* stream);
int aigv_op_rope(void* qkv, int ld, const int32_t* pos, const void* cos, const void* sin, int tokens, int n_rot,
                 int slots, int n_groups, int head_dim, void* stream);
/* q/k/v as in kernels.h AttnArgs; cu is a DEVICE int32[n_seq+1].  causal: bit 0 = causal mask; bit 1 = "every sequence has
 * exactly max_len rows" (InternViT frames), which lets the dispatcher give a short left-over query block to the key-split kernel;
 * bit 2 = the score matrix rounds to bf16 as in the reference's eager path (aigv_set_attention_numerics mode 1); bit 3 = the
 * lead-key form for non-causal key counts 64 j + 1 (full tiles over keys 1.., key 0 merged in the epilogue; opt-in, off in the scoring pass). */
int aigv_op_attention(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                      const int32_t* cu, int n_seq, int max_len, int n_heads, int n_kv_heads, int q_group_stride,
                      int kv_head_stride, int head_dim, int causal, float post_div, float q_prescale, void* stream);
/* the same with RoPE applied to the QUERY rows as they are loaded (pos: DEVICE int32 position of every packed row; cos/sin:
 * DEVICE bf16 [max_pos, head_dim/2]; three bf16 roundings as aigv_op_rope).  K must already be rotated in memory. */
int aigv_op_attention_rope(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo,
                           const int32_t* cu, int n_seq, int max_len, int n_heads, int n_kv_heads, int q_group_stride,
                           int kv_head_stride, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos,
                           const void* cos, const void* sin, void* stream);
/* aigv_op_attention_rope plus the address and mask forms of the scoring passes (parity tests: tests/test_gpu_attention_forms.py):
 *   kv_seq_stride  elements; 0 = K / V packed like the query rows, else K / V of sequence s start s * kv_seq_stride elements behind k / v
 *                  (the KV cache [seq][kv head][cap][head_dim]: ldk = ldv = head_dim, kv_head_stride = cap * head_dim)
 *   kv_off         DEVICE int32[n_seq] or NULL: keys in front of each sequence's first query row (a continuation); needs kv_seq_stride.
 *                  Query row r of sequence s sees keys 0 .. kv_off[s] + r of kv_off[s] + len[s] keys.
 *   pos_is_row     != 0: the rotary position of query row r is kv_off[s] + r, computed by the kernel (pos is not read); 0: pos[row]
 *   q_tail         > 0: only the last q_tail query rows of every sequence are consumed: rows of whole 32-row waves in front of them are
 *                  left unwritten, the others are computed as with q_tail = 0
 * The arguments are checked on the host before anything is launched (AIGV_ERR_ARG with a message naming the op). */
int aigv_op_attention_ex(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                         int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                         const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                         const void* sin, int pos_is_row, int q_tail, void* stream);
/* aigv_op_attention_ex under a key-drop mask (tests/test_gpu_key_drop.py): key_drop DEVICE uint64 [n_seq][ld_drop] or NULL (then the same call as
 * aigv_op_attention_ex, the same kernels).  Bit (j & 63) of word key_drop[s * ld_drop + (j >> 6)] set = key j of sequence s is invisible to every
 * query row and head; j is the key's absolute position in its sequence, cached keys first, so the packed form and the cache form (kv_off,
 * kv_seq_stride) share one indexing.  A query row without a visible key is written as zeros.  Dropped keys' V rows must be finite.  Refused
 * with AIGV_ERR_ARG and a message: key_drop with causal == 0 or head_dim != 128, a misaligned key_drop, and ld_drop < ceil((largest kv_off +
 * max_len) / 64) - with kv_off the entry point reads the offsets back from the device for that check (it synchronises the stream; at most 256
 * sequences). */
int aigv_op_attention_drop(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                           int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                           const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                           const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, int ld_drop, void* stream);
/* aigv_op_attention_drop with a row selector (tests/test_gpu_key_drop_rows.py): row_words DEVICE uint64 [n_seq][ld_drop] in key_drop's layout, or
 * NULL (then the same call as aigv_op_attention_drop, the same kernels).  Bit (i & 63) of word row_words[s * ld_drop + (i >> 6)] set = query row i
 * of sequence s is subject to key_drop; a score is hidden iff its key's bit and its row's bit are both set.  The packed prefill form only.
 * Refused with AIGV_ERR_ARG and a message, before anything is launched: what aigv_op_attention_drop refuses, row_words without key_drop, row_words
 * with kv_off or kv_seq_stride, and misaligned row_words. */
int aigv_op_attention_drop_rows(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu,
                                int n_seq, int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                                const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos,
                                const void* cos, const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, const uint64_t* row_words,
                                int ld_drop, void* stream);
/* aigv_op_attention_ex under the NON-causal key-drop mask (tests/test_gpu_vit_key_drop.py; head_dim 64 or 128): key_drop in aigv_op_attention_drop's
 * layout, or NULL (then the same call as aigv_op_attention_ex).  A dropped key is hidden from every query row, its own included; a row without a
 * visible key is written as zeros; dropped keys' V rows must be finite; bits at or past a sequence's length are ignored.  The masked kernel ignores
 * the lead-key bit of `causal`: under a zero mask its output is that of aigv_op_attention_ex with the bit clear.  Refused with AIGV_ERR_ARG and a
 * message, before anything is launched: causal != 0, key_drop with kv_off, kv_seq_stride or q_tail, a misaligned key_drop, ld_drop <
 * ceil(max_len / 64). */
int aigv_op_attention_nc_drop(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* o, int ldo, const int32_t* cu, int n_seq,
                              int max_len, int n_heads, int n_kv_heads, int q_group_stride, int kv_head_stride, int64_t kv_seq_stride,
                              const int32_t* kv_off, int head_dim, int causal, float post_div, float q_prescale, const int32_t* pos, const void* cos,
                              const void* sin, int pos_is_row, int q_tail, const uint64_t* key_drop, int ld_drop, void* stream);
/* The score-row attention probe on plain pointers (one layer; tests use it without a model): out [n_rows, n_heads, n_segments] fp32 as
 * aigv_score_attention_arm defines it.  q: UNROTATED fused rows (query head h at column (h / g) * q_group_stride + (h % g) * head_dim), rotated
 * by the kernel at the row's position from cos / sin [max_pos, head_dim / 2]; k: already rotated, in aigv_op_attention_ex's two forms -
 * packed (kv_seq_stride = 0, kv_off_host = NULL: key j of a sequence is its row j) or the KV cache (kv_seq_stride != 0: ldk = head_dim,
 * kv_head_stride = cap * head_dim; the row at local index r of sequence s sees cache positions [0, kv_off_host[s] + r]).  cu_host / kv_off_host /
 * rows_host are HOST arrays, so that every index the kernel forms is checked before anything is launched (AIGV_ERR_ARG with a message); seg_new
 * DEVICE int32[cu_host[n_seq]], seg_cached DEVICE int32[n_seq * ld_cached] or NULL.  head_dim 64 or 128. */
int aigv_op_attention_probe(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                            int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim, const void* cos,
                            const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new, const int32_t* seg_cached,
                            int ld_cached, int n_segments, float* out, void* stream);
/* aigv_op_attention_probe with the dense per-key output of aigv_score_attention_arm_tokens from the same launch: tok_out [n_rows, n_heads,
 * ld_tok] fp32 DEVICE (one layer).  Refused on the host (AIGV_ERR_ARG with a message, nothing launched) when ld_tok is below the largest
 * position + 1 over the probe rows or above AIGV_MAX_KV_CAPACITY, or when tok_out is NULL while ld_tok > 0; tok_out = NULL with ld_tok = 0
 * is aigv_op_attention_probe.  `out` keeps its bits. */
int aigv_op_attention_probe_tokens(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                                   int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim,
                                   const void* cos, const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new,
                                   const int32_t* seg_cached, int ld_cached, int n_segments, float* out, float* tok_out, int ld_tok, void* stream);
/* aigv_op_attention_probe_tokens with the value vectors of aigv_score_attention_arm_values from the same launch: val_out [n_rows, n_heads,
 * n_segments + 1, head_dim] fp32 DEVICE (one layer).  v: bf16 V rows in k's addressing form - packed: row j of a sequence, ldv apart, kv head
 * kvh at column kvh * kv_head_stride (for fused rows: k + head_dim); cache: [seq][kv head][cap][head_dim] with k's strides (ldv = ldk).
 * tok_out may be NULL with ld_tok = 0.  Refused on the host (AIGV_ERR_ARG with a message, nothing launched): v or val_out NULL, v not
 * 16-byte aligned or ldv not a multiple of 8, strides that do not hold the rows.  `out` and `tok_out` keep their bits. */
int aigv_op_attention_probe_values(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                                   int q_group_stride, int kv_head_stride, int64_t kv_seq_stride, const int32_t* kv_off_host, int head_dim,
                                   const void* cos, const void* sin, int max_pos, const int32_t* rows_host, int n_rows, const int32_t* seg_new,
                                   const int32_t* seg_cached, int ld_cached, int n_segments, float* out, float* tok_out, int ld_tok, const void* v, int ldv,
                                   float* val_out, void* stream);
/* The attention flow map's two kernels on plain pointers, no context (tests): rows_out [cu_host[n_seq], n_heads, n_segments] as
 * aigv_attention_map_arm defines one layer of rows_out_dev; seg_out (may be NULL) [n_seq, n_heads, n_segments, n_segments] the fold of those
 * rows.  q / k / cos / sin / the strides: aigv_op_attention_probe's packed form (q UNROTATED fused rows, k rotated), seg: DEVICE int32
 * [cu_host[n_seq]], 1 <= n_seq <= 127.  Refused on the host (AIGV_ERR_ARG with a message, nothing launched): a null operand, head_dim other
 * than 64 / 128, n_segments outside 1..AIGV_MAX_ATTN_SEGMENTS, q / k / the tables not 16-byte aligned or strides that are no multiple of 8 or
 * do not hold the rows, an empty sequence, a sequence longer than max_pos. */
int aigv_op_attention_map(const void* q, int ldq, const void* k, int ldk, const int32_t* cu_host, int n_seq, int n_heads, int n_kv_heads,
                          int q_group_stride, int kv_head_stride, int head_dim, const void* cos, const void* sin, int max_pos, const int32_t* seg,
                          int n_segments, float* rows_out, float* seg_out, void* stream);
/* The InternViT attention map's two kernels on plain pointers, no context (tests): the quantity aigv_vit_attention_arm defines, for n_seq
 * frames of S consecutive rows each; head h sits at column h * head_dim of a row of q (row stride ldq) and of k (ldk).  out: fp32
 * [n_seq][S][S], per_head: [n_seq][n_heads][S][S].  stats_scratch: DEVICE, 8-byte aligned, n_seq * n_heads * S * 2 floats, overwritten.
 * Refused on the host (AIGV_ERR_ARG with a message, nothing launched, nothing written): a null operand, head_dim other than 64 / 128, n_heads
 * outside 1..64, n_seq outside 1..65535, S outside 1..32768, q / k not 16-byte aligned or row strides that are no multiple of 8 or do not
 * hold n_heads * head_dim columns, a misaligned out / stats_scratch. */
int aigv_op_vit_attention_map(const void* q, int ldq, const void* k, int ldk, int n_seq, int S, int n_heads, int head_dim, float* out,
                              int per_head, void* stats_scratch, void* stream);
/* The KV-cache append of the prefill and continuation passes: for token t, the K and V slots of every group of the fused row
 * qkv[t * ld ..] (groups of [g query heads | K | V]) are copied to kc / vc [seq][n_kv][cap][head_dim] at [seq[t]][kvh][pos[t]]; nothing else
 * is written.  seq / pos: DEVICE int32[tokens] (the caller's promise: seq[t] inside the cache, pos[t] < cap).  Checked on the host. */
int aigv_op_kv_store(const void* qkv, int ld, const int32_t* seq, const int32_t* pos, void* kc, void* vc, int tokens, int n_kv, int g,
                     int head_dim, int cap, void* stream);
/* pixel_shuffle: vit_out [n_frames, grid^2 + 1, vit_hidden] -> out [n_frames * (grid / 2)^2, 4 * vit_hidden], the cls row dropped (grid even,
 * vit_hidden a multiple of 8).  im2col: frames [n_frames, channels, image_size, image_size] -> out [n_frames * (image_size / patch)^2, kp], columns
 * from channels * patch^2 on zero (image_size a multiple of patch, kp >= channels * patch^2).  Operands 16-byte aligned; checked on the host. */
int aigv_op_pixel_shuffle(const void* vit_out, int grid, int vit_hidden, void* out, int n_frames, void* stream);
int aigv_op_im2col(const void* frames, int n_frames, int channels, int image_size, int patch, int kp, void* out,
                   void* stream);
int aigv_op_lm_head_argmax(const void* h, int rows, int hidden, const void* W, int vocab, void* scratch_u64,
                           int64_t* idx, float* val, void* stream);
/* aigv_op_lm_head_argmax plus the log-probability of the chosen column (the lm-head of aigv_decode_step_logprob): idx / val are
 * aigv_op_lm_head_argmax's bits (first maximal bf16-rounded logit), logprob[r] = val[r] - logsumexp(bf16-rounded logits of row r) in fp32;
 * val may be null.  rows 1..64, hidden a multiple of 128, h / W / scratch 16-byte aligned; scratch: DEVICE memory of
 * aigv_op_lm_head_argmax_logprob_scratch_bytes(rows, vocab) bytes (scratch_bytes = its size; a smaller one is refused).  Arguments are
 * checked on the host (AIGV_ERR_ARG) before anything is launched. */
int aigv_op_lm_head_argmax_logprob(const void* h, int rows, int hidden, const void* W, int vocab, void* scratch, int64_t scratch_bytes,
                                   int64_t* idx, float* val, float* logprob, void* stream);
int64_t aigv_op_lm_head_argmax_logprob_scratch_bytes(int rows, int vocab);   /* -1 for arguments the op refuses */
/* The log-softmax of aigv_out_row_logprob on caller-supplied bf16 logits [rows, ldo >= vocab]: out[r] = fp32 log_softmax(logits[r, :vocab])
 * [labels[r]], NaN where labels[r] is outside [0, vocab).  One workgroup per row; the bits of a row do not depend on `rows`. */
int aigv_op_label_logprob(const void* logits_bf16, int rows, int vocab, int ldo, const int64_t* labels, float* out, void* stream);
/* aigv_op_label_logprob at C columns: out[r, c] = fp32 log_softmax(logits[r, :vocab])[cand_ids[c]] (out: DEVICE fp32 [rows, C]; cand_ids:
 * DEVICE int64 [C], 1 <= C <= AIGV_MAX_CANDIDATES; NaN columns for ids outside [0, vocab)).  Column c holds aigv_op_label_logprob's bits
 * for labels = cand_ids[c]; they depend on neither `rows`, C nor the candidates' order. */
int aigv_op_cand_logprob(const void* logits_bf16, int rows, int vocab, int ldo, const int64_t* cand_ids, int C, float* out, void* stream);
/* The lm-head of aigv_decode_step_cand_logprob: aigv_op_lm_head_argmax_logprob (idx / val / logprob: its bits, its argument rules) plus
 * cand_logprob[r, c] = bf16 lm-head logit of column cand_ids[c] - the row's log-sum-exp (DEVICE fp32 [rows, C]).  scratch: DEVICE memory
 * of aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(rows, vocab) bytes. */
int aigv_op_lm_head_argmax_cand_logprob(const void* h, int rows, int hidden, const void* W, int vocab, const int64_t* cand_ids, int C,
                                        void* scratch, int64_t scratch_bytes, int64_t* idx, float* val, float* logprob, float* cand_logprob,
                                        void* stream);
int64_t aigv_op_lm_head_argmax_cand_logprob_scratch_bytes(int rows, int vocab);   /* -1 for arguments the op refuses */
/* aigv_op_label_logprob's kernel selecting instead of gathering: the k largest logits of every row, equal logits by ascending column
 * (top_ids: DEVICE int64 [rows, k]), and their fp32 log-probabilities (top_logprob: DEVICE fp32 [rows, k]); 1 <= k <= min(AIGV_MAX_TOPK,
 * vocab).  Column j holds aigv_op_label_logprob's / aigv_op_cand_logprob's bits for the id it names; results depend on neither `rows`,
 * k nor the alignment of the rows. */
int aigv_op_topk_logprob(const void* logits_bf16, int rows, int vocab, int ldo, int k, int64_t* top_ids, float* top_logprob, void* stream);
/* The lm-head of aigv_decode_step_topk_logprob: aigv_op_lm_head_argmax_logprob (idx / val / logprob: its bits, its argument rules) plus
 * top_ids / top_logprob [rows, k] and, with cand_ids != NULL (else C == 0), aigv_op_lm_head_argmax_cand_logprob's cand_logprob.
 * scratch: DEVICE memory of aigv_op_lm_head_argmax_topk_logprob_scratch_bytes(rows, vocab) bytes. */
int aigv_op_lm_head_argmax_topk_logprob(const void* h, int rows, int hidden, const void* W, int vocab, int k, const int64_t* cand_ids, int C,
                                        void* scratch, int64_t scratch_bytes, int64_t* idx, float* val, float* logprob, int64_t* top_ids,
                                        float* top_logprob, float* cand_logprob, void* stream);
int64_t aigv_op_lm_head_argmax_topk_logprob_scratch_bytes(int rows, int vocab);   /* -1 for arguments the op refuses */

/* ---- the kernels of aigv_decode_step, one by one (parity tests; ABI 3) ----------------------------------------------------------------
 * Every pointer is DEVICE memory; the arguments are checked on the host before anything is launched (AIGV_ERR_ARG with a message
 * naming the op); device-side values (kv_lens, pos, seq) are the caller's promise.
 *
 * Split-KV decode attention (head_dim 128, g = 1..8 query heads per KV head): for sequence b and query head h = kvh * g + j,
 *   o[b * ldo + h * 128 + d] = bf16(softmax(q k^T / post_div) v) over keys 0 .. kv_lens[b] - 1 of kc / vc [n_seq][n_kv][cap][128],
 * q[b * ldq + kvh * q_group_stride + j * 128 + d] (the fused wqkv row).  The eager path's rounding points: scores -> bf16,
 * / post_div -> bf16, fp32 softmax with P -> bf16 per 128-key chunk, chunks merged in fp32.  1 <= kv_lens[b] <= max_kv_len <= cap
 * <= AIGV_MAX_KV_CAPACITY.  ws: fp32 scratch of aigv_op_attention_decode_ws_floats(n_seq, n_kv, g, cap) floats (ws_floats = its
 * size; a smaller one is refused) = n_seq * n_kv * ceil(cap / 128) * g * 130. */
int aigv_op_attention_decode(const void* q, int ldq, int q_group_stride, const void* kc, const void* vc, const int32_t* kv_lens, int cap,
                             void* o, int ldo, int n_seq, int n_kv, int g, int head_dim, float post_div, int max_kv_len, float* ws,
                             int64_t ws_floats, void* stream);
int64_t aigv_op_attention_decode_ws_floats(int n_seq, int n_kv, int g, int cap);   /* -1 for arguments the op refuses */
/* aigv_op_attention_decode under a key-drop mask (tests/test_gpu_key_drop_cache.py): key_drop DEVICE uint64 [n_seq][ld_drop] or NULL (then the same
 * call as aigv_op_attention_decode, the same kernels).  Bit (j & 63) of word key_drop[b * ld_drop + (j >> 6)] set = key j of sequence b is
 * invisible to all its query heads; bits at or past kv_lens[b] are ignored.  A dropped key's K row is not read (it may hold anything); its V row,
 * inside a 128-key chunk that keeps a visible key, is multiplied by an exact 0 and must be finite; a chunk without a visible key is not read at
 * all.  A sequence without a visible key is written as zeros.  An all-zero mask gives aigv_op_attention_decode's bits.  Refused with
 * AIGV_ERR_ARG and a message: a key_drop that is not 8-byte aligned, and ld_drop < ceil(max_kv_len / 64). */
int aigv_op_attention_decode_drop(const void* q, int ldq, int q_group_stride, const void* kc, const void* vc, const int32_t* kv_lens, int cap,
                                  void* o, int ldo, int n_seq, int n_kv, int g, int head_dim, float post_div, int max_kv_len, float* ws,
                                  int64_t ws_floats, const uint64_t* key_drop, int ld_drop, void* stream);
/* The wqkv GEMV of a decode step with RoPE and the KV-cache append in its epilogue: y = x[R, K] . W[N, K]^T, N = n_kv (g + 2) 128 in
 * groups of [g query heads | K | V].  Row r: query slots -> bf16(y) rotated (three bf16 roundings as aigv_op_rope, tables cos / sin
 * [max_pos, 64] at position pos[r]) into qkv[r * ldo + slot * 128 ..] (the K / V columns of qkv are not written); the K slot,
 * rotated, and the V slot, unrotated, into kc / vc [seq][n_kv][cap][128] at [seq[r]][kvh][pos[r]].  norm_w != NULL: x is the raw
 * residual stream and the kernel applies the RMSNorm (norm_w, eps) itself, with the bits of aigv_op_rmsnorm (R <= 4, K = 4096 or
 * 6144).  p = 1 / 2 / 4: 16 / 8 / 4 rows of W per workgroup (R <= 64 / 8 / 4); K % (128 p) == 0. */
int aigv_op_skinny_rope_kv(const void* x, int ldx, int R, const void* W, int ldw, int N, int K, void* qkv, int ldo, const int32_t* pos,
                           const int32_t* seq, const void* cos, const void* sin, void* kc, void* vc, int g, int n_kv, int cap,
                           const void* norm_w, float eps, int p, void* stream);
/* w1|w3 of a decode step with the RMSNorm in front: out[R, N / 2] = SwiGLU(RMSNorm(x) . W^T), W = w1 / w3 interleaved in 16-row blocks
 * (aigv_op_skinny_gemm epi 2); the bits of aigv_op_rmsnorm followed by aigv_op_skinny_gemm in form p.  R <= 4, K = 4096 or 6144. */
int aigv_op_skinny_swiglu_normed(const void* x, int ldx, int R, const void* W, int ldw, int N, int K, void* out, int ldo,
                                 const void* norm_w, float eps, int p, void* stream);
/* The e4m3 form of aigv_op_skinny_rope_kv (fp8 mode; aigv_op_skinny_gemm_fp8's arithmetic, its epi 7): W_e4m3 [N, ldw bytes] with one
 * fp32 scale per output channel, x RMS-normalised (norm_w required) and quantised per row inside the kernel.  R <= 4 and <= 16 / p,
 * K = 4096 or 6144. */
int aigv_op_skinny_rope_kv_fp8(const void* x, int ldx, int R, const void* W_e4m3, int ldw, const float* w_scale, int N, int K, void* qkv,
                               int ldo, const int32_t* pos, const int32_t* seq, const void* cos, const void* sin, void* kc, void* vc, int g,
                               int n_kv, int cap, const void* norm_w, float eps, int p, void* stream);

/* ---- the score head and the row kernels of the passes, one by one (test entry points) ----
 * Every argument is checked on the host before anything is launched (AIGV_ERR_ARG with a message that starts with the op's name).
 *
 * The score head of one batch slice: x [B, dims[0]] bf16 rows (leading dimension ldx) -> score[B] fp32 (the bf16 result widened).  If ANY
 * element of x is NaN, the whole slice is passed through nan_to_num(nan = 0, posinf = 1e9, neginf = -1e9) first; then n_layers of
 * ReLU(bf16(x W^T + b)), W [dims[i + 1], dims[i]] bf16, a NaN staying a NaN through the ReLU.  dims: HOST int32[n_layers + 1]; w / b: HOST
 * arrays of n_layers DEVICE pointers.  1 <= B <= 64, 1 <= n_layers <= 8, scratch >= 3 B max(dims) bf16.  Layers with a fan-in % 128 == 0
 * and a fan-out % 4 == 0 run as GEMMs; from the first other layer on, the chain runs in one tail kernel whose dims must all be <= 1024,
 * and the last layer must be a tail layer (as every fan-out of 1 is). */
int aigv_op_score_head(const void* x, int ldx, int B, int n_layers, const int32_t* dims_host, const void* const* w_dev, const void* const* b_dev,
                       void* scratch, int64_t scratch_bytes, float* score, void* stream);
/* aigv_op_score_head on G batch slices in one go: slice g = the B rows at x + g * group_stride elements (leading dimension ldx), guarded on its
 * own; score [G * B].  Slice for slice the bits of aigv_op_score_head on that slice alone (the GEMM layers run over all G * B rows in chunks of
 * at most 64, the tail kernel over all of them).  1 <= G, G * B <= 4096, group_stride >= 0; scratch >= 3 G B max(dims) bf16; B, the dims and
 * the split into GEMM and tail layers under aigv_op_score_head's rules. */
int aigv_op_score_head_groups(const void* x, int ldx, int G, int64_t group_stride, int B, int n_layers, const int32_t* dims_host,
                              const void* const* w_dev, const void* const* b_dev, void* scratch, int64_t scratch_bytes, float* score, void* stream);
/* The depth lens' tap: raw[i, :H] = src[idx[i] * ld ..] (aigv_op_gather_rows' bits) and normed[i, :H] = its RMSNorm under w (aigv_op_rmsnorm's
 * bits on the gathered rows), i < n, both dense; one launch.  H a multiple of 8 in 8..16384, ld a multiple of 8 and >= H, idx DEVICE int32 [n]. */
int aigv_op_lens_tap(const void* src, int ld, const int32_t* idx, int n, const void* w, void* raw, void* normed, int H, float eps, void* stream);
/* RMSNorm fused with the e4m3 row quantisation of its result: the bytes q [rows, ldq] and scales row_scale[rows] of aigv_op_rmsnorm followed by
 * aigv_op_quant_fp8_rows.  H a multiple of 8 in 8..16384; ldx, ldq multiples of 8 and >= H. */
int aigv_op_rmsnorm_quant_fp8(const void* x, int ldx, const void* w, void* q_e4m3, int ldq, float* row_scale, int rows, int H, float eps, void* stream);
/* aigv_op_rope on slots [first_rot, first_rot + n_rot) of every group (K only: first_rot = g, n_rot = 1); nothing else is written.
 * pos[t] must lie inside the tables. */
int aigv_op_rope_slots(void* qkv, int ld, const int32_t* pos, const void* cos, const void* sin, int tokens, int first_rot, int n_rot, int slots,
                       int n_groups, int head_dim, void* stream);
/* out[t, :H] = slot[t] < 0 ? emb[ids[t]] : slot[t] < n_vis ? vis[slot[t]] : motion[slot[t] - n_vis]  (ids DEVICE int64[tokens], slot DEVICE
 * int32[tokens]; vis / motion may be NULL when no slot selects them; the caller's promise: every index inside its table). */
int aigv_op_embed(const int64_t* ids, const int32_t* slot, const void* emb, const void* vis, const void* motion, int n_vis, void* out, int tokens, int H,
                  void* stream);
/* pos[t] = t - cu[s] + pos_offset[s], seq[t] = s for cu[s] <= t < cu[s + 1], and cu_dev[0..n_seq] = cu: cu_host / pos_offset_host (or NULL: 0) are
 * HOST int32 arrays, the outputs DEVICE int32.  1 <= n_seq <= 127, cu[0] = 0, cu[n_seq] = tokens. */
int aigv_op_seqpos(const int32_t* cu_host, int n_seq, const int32_t* pos_offset_host, int32_t* pos, int32_t* seq, int32_t* cu_dev, int tokens, void* stream);
/* The row movers (H and ld multiples of 8; idx DEVICE int32[n], every index inside its buffer):
 *   gather:  dst[i, :H] = src[idx[i] * ld ..]   (dst dense)      scatter: dst[idx[i] * ld ..] = src[i, :H]  (src dense; equal indices carry equal rows)
 *   cls:     x[f * tokens_per_frame, :H] = cls_pos[:H], f < n_frames (x dense)
 *   write_ints: dst[0..n) = host[0..n) (HOST int32 -> DEVICE int32, as kernel arguments) */
int aigv_op_gather_rows(const void* src, int ld, const int32_t* idx, int n, void* dst, int H, void* stream);
int aigv_op_scatter_rows(const void* src, const int32_t* idx, int n, void* dst, int ld, int H, void* stream);
int aigv_op_cls_rows(const void* cls_pos, void* x, int n_frames, int tokens_per_frame, int H, void* stream);
int aigv_op_write_ints(const int32_t* host, int n, int32_t* dst, void* stream);
/* One launch of the activation-patching row copy, as a pass of T rows makes it for slice `depth` of a window of n_depths depths: rows_host (HOST
 * int32 [n], checked as the pass checks them: inside [0, T), strictly ascending) are written to idx_dev (DEVICE int32 [n]); then, for i < n,
 *   to_stream = 0 (capture): side[(i * n_depths + depth) * H ..] = stream_rows[rows[i] * ld ..]      to_stream = 1 (patch): the other way round
 * - a bit copy of H bf16.  H a multiple of 8 in 8..16384, ld a multiple of 8 and >= H, both buffers 16-byte aligned, 0 <= depth < n_depths. */
int aigv_op_stream_rows(void* stream_rows, int ld, int T, const int32_t* rows_host, int n, int32_t* idx_dev, void* side, int n_depths, int depth, int H,
                        int to_stream, void* stream);
/* One launch of the head-rows kernel, as a pass of T rows makes it for slice `layer` of a window of n_layers layers, on ao [T][ld] with H = n_heads * D
 * (n_heads in 1..64, D 64 or 128); rows_host as for aigv_op_stream_rows.  Only heads whose bit of head_bits is set are read or written.
 *   mode 0 (capture): side[(i * n_layers + layer) * H ..] = ao[rows[i] * ld ..]      mode 1 (patch): the other way round      - bit copies
 *   mode 2 (scale): ao[rows[i]] = bf16(fp32(ao[rows[i]]) * scale_host[h]) for the set heads whose factor is not exactly 1 (HOST float [n_heads], no
 *   NaN); side, n_layers and layer are unused; rows_host NULL: rows 0 .. T - 1 (idx_dev unused). */
int aigv_op_head_rows(void* ao, int ld, int T, const int32_t* rows_host, int n, int32_t* idx_dev, void* side, int n_layers, int layer, int n_heads, int D,
                      int mode, uint64_t head_bits, const float* scale_host, void* stream);

/* One launch of the neuron-rows kernel, as a pass of T rows makes it for slice `layer` of a window of n_layers layers, on act [T][ld] of I columns (a
 * multiple of 8); rows_host as for aigv_op_stream_rows, NULL: rows 0 .. T - 1.  sidx_host (HOST int32 [n], each inside [0, n_side); NULL: i) names the
 * side row of entry i; cols_host (HOST int32 [m], strictly ascending inside [0, I); NULL: the dense form, W = I) the columns - element j of a side row
 * of W = m is column cols_host[j].  The host lists go to idx_dev / sidx_dev / cols_dev / factors_dev (DEVICE, n / n / m / m entries) as kernel arguments.
 *   mode 0 (capture): side[(si * n_layers + layer) * W ..] = the selected columns of act[rows[i]]      mode 1 (patch): the other way round  - bit copies
 *   mode 2 (scale): act = bf16(fp32(act) * s), s = dense_factor (dense) or factors_host[j] (sparse; HOST float [m], no NaN); a factor of exactly 1
 *   leaves its elements untouched (dense: nothing is launched); side, the side rows, n_layers and layer are unused. */
int aigv_op_neuron_rows(void* act, int ld, int T, const int32_t* rows_host, int n, int32_t* idx_dev, const int32_t* sidx_host, int32_t* sidx_dev, int n_side,
                        void* side, int n_layers, int layer, int I, const int32_t* cols_host, int m, int32_t* cols_dev, int mode, const float* factors_host,
                        float* factors_dev, float dense_factor, void* stream);

/* Frame ingest: uint8 [F,H,W,3] RGB frames already at the model resolution -> bf16 NCHW
 * pixel_values = bf16((u/255 - mean[c]) / std[c])  (torchvision ToTensor + Normalize of dataset.py:267-274 and the
 * bf16 cast of stage2_eval.py:932).  mean/std: HOST float[3].  height * width must be a multiple of 4, the frames 4-byte and out_nchw
 * 8-byte aligned; checked on the host. */
int aigv_op_frame_ingest(const void* hwc_u8, int n_frames, int height, int width, const float* mean, const float* stdv,
                         void* out_nchw, void* stream);

/* Frame resize + ingest: uint8 [F,in_h,in_w,3] RGB frames at the video's resolution -> Pillow's BICUBIC
 * `Image.resize((out_w, out_h))` (the reference's dynamic_preprocess tile, internvl/train/dataset.py:702-738 with max_num = 1;
 * stage2_eval.py:453-456), bit-exact with Pillow's 8-bit ImagingResample (22-bit fixed-point coefficients, horizontal pass
 * stored as uint8, then the vertical pass) -> uint8 [F,out_h,out_w,3] in out_u8_hwc (may be NULL) and / or the normalised bf16
 * NCHW pixel_values of aigv_op_frame_ingest in out_nchw (may be NULL).  tmp_u8: DEVICE scratch of F*in_h*out_w*3 bytes.
 * Coefficient tables are computed on the host (double precision, as Pillow does) and cached on the device per size pair; the
 * first call for a size pair synchronises on their upload.  mean/std: HOST float[3].
 * Checked against the live package on random sizes from 8 x 8 to 1200 x 2000 (tests/manual/fuzz_resize.py, Pillow 12.2).  One regime is REFUSED
 * (AIGV_ERR_ARG): frames more than 100 times taller than wide that shrink vertically - there Pillow runs its vertical pass first and the
 * uint8 intermediate makes the order visible; not a video geometry. */
int aigv_op_frame_resize_ingest(const void* hwc_u8, int n_frames, int in_h, int in_w, int out_h, int out_w, const float* mean,
                                const float* stdv, void* tmp_u8, void* out_u8_hwc, void* out_nchw, void* stream);

/* ---- tuning knobs: TESTS AND EXPERIMENTS ONLY ---------------------------------------------------------------------------------------
 * Every knob lives in the CONTEXT (aigv_ctx_tune; value -1 = follow the process default): two contexts of one process can run different
 * kernel forms side by side, and the kernel files hold no mutable state - each launch carries its selectors.  aigv_tune_gemm /
 * aigv_tune_attention / aigv_tune_skinny set the PROCESS defaults, which apply to the context-free aigv_op_* entry points and to
 * contexts that left a knob at -1 (not thread-safe: in-process A/B scripts and tests that must force a kernel form).  A deployment calls
 * none of them: what a context needs per instance is aigv_set_gemm_mode / aigv_set_precision / aigv_set_row_trimming /
 * aigv_set_attention_numerics above. */
enum aigv_tune_knob {
  AIGV_TUNE_GEMM_MODE = 0,       /* = aigv_set_gemm_mode */
  AIGV_TUNE_GEMM256_ORDER = 1,   /* tile order of the 256 kernel: 0 by weight size, 1 row groups, 1 + g groups of g column tiles */
  AIGV_TUNE_GEMM256_VARIANT = 2, /* 0 the shipped schedule, 1 + v schedule variant v (0..3); 5..7: the 256x256 kernel runs its shipped schedule, the co-resident kernel a diagnostic form (AIGV_CO_DIAG builds only) */
  AIGV_TUNE_ATTN_WAVES = 3,      /* prefill attention: 0 default, 4 / 8 waves per workgroup */
  AIGV_TUNE_SKINNY_P = 4,        /* decode GEMV form: 0 per-shape default, 1 / 2 / 4; 1000 + (wqkv | wo << 3 | w1w3 << 6 | w2 << 9) = one form per GEMV */
  AIGV_TUNE_BODY_TILE = 5,       /* tile kernel of a row plan's body rows: 0 / 1 = 256x256 (shipped), 2 = 128x128 (same bits, slower) */
  AIGV_TUNE_CO_KMAX = 6,         /* GEMMs with K <= value run on the co-resident 256x128 kernel (same bits as the 256x256 one): 0 never (default) */
  AIGV_TUNE_TAIL_SLICES = 7,     /* split-K factor of the row plans' tail half tiles: 0 = the per-(N, K) rule, 1 = inside the body's launch, S = one factor wherever it divides */
  AIGV_TUNE_ATTN_LEAD_KEY = 8,   /* InternViT attention (64 j + 1 keys): 1 = full tiles over keys 1.. + key 0 merged in the epilogue (another summation order) */
  AIGV_TUNE_DECODE_FUSED = 9,    /* decode: 1 (default) = RMSNorm inside the GEMV that consumes it, 0 = separate norm kernels */
  AIGV_TUNE_DECODE_FP8 = 10,     /* decode in fp8 mode: 1 (default) = e4m3 GEMVs, 0 = bf16 GEMVs */
  AIGV_TUNE_SKINNY_P8 = 11,      /* form of the e4m3 decode GEMVs: 0 per-GEMV defaults, 1 / 2 / 4 */
  AIGV_TUNE_FUSE_TAILS = 12,     /* the tail tiles' K slices inside the body's launch: 0 = when the body leaves CUs idle (default), 1 = never, 2 = always; same bits */
  AIGV_TUNE_LONE_BODY = 13,      /* row-plan bodies of <= 128 tiles on the 256x128 kernel's one-workgroup-per-CU form: 0 = by fill, 1 = never (default), 2 = always, 3 / 4 = by fill for GEMMs with / without split-K tails; same bits */
  AIGV_TUNE_COUNT = 14           /* number of knobs, not a knob */
};
int aigv_ctx_tune(aigv_ctx* ctx, int knob, int value);
/* GEMM tile-kernel selection: mode 0 = cost model (default), 1 = always the 128x128 kernel, 2 = always the 256x256
 * phase-interleaved kernel where N % 256 == 0, 4 = always the co-resident 256x128 kernel; rate256 > 0 overrides the model's relative throughput of the 256 kernel. */
/* mode bits 4..6: 1 + v selects schedule variant v of the 256 kernel (0 = keep); bits 10..13: tile order of the 256 kernel, 0 = by weight
 * size (default), 1 = row groups, 1 + g = groups of g column tiles; bits 14..15: tile kernel of a row plan's body (AIGV_TUNE_BODY_TILE). */
int aigv_tune_gemm(int mode, double rate256);
/* Process default of AIGV_TUNE_CO_KMAX: 0 = the co-resident 256x128 kernel is never chosen by the dispatcher, else the largest K it takes. */
int aigv_tune_co_gemm(int kmax);
/* Process default of AIGV_TUNE_TAIL_SLICES / _FUSE_TAILS / _LONE_BODY / _ATTN_LEAD_KEY / _CO_KMAX (same value ranges as aigv_ctx_tune, without the -1). */
int aigv_tune_default(int knob, int value);
/* The row bands run_gemm would cut an M x N x K problem into (host logic only, no GPU): plan[0] = row tiles (x256 rows) on the
 * 256x256 kernel in whole rounds, or -1 = the whole problem in one launch of that kernel; plan[1] = row tiles on the 256x256
 * kernel with split-K, plan[2] = their K slices; plan[3] = remaining rows, plan[4] = their kernel (0 none, 1 skinny
 * weight-streaming, 2 the 128x128 kernel), plan[5] = split-K slices on the 128x128 kernel (1 = none); plan[6] = width of a right-hand
 * column band that runs on the 128x128 kernel over all rows (N = 256 j + 128: plan[0..5] then describe the first 256 j columns;
 * 0 = no column split); `plan` holds 7 ints; est_us = the model's time. */
int aigv_plan_gemm(int M, int N, int K, int epi, int* plan, double* est_us);
/* The launches the GEMM dispatcher (aigv_op_gemm, aigv_op_gemm_rows and every pass) has made in this process since the record was last
 * cleared: the OR of one AIGV_ROUTE_* bit per kind of launch, set where the launch is issued.  clear != 0 returns the record and empties
 * it.  Host only; for tests that force a route and must prove that it ran (ABI 3, added symbol). */
enum {
  AIGV_ROUTE_128 = 1,              /* every row of the (sliced) problem on the 128x128 kernel */
  AIGV_ROUTE_256 = 2,              /* ... on the 256x256 kernel */
  AIGV_ROUTE_CO = 4,               /* ... on the co-resident 256x128 kernel */
  AIGV_ROUTE_SPLITK_128 = 8,       /* a row band as K slices of the 128x128 kernel + finalize */
  AIGV_ROUTE_SPLITK_256 = 16,      /* a row band as K slices of the 256x256 kernel + finalize */
  AIGV_ROUTE_SKINNY = 32,          /* the last rows of run_gemm on the weight-streaming kernel */
  AIGV_ROUTE_COLUMN_BAND = 64,     /* N = 256 j + 128 cut into a left part and a right-hand 128-column band */
  AIGV_ROUTE_TAB_256 = 128,        /* half tiles of a row plan on the 256x256 kernel, full K */
  AIGV_ROUTE_TAB_SPLITK = 256,     /* tail half tiles of a row plan as K slices in a launch of their own + finalize */
  AIGV_ROUTE_TAB_FUSED = 512,      /* body tiles and the tails' K slices in one launch, then finalize */
  AIGV_ROUTE_TAB_LONE = 1024,      /* half tiles on the co-resident kernel's one-workgroup-per-CU form */
  AIGV_ROUTE_TAB_128 = 2048,       /* body half tiles on the 128x128 kernel */
  AIGV_ROUTE_TAB_CO = 4096,        /* body and tail half tiles on the co-resident kernel (K <= AIGV_TUNE_CO_KMAX) */
  AIGV_ROUTE_TINY = 8192,          /* tiny sequence tails on the weight-streaming kernel, one launch per sequence */
  AIGV_ROUTE_TINY_STRIDED = 16384  /* uniform tiny tails: one launch per tail row over all sequences, row stride = sequence length */
};
int aigv_gemm_route(int clear);
/* Prefill-attention kernel form (process-wide; experiments and tests): 0 = default (attention.hip: 4 waves x 32 query rows per
 * workgroup, two-deep K/V ring); 4 or 8 = that many waves per workgroup (three-deep rings lost the in-step A/B and were removed:
 * profiles/r3_attn_ring_negative.txt). */
int aigv_tune_attention(int waves);
/* Form of the decode GEMVs (process-wide; experiments and tests): 0 = default (per-shape choice in aigv_decode_step, 16-row slabs
 * in aigv_op_skinny_gemm); 1 / 2 / 4 = 16 / 8 / 4 rows of W per workgroup and slab wherever legal (R <= 16 / p, epi store /
 * residual / swiglu).  Results agree up to fp32 summation order. */
int aigv_tune_skinny(int p);

/* ---- measurement ------------------------------------------------------------------------------------ */
/* When enabled every GEMM / attention launch of the hot path is bracketed by HIP events on the launch stream. */
/* AIGV_PROF_GEMM = the bf16 tile-kernel GEMMs of the InternLM2 pass, AIGV_PROF_GEMM_VIT = those of InternViT and the mlp1 projector
 * (aigv_vit_forward / aigv_project) - two classes because the short-K InternViT shapes run at a different fraction of the MFMA peak. */
enum aigv_prof_class { AIGV_PROF_GEMM = 0, AIGV_PROF_ATTN_VIT = 1, AIGV_PROF_ATTN_LLM = 2, AIGV_PROF_SKINNY = 3,
                       AIGV_PROF_GEMM_FP8 = 4, AIGV_PROF_GEMM_VIT = 5, AIGV_PROF_COUNT = 6 };
int aigv_prof_enable(aigv_ctx* ctx, int on);
/* Synchronises the recorded events and returns (and clears) launches, total milliseconds and algorithmic
 * FLOPs (2*M*N*K; attention 4*sum(len_q*len_kv_visible)*d*heads) and bytes per class. */
int aigv_prof_read(aigv_ctx* ctx, int cls, int64_t* launches, double* total_ms, double* flops, double* bytes);

/* ---- SlowFast-R50 motion branch ---------------------------------------------------------------------
 * Replaces the reference's ``slowfast`` module + pack_pathway_output (internvl/model/internvl_chat_eval2/modeling_internvl_chat.py:97-193):
 * frames -> [clips, 2304] motion feature, the input of motion_mlp (aigv_motion_project).  Its own handle: the branch shares nothing
 * with the scorer context but the frames tensor.  Weights arrive by their state-dict names under
 * ``slowfast_model.feature_extraction.`` (that prefix, ``feature_extraction.`` or pytorchvideo's ``blocks.`` are all accepted):
 * conv ``.weight`` [Cout, Cin, kt, kh, kw] and BatchNorm ``.weight/.bias/.running_mean/.running_var``; finalize folds the eval-mode
 * norms into the convs, packs for the kernel, uploads, and reports missing / mis-shaped tensors by name.
 *   frames: DEVICE bf16 [clips * T, 3, H, W] NCHW, clip-major (the pixel_values tensor of the scorer); feature: DEVICE bf16 [clips, 2304].
 *   T a multiple of 4 in [8, 32] (slow pathway = frames linspace(0, T-1, T/4).long()); H, W multiples of 32 in [224, 1024].
 * Parity with pytorchvideo itself cannot be pinned offline (oracle/slowfast.py restates the published architecture). */
typedef struct aigv_slowfast aigv_slowfast;
int aigv_slowfast_create(int device, int max_clips, int frames_per_clip, int height, int width, aigv_slowfast** out);
void aigv_slowfast_destroy(aigv_slowfast* sf);
int aigv_slowfast_load_weight(aigv_slowfast* sf, const char* name, const void* host_data, const int64_t* shape, int ndim, int dtype);
int aigv_slowfast_finalize(aigv_slowfast* sf);
int aigv_slowfast_forward(aigv_slowfast* sf, const void* frames_nchw_bf16, int clips, void* feature_bf16, void* stream);
double aigv_slowfast_flops_per_clip(const aigv_slowfast* sf);
/* one convolution with the branch's implicit-GEMM kernel (tests / profiling): x channels-last bf16 [B, Ti, Hi, Wi, ld_in];
 * w_packed bf16 [ceil16(Cout), Kp], k = ((dt * kh + dy) * kw + dx) * Cin + ci zero padded to Kp (multiple of 64); bias fp32 [Cout];
 * dims = {Ti, Hi, Wi, kt, kh, kw, st, sh, sw, pt, ph, pw}; out[row, c_off + c] = relu?(conv + bias + res[row, c]) */
int aigv_op_conv3d(const void* x, int ld_in, int Cin, int B, const int* dims, const void* w_packed, int Kp, const float* bias, int Cout,
                   const void* res, int ld_res, void* out, int ld_out, int c_off, int relu, void* stream);

/* ---- the branch's plan, one op at a time (tests / profiling, like aigv_op_conv3d; not part of the scoring path) ---------------------
 * A finalized handle holds a PLAN: the list of launches aigv_slowfast_forward makes, in order (one repack, ~105 convolutions, two
 * max-pools, two head pools).  These entries describe the ops, run a range of them through the code the forward runs, and copy the
 * activation buffers they work on, so that a test can hold each op alone against a reference computed from the input it really had.
 *
 * Activation buffers are numbered 0 .. AIGV_SF_BUFFERS-1 and reused along the plan; an op reads / writes the FRONT of a buffer as
 * [clips][per-clip elements] bf16, channels-last with a row stride (ld).  The per-clip counts below are those of the op's own view. */
#define AIGV_SF_BUFFERS 14
enum aigv_slowfast_op_kind { AIGV_SF_REPACK = 0, AIGV_SF_CONV = 1, AIGV_SF_MAXPOOL = 2, AIGV_SF_HEADPOOL = 3 };
typedef struct aigv_slowfast_op {
  int32_t kind;                          /* aigv_slowfast_op_kind */
  int32_t in_buf, res_buf, out_buf;      /* buffer ids, -1 = none.  Repack: in = the caller's frames (-1), out = the fast stem's input
                                            [T, H, W, 4]; head pool: out = the caller's feature (-1) */
  int32_t out2_buf;                      /* repack only: the slow stem's input [To, H, W, 4]; -1 otherwise */
  int32_t pair_stem;                     /* conv: 1 = a stem, run as a 4-tap conv over PAIRS of 4-channel pixels (3 real channels + a zero
                                            one): the geometry below is the pair form - Wi = W / 2, Cin = 8, kw = 4, sw = 1, pw = 2 - of the
                                            state dict's [Cout, 3, kt, 7, 7] kernel with stride (1, 2, 2) and pad (kt / 2, 3, 3) */
  int64_t in_elems, res_elems, out_elems, out2_elems;   /* per clip; 0 where the id is -1 */
  /* convolution (also max-pool: Hi, Wi, Ho, Wo, ld_out) */
  int32_t ld_in, Cin, Ti, Hi, Wi;
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
  int32_t To, Ho, Wo, Cout, Kp;          /* repack: To = the number of slow frames */
  int32_t ld_res, ld_out, c_off, relu;   /* out[row, c_off + c], c < Cout (head pool: c < C, ld_out = 2304) */
  int32_t k_slices;                      /* planned split-K slices (per-clip shape); > 1: slabs + the finalize kernel */
  /* pools and repack: the op's input map, T frames of H x W with C channels (repack: the frames, C = 4 channels written) */
  int32_t T, H, W, C;
  int32_t window;                        /* head pool: temporal window over the 4x repeated frames (8 slow, 32 fast) */
  int32_t reserved;
  char conv_name[128], norm_name[128];   /* conv: state-dict names under feature_extraction. ("" otherwise) */
} aigv_slowfast_op;
/* number of ops of a finalized handle's plan (negative aigv_status otherwise) */
int aigv_slowfast_plan_size(const aigv_slowfast* sf);
/* describes op `index`; sizeof_op = sizeof(aigv_slowfast_op) of the caller (a mismatch is refused) */
int aigv_slowfast_plan_op(const aigv_slowfast* sf, int index, aigv_slowfast_op* op, int sizeof_op);
/* runs ops first .. last (inclusive) for `clips` clips on `stream`.  frames is read by the repack only, feature written by the head pools
 * only: either may be NULL when the range holds no such op.  aigv_slowfast_forward is this call over the whole plan.  A convolution
 * whose planned k_slices cannot run (workspace too small) is an error, never a silent unsplit launch. */
int aigv_slowfast_run_ops(aigv_slowfast* sf, const void* frames_nchw_bf16, int clips, void* feature_bf16, int first, int last, void* stream);
/* device-to-device copies of the first clips * elems_per_clip bf16 elements of activation buffer `buf`, on `stream` */
int aigv_slowfast_buffer_read(aigv_slowfast* sf, int buf, int64_t elems_per_clip, int clips, void* dst_bf16, void* stream);
int aigv_slowfast_buffer_write(aigv_slowfast* sf, int buf, int64_t elems_per_clip, int clips, const void* src_bf16, void* stream);
/* The host arithmetic of create / finalize, callable without a device (HOST pointers).
 * slow-pathway frame indices, torch.linspace(0, T - 1, T / 4).long(): writes T / 4 ints (T a multiple of 4 in [4, 256]), returns the count */
int aigv_slowfast_slow_indices(int frames_per_clip, int32_t* idx);
/* head pool = repeat_interleave(4) + AvgPool3d((window, 7, 7), stride 1) + AdaptiveAvgPool3d(1) as ONE weighted mean with separable
 * weights: wt[frames], wy[H], wx[W] (1 <= frames <= 32 with 4 * frames >= window, 7 <= H, W <= 32) */
int aigv_slowfast_pool_weights(int frames, int H, int W, int window, float* wt, float* wy, float* wx);
/* split-K slices the plan gives a convolution of `rows` output positions PER CLIP, ceil16(Cout) = CoutPad, padded K = Kp */
int aigv_slowfast_conv_k_slices(int64_t rows, int CoutPad, int Kp);

#ifdef __cplusplus
}
#endif
#endif /* AIGV_AMD_H */
