// Score-row attention probe: where ONE query row of a causal GQA attention looks, folded into a few key segments (frames, motion token,
// text).  The flash prefill kernel (attention.hip) never forms a probability matrix; this stand-alone kernel recomputes the softmax of the
// few rows somebody asks about from the Q (unrotated) and K (rotated) that llm_layer_qkv leaves in the fused qkv rows - or, for a
// continuation, from the KV cache - and touches nothing the pass itself reads afterwards.
//
// One 256-thread workgroup per (probe row, query head).  For the row at position p = key offset + local row of its sequence:
//   1. q is rotated at p with rope_pair (common.h: rope_kernel's arithmetic, so the rotated q carries the bits aigv_op_rope would store);
//   2. s_j = (q . k_j) / sqrt(D) in fp32 for the keys j = 0..p of the SAME sequence (the causal rule: a later key, or another sequence's, is
//      never read); thread t takes keys t, t + 256, ... in ascending order.  Scores are always fp32 here, whatever the pass's attention
//      numerics (aigv_set_attention_numerics) say: the probe reports where the row looks, it does not feed the pass;
//   3. the row maximum m comes out of the log-probability kernels' one reduction tree (lse_of_block, common.h) - only m is used;
//   4. a second sweep adds e_j = exp(s_j - m) to the thread's own LDS column of bin seg[j] and of the total; an id outside [0, S) drops
//      the key from the bins, not from the total;
//   5. columns are summed lanes first (xor butterfly), then waves in wave order; out[seg] = bin[seg] / total, ONE fp32 division.
// The DENSE form (a template argument: the plain instantiation is the code above and nothing else) also reports every key on its own:
//   4'. in the second sweep thread t stores e_j of its keys t, t + 256, ... to tok[j] (coalesced 4-byte stores);
//   5'. once the total is known every thread reads back the elements IT wrote - no fence: a thread sees its own stores - and stores
//       tok[j] = e_j / total, the bins' total and the bins' division, so a bin of one key holds that key's dense bits; the columns behind
//       the row, pos < j < ld_tok, are set to +0.0.  All ld_tok columns are written, nothing outside them.
// The summation order is a function of the key index alone (no float atomics, nothing depends on the row count, the batch mates or the
// grid), so a row's bits are its own - and integer-valued e_j (Q = 0: every e_j is 1) give exact counts.
//
// The VALUES form (the third template argument of the ONE kernel: steps 1 - 3, step 4's statement for key j, the bins' reduction, `out` and the
// dense tail are the same source lines in every form; the plain and dense instantiations hold no barrier, LDS byte or loop of this form) also
// reports WHAT the row takes from every segment: val[row][head][s][c] = (sum over the keys j of segment s of e_j v_j[c]) / total for
// s = 0 .. S and c = 0 .. D - 1, slot S collecting the keys whose id lies outside [0, S) - so the S + 1 vectors sum to the head's output.  v_j
// is the bf16 V row the pass's attention reads (packed: the V columns of the fused rows; cache: the V cache, with K's strides), kv head h / g.
// The second sweep runs tile by tile, tile i = keys 256 i .. 256 i + 255, a trip count that is uniform over the workgroup:
//   4v. thread t computes e_j and the id of key j = 256 i + t exactly as step 4 does - the same thread, the same keys in the same order, so
//       `out` and `tok` carry the plain / dense form's bits - and leaves (e_j, id; an id outside [0, S) as S) in an LDS tile;
//   5v. behind a barrier the threads regroup as (key lane kl = t / D, column c = t % D), KL = 256 / D key lanes.  Lane kl walks the tile's keys
//       256 i + kl, 256 i + kl + KL, ... in ascending order and does acc[kl][id][c] = fmaf(e_j, float(v_j[c]), acc[kl][id][c]) - ONE fma per
//       key, from +0.0; the accumulator of the running id is kept in a register and exchanged with its LDS slot when the id changes (a cache:
//       the chain is the same).  Tile after tile, so acc[kl][s][c] is the fma chain over the keys j = kl (mod KL) of segment s, ascending;
//   6v. val[s][c] = (((acc[0][s][c] + acc[1][s][c]) + ...) + acc[KL - 1][s][c]) / total: KL - 1 additions in lane order, ONE fp32 division by
//       the bins' own total (step 5's bits).  All (S + 1) D elements are written, nothing outside them.
// The rounding chain of one element, which tests/score_values_reference.py counts: expf's ulp on e_j and on every term of the total, the
// total's ceil(n / 256) + 9 additions, at most ceil(n / KL) fmas (the longest key lane), KL - 1 lane additions, one division.  The order is a
// function of the key index alone, as above.  0 x Inf is NaN here as in torch and in the flash kernel: a non-finite V row of a key whose
// weight underflowed to 0 makes its segment NaN; that is not special-cased.
#include "common.h"
#include "kernels.h"

namespace {

// (q . k) / post_div with the products accumulated in key-element order by explicit fmaf: both sweeps get the same bits
template <int D>
__device__ __forceinline__ float probe_score(const float* __restrict__ qs, const bf16_t* __restrict__ kp, float post_div) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < D / 8; ++c) {
    const u16x8 kv = *(const u16x8*)(kp + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(qs[8 * c + e], bf2f(kv[e]), acc);
  }
  return acc / post_div;
}

constexpr int AIGV_PROBE_VALUES_MAX_LDS = 160 * 1024 - 2048;   // a CDNA4 CU's LDS less the kernel's static arrays (qs, red, the tree's)

// the four wave partials of one column of `red`, added in wave order: the last step of every bin's sum and of the total's
__device__ __forceinline__ float waves_in_order(const float* r) { return ((r[0] + r[1]) + r[2]) + r[3]; }

// step 1: q of head h rotated at pos, as fp32, into qs[D] (the first D / 2 threads; the caller's barrier publishes it)
template <int D>
__device__ __forceinline__ void probe_rotate_q(const ProbeArgs& p, const ProbeRow& pr, int h, int pos, float* qs) {
  constexpr int half = D / 2;
  const int tid = threadIdx.x, g = p.n_heads / p.n_kv_heads;
  if (tid < half) {
    const bf16_t* q = p.q + (size_t)pr.row * p.ldq + (size_t)(h / g) * p.q_group_stride + (size_t)(h % g) * D;
    const size_t tb = (size_t)pos * half + tid;
    bf16_t lo, hi;
    rope_pair(q[tid], q[tid + half], p.rope_cos[tb], p.rope_sin[tb], lo, hi);
    qs[tid] = bf2f(lo);
    qs[tid + half] = bf2f(hi);
  }
}

// steps 2 and 3: the maximum of the row's scores, out of the log-probability kernels' tree
template <int D>
__device__ __forceinline__ float probe_row_max(const ProbeArgs& p, const float* qs, const bf16_t* kb, int n_keys) {
  float m = -INFINITY, sum = 0.0f;
  for (int j = threadIdx.x; j < n_keys; j += LSE_THREADS) lse_push(m, sum, probe_score<D>(qs, kb + (size_t)j * p.ldk, p.post_div));
  float row_max = 0.0f;
  lse_of_block<false>(m, sum, &row_max);
  return row_max;
}

// the segment id of key j: a cached key's from the sequence's row of seg_cached, a key of the pass from seg_new
__device__ __forceinline__ int probe_segment(const ProbeArgs& p, const ProbeRow& pr, int j) {
  return j < pr.off ? p.seg_cached[(size_t)pr.seq * p.ld_cached + j] : p.seg_new[pr.row0 + (j - pr.off)];
}

// step 5': the thread's own stores of the second sweep, divided; the stride goes on behind the row, so the 256 threads cover every column up to
// ld_tok
__device__ __forceinline__ void probe_dense_tail(float* tok, float total, int n_keys, int ld_tok) {
  int j = threadIdx.x;
  for (; j < n_keys; j += LSE_THREADS) tok[j] = tok[j] / total;
  for (; j < ld_tok; j += LSE_THREADS) tok[j] = 0.0f;
}

template <int D, bool DENSE, bool VALUES>
__global__ __launch_bounds__(LSE_THREADS) void attn_probe_kernel(const ProbeArgs p) {
  constexpr int KL = LSE_THREADS / D;                  // VALUES: key lanes
  extern __shared__ float bins[];                      // [n_seg + 1][256]: column = thread, row n_seg = the total
                                                       // VALUES: | [KL][n_seg + 1][D] accumulators | the tile: e [256], id [256]
  __shared__ float qs[D];
  __shared__ float red[(AIGV_MAX_ATTN_SEGMENTS + 1) * (LSE_THREADS / AIGV_WAVE)];
  const int tid = threadIdx.x, lane = tid % AIGV_WAVE, wave = tid / AIGV_WAVE;
  const ProbeRow pr = p.tab.r[blockIdx.x];
  const int h = blockIdx.y, hk = h / (p.n_heads / p.n_kv_heads);
  const int pos = pr.off + (pr.row - pr.row0), n_keys = pos + 1, S = p.n_seg;
  float* acc = bins + (S + 1) * LSE_THREADS;
  float* tile_e = acc + (S + 1) * LSE_THREADS;         // (KL * D = 256)
  int* tile_id = (int*)(tile_e + LSE_THREADS);

  probe_rotate_q<D>(p, pr, h, pos, qs);
  for (int s = 0; s <= S; ++s) {
    bins[s * LSE_THREADS + tid] = 0.0f;
    if constexpr (VALUES) acc[s * LSE_THREADS + tid] = 0.0f;   // (every slot once: [kl][s][c] is kl * (S + 1) * D + s * D + c < (S + 1) * 256)
  }
  __syncthreads();

  // packed: the sequence's rows of the pass (row0 + j);  cache: [seq][kv head][cap][D], position j
  const size_t kv_base = (p.kv_seq_stride ? (size_t)pr.seq * p.kv_seq_stride : (size_t)pr.row0 * p.ldk) + (size_t)hk * p.kv_head_stride;
  const bf16_t* kb = p.k + kv_base;
  const float row_max = probe_row_max<D>(p, qs, kb, n_keys);

  float* tok = nullptr;                                // DENSE: the ld_tok columns of this (row, head)
  if constexpr (DENSE) tok = p.tok + (size_t)blockIdx.x * p.tok_row_stride + (size_t)h * p.ld_tok;
  // step 4 for the thread's key j, the one statement of it: returns e_j, hands out the key's id
  auto weigh = [&](int j, int& sg) {
    const float e = expf(probe_score<D>(qs, kb + (size_t)j * p.ldk, p.post_div) - row_max);
    sg = probe_segment(p, pr, j);
    bins[S * LSE_THREADS + tid] += e;
    if (sg >= 0 && sg < S) bins[sg * LSE_THREADS + tid] += e;
    if constexpr (DENSE) tok[j] = e;
    return e;
  };
  if constexpr (!VALUES) {
    for (int j = tid; j < n_keys; j += LSE_THREADS) {
      int sg;
      weigh(j, sg);
    }
  } else {
    const bf16_t* vb = p.v + (p.kv_seq_stride ? kv_base : (size_t)pr.row0 * p.ldv + (size_t)hk * p.kv_head_stride);
    const int kl = tid / D, c = tid % D;
    float* my_acc = acc + (size_t)kl * (S + 1) * D + c;  // this thread's slots: my_acc[s * D]
    int run = S;                                       // the running id and its accumulator (the slot holds +0.0 until the first exchange)
    float run_acc = 0.0f;
    const int n_tiles = (n_keys + LSE_THREADS - 1) / LSE_THREADS;
    for (int i = 0; i < n_tiles; ++i) {
      const int j = i * LSE_THREADS + tid;
      if (j < n_keys) {
        int sg;
        tile_e[tid] = weigh(j, sg);
        tile_id[tid] = sg >= 0 && sg < S ? sg : S;
      }
      __syncthreads();
      const int in_tile = min(LSE_THREADS, n_keys - i * LSE_THREADS);
      const bf16_t* vt = vb + (size_t)i * LSE_THREADS * p.ldv + c;
      constexpr int UN = 8;                            // V elements in flight per thread: the loads do not depend on the fma chain
      int jj = kl;
      for (; jj + (UN - 1) * KL < in_tile; jj += UN * KL) {
        float v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) v[u] = bf2f(vt[(size_t)(jj + u * KL) * p.ldv]);
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int id = tile_id[jj + u * KL];
          if (id != run) {
            my_acc[run * D] = run_acc;
            run_acc = my_acc[id * D];
            run = id;
          }
          run_acc = fmaf(tile_e[jj + u * KL], v[u], run_acc);
        }
      }
      for (; jj < in_tile; jj += KL) {
        const int id = tile_id[jj];
        if (id != run) {
          my_acc[run * D] = run_acc;
          run_acc = my_acc[id * D];
          run = id;
        }
        run_acc = fmaf(tile_e[jj], bf2f(vt[(size_t)jj * p.ldv]), run_acc);
      }
      __syncthreads();                                 // the tile is rewritten by the next trip
    }
    my_acc[run * D] = run_acc;
  }
  // step 5.  Every thread has written its own column of `bins` only: no barrier in front of the butterflies.  (The reduction and the `out` store
  // stand here and not in functions: handed `red` as a pointer argument, hipcc schedules the plain instantiations differently from the code they
  // were - profiles/readout_kernels_refactor.txt.)
  for (int s = 0; s <= S; ++s) {
    const float v = wave_sum(bins[s * LSE_THREADS + tid]);
    if (lane == 0) red[s * (LSE_THREADS / AIGV_WAVE) + wave] = v;
  }
  __syncthreads();                                     // (VALUES also: every accumulator slot is in LDS)
  if (tid < S) {
    const float total = waves_in_order(red + S * (LSE_THREADS / AIGV_WAVE));
    const float bin = waves_in_order(red + tid * (LSE_THREADS / AIGV_WAVE));
    p.out[(size_t)blockIdx.x * p.out_row_stride + (size_t)h * S + tid] = bin / total;
  }
  // the bins' total, from the bins' statement of it: every form divides by these bits
  if constexpr (DENSE) probe_dense_tail(tok, waves_in_order(red + S * (LSE_THREADS / AIGV_WAVE)), n_keys, p.ld_tok);
  if constexpr (VALUES) {
    const float total = waves_in_order(red + S * (LSE_THREADS / AIGV_WAVE));
    float* val = p.val + (size_t)blockIdx.x * p.val_row_stride + (size_t)h * (S + 1) * D;
    for (int x = tid; x < (S + 1) * D; x += LSE_THREADS) {   // x = s * D + c: coalesced
      float a = acc[x];
#pragma unroll
      for (int l = 1; l < KL; ++l) a += acc[(size_t)l * (S + 1) * D + x];
      val[x] = a / total;
    }
  }
}

// the dynamic LDS in bytes: the bins; VALUES: bins + accumulators + tile
constexpr int probe_lds(bool values, int n_seg) { return (values ? 2 * (n_seg + 1) + 2 : n_seg + 1) * LSE_THREADS * (int)sizeof(float); }

template <int D, bool DENSE, bool VALUES>
hipError_t launch_probe(const ProbeArgs& a, hipStream_t s) {
  static LdsAttrOnce lds_attr;
  if (hipError_t e = lds_attr.ensure((const void*)attn_probe_kernel<D, DENSE, VALUES>, probe_lds(VALUES, AIGV_MAX_ATTN_SEGMENTS)); e != hipSuccess) return e;
  hipLaunchKernelGGL((attn_probe_kernel<D, DENSE, VALUES>), dim3(a.n_rows, a.n_heads), dim3(LSE_THREADS), probe_lds(VALUES, a.n_seg), s, a);
  return hipGetLastError();
}

template <int D>
hipError_t launch_probe_form(const ProbeArgs& a, hipStream_t s) {
  if (a.val) return a.tok ? launch_probe<D, true, true>(a, s) : launch_probe<D, false, true>(a, s);
  return a.tok ? launch_probe<D, true, false>(a, s) : launch_probe<D, false, false>(a, s);
}

}  // namespace

// Every index the kernel forms is bounded here, on the host, from the host copies of the sequence table: nothing is launched otherwise.
const char* aigv_probe_check(const ProbeArgs& a, int head_dim, int total_rows, int max_pos) {
  if (head_dim != 64 && head_dim != 128) return "attention probe: head_dim must be 64 or 128";
  if (!a.q || !a.k || !a.rope_cos || !a.rope_sin || !a.seg_new || !a.out) return "attention probe: null operand";
  if (a.n_rows < 1 || a.n_rows > AIGV_MAX_PROBE_ROWS) return "attention probe: the number of probe rows is outside 1..AIGV_MAX_PROBE_ROWS (64)";
  if (a.n_seg < 1 || a.n_seg > AIGV_MAX_ATTN_SEGMENTS) return "attention probe: the number of segments is outside 1..AIGV_MAX_ATTN_SEGMENTS (64)";
  if (a.n_kv_heads < 1 || a.n_heads < a.n_kv_heads || a.n_heads % a.n_kv_heads || a.n_heads > 65535) return "attention probe: n_heads must be a multiple of n_kv_heads";
  const int g = a.n_heads / a.n_kv_heads;
  if (a.q_group_stride < g * head_dim || (int64_t)a.ldq < (int64_t)(a.n_kv_heads - 1) * a.q_group_stride + g * head_dim) return "attention probe: q strides too small";
  if (a.ldk % 8 || a.kv_head_stride % 8 || a.kv_seq_stride % 8 || ((uintptr_t)a.k & 15)) return "attention probe: K must be 16-byte aligned with strides that are multiples of 8";
  if (!(a.post_div > 0.0f)) return "attention probe: post_div must be positive";
  if (a.out_row_stride < (size_t)a.n_heads * a.n_seg) return "attention probe: out row stride below n_heads * n_segments";
  // dense form (one value per key): asked for by either argument, so that a half-given pair is refused and not read as the plain form
  const bool dense = a.tok || a.ld_tok != 0;
  if (dense) {
    if (a.ld_tok < 0 || a.ld_tok > AIGV_MAX_KV_CAPACITY) return "attention probe: ld_tok is outside 0..AIGV_MAX_KV_CAPACITY (262144)";
    if (!a.tok) return "attention probe: null tok_out with ld_tok > 0";
    if (a.tok_row_stride < (size_t)a.n_heads * a.ld_tok) return "attention probe: tok row stride below n_heads * ld_tok";
  }
  // values form (one D-vector per segment and the rest slot): likewise asked for by either argument
  const bool values = a.v || a.val;
  if (values) {
    if (!a.v) return "attention probe: null v with val_out given";
    if (!a.val) return "attention probe: null val_out with v given";
    if (a.ldv % 8 || ((uintptr_t)a.v & 15)) return "attention probe: V must be 16-byte aligned with a row stride that is a multiple of 8";
    if (a.val_row_stride < (size_t)a.n_heads * (a.n_seg + 1) * head_dim) return "attention probe: val row stride below n_heads * (n_segments + 1) * head_dim";
    if (a.kv_seq_stride ? a.ldv != a.ldk : (int64_t)a.ldv < (int64_t)(a.n_kv_heads - 1) * a.kv_head_stride + head_dim)
      return a.kv_seq_stride ? "attention probe: the V cache takes K's strides (ldv = ldk)" : "attention probe: packed V strides too small";
    if (probe_lds(true, a.n_seg) > AIGV_PROBE_VALUES_MAX_LDS) return "attention probe: the values form's bins and accumulators do not fit the LDS";
  }
  int cap = 0;
  if (a.kv_seq_stride) {   // cache layout [seq][kv head][cap][D]
    if (a.ldk < head_dim || a.kv_head_stride < a.ldk) return "attention probe: cache strides too small";
    cap = a.kv_head_stride / a.ldk;
    if (a.kv_seq_stride < (size_t)a.n_kv_heads * a.kv_head_stride) return "attention probe: kv_seq_stride below n_kv_heads * kv_head_stride";
  } else if (a.kv_head_stride < head_dim || (int64_t)a.ldk < (int64_t)(a.n_kv_heads - 1) * a.kv_head_stride + head_dim) {
    return "attention probe: packed K strides too small";
  }
  for (int i = 0; i < a.n_rows; ++i) {
    const ProbeRow& r = a.tab.r[i];
    if (r.row < 0 || r.row >= total_rows || r.row0 < 0 || r.row0 > r.row || r.seq < 0) return "attention probe: a probe row lies outside the pass";
    if (r.off < 0 || (r.off > 0 && (!a.kv_seq_stride || !a.seg_cached || a.ld_cached < r.off))) return "attention probe: cached keys need the cache layout and a seg_cached table that covers them";
    const int pos = r.off + (r.row - r.row0);
    if (pos >= max_pos) return "attention probe: a probe row's position lies outside the RoPE table";
    if (a.kv_seq_stride && pos >= cap) return "attention probe: a probe row's position lies outside the KV cache";
    if (dense && pos >= a.ld_tok) return "attention probe: ld_tok is below a probe row's key count (position + 1)";
  }
  return nullptr;
}

hipError_t aigv_launch_attention_probe(const ProbeArgs& a, int head_dim, hipStream_t s) {
  return head_dim == 128 ? launch_probe_form<128>(a, s) : head_dim == 64 ? launch_probe_form<64>(a, s) : hipErrorInvalidValue;
}
