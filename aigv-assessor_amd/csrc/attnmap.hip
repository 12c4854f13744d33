// Attention flow map: where EVERY query row of a causal GQA attention looks, folded into a few key segments - the all-rows sibling of the
// score-row probe (attnprobe.hip), on the matrix cores.  The flash prefill kernel (attention.hip) never forms a probability matrix; this
// stand-alone kernel recomputes the softmax of all rows from the Q (unrotated) and K (rotated) that llm_layer_qkv leaves in the fused qkv rows
// and touches nothing the pass itself reads afterwards.  Packed layout only.
//
// One wave per (32 query rows of ONE sequence, query head), in the lane layout of qk_tiles.h (lane (r, hf), rho, the tile product, the two
// sweeps): query tile i of a sequence is its positions 32 i .. 32 i + 31, key tile kt its keys 32 kt .. 32 kt + 31 - both counted from the
// sequence's first row, so a row's arithmetic is a function of its position, never of where the sequence lies in the pack.
//   1. lane (r, hf) loads its columns of query row r and rotates them at the row's position with rope_pair (common.h) - both halves of a rotary
//      pair lie on the same lane - the bf16 bits the probe and the flash kernel use.  These are the B fragments of every product below;
//   2. sweep 1 (qk_raw_max) over the key tiles 0 .. i takes the maximum of the raw accumulators over the keys j <= p (the causal rule; a key
//      behind the row, or past the sequence's end, never enters arithmetic), then m = max / sqrt(D);
//   3. sweep 2 (qk_weights) recomputes the same accumulators, e_j = expf(acc_j / sqrt(D) - m), 0 for a key the row does not see; the lane adds
//      its 16 e_j per tile to its total in register order, tile after tile;
//   4. binning without rounding the weights and without atomics: bins^T[seg, q] += OneHot^T[seg, key] . P^T[key, q] on the fp32-input
//      v_mfma_f32_32x32x2_f32 - bit for bit a k-ordered fmaf chain, the factor exactly 1 or 0 - whose B operand IS accumulator register i
//      (k = hf), the A operand the lane's own comparison seg[key rho(i, hf)] == r.  32 segments per pass, a second accumulator for 33 .. 64.
//      The chain of one bin: key tiles ascending, inside a tile the keys 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ... (rho's order);
//   5. total = the two lane halves' totals added (one lane ^ 32 exchange); rows[t][h][seg] = bin / total, ONE fp32 division.
// Key tiles behind the query tile are never visited.  Rows past the sequence's end inside its last tile are loaded from the sequence's last
// row (a valid address) and never stored.  A row's bits depend on its own keys, its position and the segment table alone: nothing depends on
// the batch mates, the grid or the row count - and integer-valued e_j (Q = 0: every e_j is 1) give exact counts.
//
// The fold kernel (attn_map_fold_kernel) turns the rows into the segment-to-segment matrix: one thread per (a, c) walks the rows of one
// sequence in ascending order, adds rows[t][h][c] of the rows whose id is a (a plain fp32 chain from +0.0) and divides ONCE by their number -
// 0 / 0 = NaN where the segment has no row.  No atomics.
#include "common.h"
#include "kernels.h"
#include "qk_tiles.h"

namespace {

template <int D, int NP>
__global__ __launch_bounds__(AIGV_WAVE) void attn_map_kernel(const AttnMapArgs p) {
  const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
  int b = 0, t0 = 0;                                   // the sequence of this query tile (the grid is exactly the sum of the tile counts)
  for (; b < p.n_seq - 1; ++b) {
    const int nt = (p.cu[b + 1] - p.cu[b] + 31) >> 5;
    if ((int)blockIdx.x < t0 + nt) break;
    t0 += nt;
  }
  const int row0 = p.cu[b], len = p.cu[b + 1] - row0, qt = blockIdx.x - t0;
  const int h = blockIdx.y, g = p.n_heads / p.n_kv_heads, hk = h / g, S = p.n_seg;
  const int qpos = 32 * qt + r, qc = min(qpos, len - 1);
  constexpr int NS = D / 16, half = D / 2;

  bf16x8 qf[NS];
  {
    const bf16_t* qp = p.q + (size_t)(row0 + qc) * p.ldq + (size_t)hk * p.q_group_stride + (size_t)(h % g) * D + 8 * hf;
    u16x8 raw[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) raw[s] = *(const u16x8*)(qp + 16 * s);
#pragma unroll
    for (int s = 0; s < NS / 2; ++s) {
      const size_t tb = (size_t)qc * half + 16 * s + 8 * hf;
      const u16x8 co = *(const u16x8*)(p.rope_cos + tb), si = *(const u16x8*)(p.rope_sin + tb);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bf16_t lo, hi;
        rope_pair(raw[s][j], raw[s + NS / 2][j], co[j], si[j], lo, hi);
        raw[s][j] = lo;
        raw[s + NS / 2][j] = hi;
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = __builtin_bit_cast(bf16x8, raw[s]);
  }

  const QkSweep sw = {p.k + (size_t)row0 * p.ldk + (size_t)hk * p.kv_head_stride + 8 * hf, p.ldk, qt + 1, qc, len - 1, r, hf};
  const float mx = qk_raw_max<D>(sw, qf);
  const float m = mx / p.post_div;

  f32x16 bins[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) bins[q] = f32x16{};
  float total = 0.0f;
  const int32_t* sg = p.seg + row0;
  qk_weights<D>(sw, qf, p.post_div, m, [&](int, int, int key, float e) {
    const int id = sg[min(key, len - 1)];
    total += e;
#pragma unroll
    for (int q = 0; q < NP; ++q) bins[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(id == r + 32 * q ? 1.0f : 0.0f, e, bins[q], 0, 0, 0);
  });
  total += __shfl_xor(total, 32);

  if (qpos < len) {
    float* out = p.rows + ((size_t)(row0 + qpos) * p.n_heads + h) * S;
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int s = 32 * q + qk_rho(i, hf);
        if (s < S) out[s] = bins[q][i] / total;
      }
  }
}

constexpr int FOLD_THREADS = 256;

__global__ __launch_bounds__(FOLD_THREADS) void attn_map_fold_kernel(const AttnMapArgs p) {
  const int S = p.n_seg, x = blockIdx.x * FOLD_THREADS + threadIdx.x;
  if (x >= S * S) return;
  const int a = x / S, c = x % S, h = blockIdx.y, b = blockIdx.z;
  float sum = 0.0f;
  int n = 0;
  constexpr int UN = 8;                                // rows in flight: the loads do not depend on the chain, the additions keep their order
  const int end = p.cu[b + 1];
  for (int t0 = p.cu[b]; t0 < end; t0 += UN) {
    bool mine[UN];
    float v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) mine[u] = t0 + u < end && p.seg[t0 + u] == a;
#pragma unroll
    for (int u = 0; u < UN; ++u) v[u] = mine[u] ? p.rows[((size_t)(t0 + u) * p.n_heads + h) * S + c] : 0.0f;
#pragma unroll
    for (int u = 0; u < UN; ++u)
      if (mine[u]) {
        sum += v[u];
        ++n;
      }
  }
  p.seg_out[(size_t)b * p.seg_out_seq_stride + ((size_t)h * S + a) * S + c] = sum / (float)n;
}

template <int D>
hipError_t launch_map(const AttnMapArgs& a, int tiles, hipStream_t s) {
  if (a.n_seg <= 32) hipLaunchKernelGGL((attn_map_kernel<D, 1>), dim3(tiles, a.n_heads), dim3(AIGV_WAVE), 0, s, a);
  else hipLaunchKernelGGL((attn_map_kernel<D, 2>), dim3(tiles, a.n_heads), dim3(AIGV_WAVE), 0, s, a);
  return hipGetLastError();
}

}  // namespace

// Every index the two kernels form is bounded here, on the host, from the sequence table that travels as the kernels' argument: nothing is
// launched otherwise.
const char* aigv_attn_map_check(const AttnMapArgs& a, int head_dim, int max_pos) {
  if (head_dim != 64 && head_dim != 128) return "attention map: head_dim must be 64 or 128";
  if (!a.q || !a.k || !a.rope_cos || !a.rope_sin || !a.seg || !a.rows) return "attention map: null operand";
  if (a.n_seg < 1 || a.n_seg > AIGV_MAX_ATTN_SEGMENTS) return "attention map: the number of segments is outside 1..AIGV_MAX_ATTN_SEGMENTS (64)";
  if (a.n_kv_heads < 1 || a.n_heads < a.n_kv_heads || a.n_heads % a.n_kv_heads || a.n_heads > 65535) return "attention map: n_heads must be a multiple of n_kv_heads";
  const int g = a.n_heads / a.n_kv_heads;
  if (a.q_group_stride < g * head_dim || (int64_t)a.ldq < (int64_t)(a.n_kv_heads - 1) * a.q_group_stride + g * head_dim) return "attention map: q strides too small";
  if (a.ldq % 8 || a.q_group_stride % 8 || ((uintptr_t)a.q & 15)) return "attention map: Q must be 16-byte aligned with strides that are multiples of 8";
  if (a.ldk % 8 || a.kv_head_stride % 8 || ((uintptr_t)a.k & 15)) return "attention map: K must be 16-byte aligned with strides that are multiples of 8";
  if (a.kv_head_stride < head_dim || (int64_t)a.ldk < (int64_t)(a.n_kv_heads - 1) * a.kv_head_stride + head_dim) return "attention map: packed K strides too small";
  if (((uintptr_t)a.rope_cos & 15) || ((uintptr_t)a.rope_sin & 15)) return "attention map: the RoPE tables must be 16-byte aligned";
  if (!(a.post_div > 0.0f)) return "attention map: post_div must be positive";
  if (a.n_seq < 1 || a.n_seq > AIGV_MAP_MAX_SEQS) return "attention map: the number of sequences is outside 1..127";
  if (a.cu[0] != 0) return "attention map: cu[0] must be 0";
  for (int b = 0; b < a.n_seq; ++b) {
    if (a.cu[b + 1] <= a.cu[b]) return "attention map: an empty sequence";
    if (a.cu[b + 1] - a.cu[b] > max_pos) return "attention map: a sequence is longer than the RoPE table";
  }
  if (a.seg_out && a.seg_out_seq_stride < (size_t)a.n_heads * a.n_seg * a.n_seg) return "attention map: seg_out sequence stride below n_heads * n_segments^2";
  return nullptr;
}

hipError_t aigv_launch_attention_map(const AttnMapArgs& a, int head_dim, hipStream_t s) {
  int tiles = 0;
  for (int b = 0; b < a.n_seq; ++b) tiles += (a.cu[b + 1] - a.cu[b] + 31) >> 5;
  hipError_t e = head_dim == 128 ? launch_map<128>(a, tiles, s) : head_dim == 64 ? launch_map<64>(a, tiles, s) : hipErrorInvalidValue;
  if (e != hipSuccess || !a.seg_out) return e;
  hipLaunchKernelGGL(attn_map_fold_kernel, dim3((a.n_seg * a.n_seg + FOLD_THREADS - 1) / FOLD_THREADS, a.n_heads, a.n_seq), dim3(FOLD_THREADS), 0, s, a);
  return hipGetLastError();
}
