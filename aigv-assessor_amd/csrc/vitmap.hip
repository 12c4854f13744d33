// InternViT attention map: the full, NON-causal softmax matrix of every query row of every frame - the vision tower's sibling of the attention
// flow map (attnmap.hip), on the matrix cores.  The flash kernel (attention.hip) never forms a probability matrix; these two stand-alone kernels
// recompute the softmax from the bf16 Q and K the ViT layer leaves in its fused qkv rows (after the full-width QK RMSNorm where the config has
// one) and touch nothing the pass reads afterwards.
//
// Mapped quantity, for frame f, head h, query row i, key j, 0 <= i, j < S:
//   acc_ij   = the fp32 MFMA accumulation of the exact bf16 products q_i . k_j
//   s_ij     = acc_ij / sqrtf(D)
//   m_i      = max_j s_ij
//   e_ij     = expf(s_ij - m_i)
//   total_i  = the fp32 sum of the e_ij, in an order fixed by the key index alone
//   p_ij     = e_ij / total_i
// per head:  out[f][h][i][j] = p_ij
// head mean: out[f][i][j]    = (p0_ij + p1_ij + ... in ascending h, starting from +0.0) / n_heads, ONE fp32 division
// Scores and weights are fp32 whatever aigv_set_attention_numerics says, and the UNSCALED bf16 Q is used: the flash kernel's bf16 q_prescale
// rounding (exact only for D = 64) is not reproduced.
//
// Both kernels use the lane layout of qk_tiles.h (lane (r, hf), rho, the tile product, the two sweeps); the bf16 Q is loaded as it stands.
//   stats kernel, one wave per (32 query rows, head, frame): sweep 1 (qk_raw_max) over ALL key tiles takes the maximum of the raw accumulators
//     over the keys j < S (a key past the frame's end inside the last tile never enters arithmetic), m = max / sqrt(D).  Sweep 2 (qk_weights)
//     recomputes the same accumulators and adds the lane's 16 e_ij per tile in register order, tile after tile; the two lane halves' totals
//     are added (one exchange).  The order of total_i's chain: lane half hf adds, key tiles ascending, the keys rho(0, hf), rho(1, hf), ... of
//     each tile; then half 0 + half 1.  (m_i, total_i) go to stats[f][h][i].
//   write kernel, one wave per (query tile, key tile, frame): for h = 0, 1, ... it recomputes the 32 x 32 accumulator tile (again the same
//     instructions), forms p_ij = expf(acc_ij / sqrt(D) - m_i) / total_i and either stores it or adds it to the head mean kept in registers,
//     which is divided once at the end.  The tile crosses the lanes through LDS so that a store instruction writes 32 consecutive keys of
//     one query row.
// No atomics.  Rows past the frame's end inside its last tile are loaded from the frame's last row (a valid address of the same frame) and
// never stored.  A row's bits depend on its own frame's Q and K alone: nothing depends on the batch mates, the grid or the frame count - and
// integer-valued e_ij (Q = 0: every e_ij is 1) give total_i = S exactly.  Every offset into the output is 64-bit.
#include "common.h"
#include "kernels.h"
#include "qk_tiles.h"

namespace {

template <int D>
__device__ __forceinline__ void vm_load_q(const bf16_t* __restrict__ qp, bf16x8* qf) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s) qf[s] = *(const bf16x8*)(qp + 16 * s);
}

template <int D>
__global__ __launch_bounds__(AIGV_WAVE) void vit_map_stats_kernel(const VitMapArgs p) {
  const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
  const int qt = blockIdx.x, h = blockIdx.y, f = blockIdx.z, S = p.S;
  const int qpos = 32 * qt + r, qc = min(qpos, S - 1);
  const size_t row0 = (size_t)f * S;
  bf16x8 qf[D / 16];
  vm_load_q<D>(p.q + (row0 + qc) * p.ldq + (size_t)h * D + 8 * hf, qf);
  const QkSweep sw = {p.k + row0 * p.ldk + (size_t)h * D + 8 * hf, p.ldk, (S + 31) >> 5, S - 1, S - 1, r, hf};
  const float mx = qk_raw_max<D>(sw, qf);
  const float m = mx / p.post_div;

  float total = 0.0f;
  qk_weights<D>(sw, qf, p.post_div, m, [&](int, int, int, float e) { total += e; });
  total += __shfl_xor(total, 32);
  if (hf == 0 && qpos < S) p.stats[((size_t)f * p.n_heads + h) * S + qpos] = make_float2(m, total);
}

template <int D, bool PER_HEAD>
__global__ __launch_bounds__(AIGV_WAVE) void vit_map_write_kernel(const VitMapArgs p) {
  __shared__ float tile[32][33];                       // [query][key]: written by the query's lane pair, read a query row at a time
  const int lane = threadIdx.x, r = lane & 31, hf = lane >> 5;
  const int qt = blockIdx.x, kt = blockIdx.y, f = blockIdx.z, S = p.S;
  const int qc = min(32 * qt + r, S - 1), kc = min(32 * kt + r, S - 1);
  const size_t row0 = (size_t)f * S;
  const bf16_t* qp = p.q + (row0 + qc) * p.ldq + 8 * hf;
  const bf16_t* kp = p.k + (row0 + kc) * p.ldk + 8 * hf;
  const float2* st = p.stats + (size_t)f * p.n_heads * S + qc;
  float* out = p.out + (size_t)f * p.out_frame_stride;
  const bool key_ok = 32 * kt + r < S;                 // the key this lane STORES (after the exchange)

  auto store = [&](const f32x16& v, float* base) {     // base: element [query 0][key 0] of the S x S matrix
#pragma unroll
    for (int i = 0; i < 16; ++i) tile[r][qk_rho(i, hf)] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = 2 * i + hf;
      if (key_ok && 32 * qt + q < S) base[(size_t)(32 * qt + q) * S + (size_t)(32 * kt + r)] = tile[q][r];
    }
    __syncthreads();
  };

  f32x16 mean = {};
  for (int h = 0; h < p.n_heads; ++h) {
    bf16x8 qf[D / 16];
    vm_load_q<D>(qp + (size_t)h * D, qf);
    const f32x16 acc = qk_scores<D>(kp + (size_t)h * D, qf);
    const float2 mt = st[(size_t)h * S];
    f32x16 pr;
#pragma unroll
    for (int i = 0; i < 16; ++i) pr[i] = expf(acc[i] / p.post_div - mt.x) / mt.y;
    if (PER_HEAD) store(pr, out + (size_t)h * S * S);
    else
#pragma unroll
      for (int i = 0; i < 16; ++i) mean[i] += pr[i];
  }
  if (!PER_HEAD) {
    const float n = (float)p.n_heads;
#pragma unroll
    for (int i = 0; i < 16; ++i) mean[i] = mean[i] / n;
    store(mean, out);
  }
}

template <int D>
hipError_t launch_vit_map(const VitMapArgs& a, hipStream_t s) {
  const int tiles = (a.S + 31) >> 5;
  hipLaunchKernelGGL((vit_map_stats_kernel<D>), dim3(tiles, a.n_heads, a.n_seq), dim3(AIGV_WAVE), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (a.per_head) hipLaunchKernelGGL((vit_map_write_kernel<D, true>), dim3(tiles, tiles, a.n_seq), dim3(AIGV_WAVE), 0, s, a);
  else hipLaunchKernelGGL((vit_map_write_kernel<D, false>), dim3(tiles, tiles, a.n_seq), dim3(AIGV_WAVE), 0, s, a);
  return hipGetLastError();
}

}  // namespace

// Every index the two kernels form is bounded here, on the host: nothing is launched otherwise.
const char* aigv_vit_map_check(const VitMapArgs& a, int head_dim) {
  if (head_dim != 64 && head_dim != 128) return "vit attention map: head_dim must be 64 or 128";
  if (!a.q || !a.k || !a.out || !a.stats) return "vit attention map: null operand";
  if (a.n_heads < 1 || a.n_heads > AIGV_VIT_MAP_MAX_HEADS) return "vit attention map: n_heads is outside 1..64";
  if (a.n_seq < 1 || a.n_seq > AIGV_VIT_MAP_MAX_FRAMES) return "vit attention map: the number of frames is outside 1..65535";
  if (a.S < 1 || a.S > AIGV_VIT_MAP_MAX_ROWS) return "vit attention map: the rows of a frame are outside 1..32768";
  if ((int64_t)a.ldq < (int64_t)a.n_heads * head_dim || (int64_t)a.ldk < (int64_t)a.n_heads * head_dim) return "vit attention map: row strides too small for n_heads * head_dim columns";
  if (a.ldq % 8 || ((uintptr_t)a.q & 15)) return "vit attention map: Q must be 16-byte aligned with a row stride that is a multiple of 8";
  if (a.ldk % 8 || ((uintptr_t)a.k & 15)) return "vit attention map: K must be 16-byte aligned with a row stride that is a multiple of 8";
  if (((uintptr_t)a.out & 3) || ((uintptr_t)a.stats & 7)) return "vit attention map: out must be 4-byte and the stats scratch 8-byte aligned";
  if (a.out_frame_stride < (size_t)(a.per_head ? a.n_heads : 1) * a.S * a.S) return "vit attention map: the output's frame stride does not hold a frame's maps";
  if (!(a.post_div > 0.0f)) return "vit attention map: post_div must be positive";
  return nullptr;
}

hipError_t aigv_launch_vit_map(const VitMapArgs& a, int head_dim, hipStream_t s) {
  return head_dim == 128 ? launch_vit_map<128>(a, s) : head_dim == 64 ? launch_vit_map<64>(a, s) : hipErrorInvalidValue;
}
