// The 32 x 32 Q K^T tile core of the two attention-map files (attnmap.hip, vitmap.hip), on the matrix cores: device-only, no kernels.
//
// attention.hip's "key on the row, query on the lane".  One wave owns 32 query rows; query tile qt is the rows 32 qt .. 32 qt + 31, key tile kt the
// keys 32 kt .. 32 kt + 31, both counted from the first row of the sequence (or frame):
//   - lane (r, hf) = (lane & 31, lane >> 5) holds the columns 16 s + 8 hf .. + 7 (s = 0 .. D / 16 - 1) of query row r as the B fragments qf[s] of
//     every product - how they are loaded (and rotated) is the caller's; a lane owns ONE query column;
//   - the key tile's rows are the A fragments: lane (r, hf) loads the same columns of key row r, so a key pointer carries the + 8 hf as well;
//   - S^T[key, q] = K . Q^T on v_mfma_f32_32x32x16_bf16 (bf16 products are exact; fp32 accumulation): accumulator register i of lane (r, hf) is
//     the score of key 32 kt + rho(i, hf), rho = (i & 3) + 8 (i >> 2) + 4 hf, for query r.
// The two sweeps below walk the same tiles with the same instructions, so sweep 2 sees the accumulator bits sweep 1 took the maximum of.  A key
// behind last_key is selected away and never enters arithmetic - NaN there is harmless; a key row behind last_row is loaded from last_row, a valid
// address.
#pragma once
#include "common.h"

__device__ __forceinline__ int qk_rho(int i, int hf) { return (i & 3) + 8 * (i >> 2) + 4 * hf; }

// the tile product: D / 16 MFMA steps into a zero accumulator.  kp = the lane's key row, at its + 8 hf
template <int D>
__device__ __forceinline__ f32x16 qk_scores(const bf16_t* __restrict__ kp, const bf16x8* qf) {
  f32x16 acc = {};
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const bf16x8 a = *(const bf16x8*)(kp + 16 * s);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], acc, 0, 0, 0);
  }
  return acc;
}

// what a lane sweeps: the key tiles 0 .. n_kt - 1 of the rows at kb (the first key row, at the lane's + 8 hf), of which the lane's query sees the
// keys <= last_key; last_row = the last row that may be loaded
struct QkSweep {
  const bf16_t* kb;
  int ldk, n_kt, last_key, last_row, r, hf;
};

// sweep 1: the maximum of the RAW accumulators over the visible keys, both lane halves (one lane ^ 32 exchange).  The caller divides by post_div:
// division by a positive number is monotonic, so that IS max_j s_j with s_j = acc_j / post_div
template <int D>
__device__ __forceinline__ float qk_raw_max(const QkSweep& w, const bf16x8* qf) {
  float mx = -INFINITY;
  for (int kt = 0; kt < w.n_kt; ++kt) {
    const f32x16 acc = qk_scores<D>(w.kb + (size_t)min(32 * kt + w.r, w.last_row) * w.ldk, qf);
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = 32 * kt + qk_rho(i, w.hf) <= w.last_key ? fmaxf(mx, acc[i]) : mx;
  }
  return fmaxf(mx, __shfl_xor(mx, 32));
}

// sweep 2: f(kt, i, key, e) for every accumulator register, tiles ascending, i = 0 .. 15 inside a tile; e = expf(acc / post_div - m), 0 for a key
// the query does not see
template <int D, class F>
__device__ __forceinline__ void qk_weights(const QkSweep& w, const bf16x8* qf, float post_div, float m, F&& f) {
  for (int kt = 0; kt < w.n_kt; ++kt) {
    const f32x16 acc = qk_scores<D>(w.kb + (size_t)min(32 * kt + w.r, w.last_row) * w.ldk, qf);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int key = 32 * kt + qk_rho(i, w.hf);
      const float e = key <= w.last_key ? expf(acc[i] / post_div - m) : 0.0f;
      f(kt, i, key, e);
    }
  }
}
