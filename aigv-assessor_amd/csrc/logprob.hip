// Log-probabilities of chosen tokens: log_softmax(logits.float())[id] over a row's bf16 lm-head logits - the per-token term of the
// reference's CrossEntropyLoss over the answer tokens (internvl_chat_eval2/modeling_internvl_chat.py:452-463, modeling_internlm2.py:
// 1095-1096), read at the row's label (`logprob`) or at C <= 64 candidate ids shared by all rows (`cand_logprob`: the quality levels'
// first answer tokens, "The quality of the video is <level>.").
//
// Two kernels, one workgroup of LSE_THREADS = 256 threads per row, and ONE reduction (lse_of_block, common.h):
//   row_logprob_kernel  scoring pass: thread t folds the 4-column chunks t, t + 256, ... of the row's logits into a (max, sum-exp) pair.
//   lse_finish_kernel   decode step: thread t folds the slots t, t + 256, ... of the lm-head's per-16-column partials (SK_ARGMAX_LSE,
//                       head.hip); the C candidate logits come from cand_gemv_kernel.
// Both hand the pair to lse_of_block and subtract the row's log-sum-exp it returns from gathered bf16 logits.  What a thread folds, and in
// which order, is fixed by the vocabulary size alone; the tree behind it by the thread count.  Hence, from the source:
//   label == candidate column   both launchers run row_logprob_kernel; they differ in where thread t finds its id (ids[r] / ids[t])
//   finisher == finisher with candidates   one kernel; the candidates add stores after the reduction, never an operation inside it
//   scalar == vector            VEC changes how a chunk is loaded, not which columns it holds nor the order they are pushed in
//   alone == in a batch         nothing above reads the row count, the row's index or C before the log-sum-exp is final
//
// Top-k (topk_of_row below) is a third set of stores behind the same reductions: the TOPK instantiations of the two kernels run the fold and
// lse_of_block of the plain ones and then select over the row's bf16 logits - the scoring pass's own row, or the row the lm-head's
// SK_ARGMAX_LSE_STORE form (head.hip) kept.  The plain instantiations are the code they were.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int CAND_LD = AIGV_MAX_CANDIDATES;   // row stride of the decode step's candidate-logit scratch [R][CAND_LD] bf16

// The k largest logits of one row and their log-probabilities, in the order of the lm-head's packed argmax key (argmax_key, common.h: bf16
// logit descending, equal logits by ascending column) - entry 0 is the argmax token by the first-max rule, entry j the largest key strictly
// below entry j - 1's.  The keys are a strict total order, so nothing needs an exclusion list.  Every thread keeps the TOPK_KEEP largest
// keys of its own columns (the 4-column chunks t, t + 256, ... of the row kernel), sorted; a round takes the maximum of the threads' heads
// over the workgroup (butterfly per wave, four wave maxima through LDS, double-buffered: one barrier per round), thread 0 stores it and
// its owner pops it - and scans its columns again, for keys below the winner, only once its list has run dry (a row with many of its
// largest logits in one thread's columns: rows of ties).  So a row costs one pass plus k rounds of shuffles.  Comparisons only: VEC (8-byte
// loads of whole chunks from 8-byte aligned rows) cannot change a bit.  ids[j] / lp[j] = column and float(logit) - lse.  Called by all
// LSE_THREADS threads of a workgroup with 1 <= k <= min(V, AIGV_MAX_TOPK); it sees one row and its log-sum-exp, never a row index or count.
constexpr int TOPK_KEEP = 4;

// top[] <- the TOPK_KEEP largest keys below `below` among this thread's columns, descending, 0 = none (no key is 0: column < 2^32 - 1)
template <bool VEC>
__device__ __forceinline__ void topk_scan(const bf16_t* __restrict__ row, int V, unsigned long long below, unsigned long long (&top)[TOPK_KEEP]) {
#pragma unroll
  for (int i = 0; i < TOPK_KEEP; ++i) top[i] = 0ull;
#pragma unroll 4
  for (int c = 4 * (int)threadIdx.x; c < V; c += 4 * LSE_THREADS) {
    bf16_t x[4];
    if (VEC && c + 4 <= V) {
      const u16x4 v = *(const u16x4*)(row + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = c + j < V ? row[c + j] : (bf16_t)0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned long long key = argmax_key(bf2f(x[j]), c + j);
      if (c + j < V && key < below && key > top[TOPK_KEEP - 1]) {
#pragma unroll
        for (int i = 0; i < TOPK_KEEP; ++i) {      // sorted insert: the key sinks to its place, the last one falls out
          const unsigned long long hi = key > top[i] ? key : top[i];
          key = key > top[i] ? top[i] : key;
          top[i] = hi;
        }
      }
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void topk_of_row(const bf16_t* __restrict__ row, int V, int k, float lse, int64_t* __restrict__ ids, float* __restrict__ lp) {
  __shared__ unsigned long long wk[2][LSE_THREADS / AIGV_WAVE];
  const int wave = threadIdx.x / AIGV_WAVE, lane = threadIdx.x % AIGV_WAVE;
  unsigned long long top[TOPK_KEEP];
  topk_scan<VEC>(row, V, ~0ull, top);               // (no key is ~0 either: a bf16 logit's order word never has all bits set)
  for (int j = 0; j < k; ++j) {
    unsigned long long w = top[0];
#pragma unroll
    for (int off = AIGV_WAVE / 2; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(w, off);
      w = o > w ? o : w;
    }
    if (lane == 0) wk[j & 1][wave] = w;
    __syncthreads();
    w = wk[j & 1][0];
#pragma unroll
    for (int i = 1; i < LSE_THREADS / AIGV_WAVE; ++i) w = wk[j & 1][i] > w ? wk[j & 1][i] : w;
    if (threadIdx.x == 0) {
      float v;
      unpack_argmax_key(w, ids[j], v);
      lp[j] = v - lse;
    }
    if (top[0] == w) {                               // keys are distinct: one owner
#pragma unroll
      for (int i = 0; i + 1 < TOPK_KEEP; ++i) top[i] = top[i + 1];
      top[TOPK_KEEP - 1] = 0ull;
      if (top[0] == 0ull && j + 1 < k) topk_scan<VEC>(row, V, w, top);
    }
  }
}

// out[r][t] = logits[r][id] - lse(row r) with id = ids[r * id_row_stride + t], t < C: labels are (C = 1, stride 1), candidates (C, stride 0).
// An id outside [0, V) gives NaN.  VEC: every row start is 8-byte aligned (ldo % 4 == 0 and an aligned base): whole chunks come in as one
// 8-byte load.  The scalar form reads the same columns in the same order - both forms give the same bits.
// TOPK: the ids are optional (C = 0) and the row's k largest logits follow the same log-sum-exp (topk_of_row) into top_ids / top_lp [rows][k].
template <bool VEC, bool TOPK = false>
__global__ __launch_bounds__(LSE_THREADS) void row_logprob_kernel(const bf16_t* __restrict__ logits, int V, int ldo, const int64_t* __restrict__ ids,
                                                                 int id_row_stride, int C, float* __restrict__ out, int k = 0,
                                                                 int64_t* __restrict__ top_ids = nullptr, float* __restrict__ top_lp = nullptr) {
  const int r = blockIdx.x;
  const bf16_t* row = logits + (size_t)r * ldo;
  float m = -INFINITY, s = 0.0f;
#pragma unroll 4
  for (int c = 4 * (int)threadIdx.x; c < V; c += 4 * LSE_THREADS) {
    float x[4];
    if (VEC && c + 4 <= V) {
      const u16x4 v = *(const u16x4*)(row + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = bf2f(v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = c + j < V ? bf2f(row[c + j]) : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) lse_push(m, s, x[j]);
  }
  const float lse = lse_of_block<false>(m, s);
  if constexpr (TOPK) topk_of_row<VEC>(row, V, k, lse, top_ids + (size_t)r * k, top_lp + (size_t)r * k);
  if ((int)threadIdx.x >= C) return;
  const int64_t id = ids[(size_t)r * id_row_stride + threadIdx.x];
  out[(size_t)r * C + threadIdx.x] = (id < 0 || id >= V) ? __builtin_nanf("") : bf2f(row[id]) - lse;
}

hipError_t launch_row_topk(const bf16_t* logits, int rows, int V, int ldo, int k, int64_t* top_ids, float* top_lp, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!logits || !top_ids || !top_lp || V < 1 || ldo < V || k < 1 || k > AIGV_MAX_TOPK || k > V) return hipErrorInvalidValue;
  const bool vec = ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 7) == 0;
  if (vec) hipLaunchKernelGGL((row_logprob_kernel<true, true>), dim3(rows), dim3(LSE_THREADS), 0, s, logits, V, ldo, nullptr, 0, 0, nullptr, k, top_ids, top_lp);
  else hipLaunchKernelGGL((row_logprob_kernel<false, true>), dim3(rows), dim3(LSE_THREADS), 0, s, logits, V, ldo, nullptr, 0, 0, nullptr, k, top_ids, top_lp);
  return hipGetLastError();
}

hipError_t launch_row_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* ids, int id_row_stride, int C, float* out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!logits || !ids || !out || V < 1 || ldo < V || C < 1 || C > AIGV_MAX_CANDIDATES) return hipErrorInvalidValue;
  const bool vec = ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 7) == 0;
  if (vec) hipLaunchKernelGGL((row_logprob_kernel<true, false>), dim3(rows), dim3(LSE_THREADS), 0, s, logits, V, ldo, ids, id_row_stride, C, out);
  else hipLaunchKernelGGL((row_logprob_kernel<false, false>), dim3(rows), dim3(LSE_THREADS), 0, s, logits, V, ldo, ids, id_row_stride, C, out);
  return hipGetLastError();
}

// The decode step's candidate logits, with the lm-head kernel's arithmetic so that a column gets the bits that kernel rounds for it
// whatever slab it sits in there (tests/test_gpu_cand_logprob.py holds the two against each other): four K slices of K / 4, one MFMA
// 16x16x32 chain per slice in ascending k, slices summed as acc0 + ((p1 + p2) + p3), one bf16 rounding - an MFMA output element depends on
// its own A row and B column only.  Extra weight bytes per step: ceil16(C) x hidden x 2.
// logit[r][16 b + j] = bf16(x_r . W[cand[16 b + j]]) for workgroup b: skinny_kernel's one-slab, four-slice form with the slab's rows
// gathered by id.  Lane (fr, fq) streams 8-element fragments of W row cand[16 b + fr]; slots past C repeat the last candidate and ids
// outside [0, N) are clamped (their columns are NaN in the finisher) - every load stays inside W.  The id is read once per lane, in
// front of the K loop.
template <int RT>
__global__ __launch_bounds__(256) void cand_gemv_kernel(const bf16_t* __restrict__ x, int ldx, int R, const bf16_t* __restrict__ W, int ldw,
                                                        int N, int K, const int64_t* __restrict__ cand, int C, bf16_t* __restrict__ out) {
  __shared__ float part[3][RT][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int64_t id = cand[min((int)blockIdx.x * 16 + fr, C - 1)];
  const int n = (int)(id < 0 ? 0 : id >= N ? N - 1 : id);
  const int kper = K / 4, kbeg = wave * kper;           // K % 128 == 0 checked by the launcher
  const bf16_t* wrow = W + (size_t)n * ldw + kbeg + fq * 8;
  const bf16_t* xrow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) xrow[t] = x + (size_t)min(t * 16 + fr, R - 1) * ldx + kbeg + fq * 8;
  f32x4 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int DEPTH = RT == 1 ? 8 : 4;                // k-steps loaded ahead of their MFMAs; the order of the chain is k's either way
  int k = 0;
  for (; k + 32 * DEPTH <= kper; k += 32 * DEPTH) {
    bf16x8 wf[DEPTH], xf[DEPTH][RT];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      wf[u] = *(const bf16x8*)(wrow + k + 32 * u);
#pragma unroll
      for (int t = 0; t < RT; ++t) xf[u][t] = *(const bf16x8*)(xrow[t] + k + 32 * u);
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u)
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u], xf[u][t], acc[t], 0, 0, 0);
  }
  for (; k < kper; k += 32) {
    const bf16x8 wf = *(const bf16x8*)(wrow + k);
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, *(const bf16x8*)(xrow[t] + k), acc[t], 0, 0, 0);
  }
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) part[wave - 1][t][e][lane] = acc[t][e];
  }
  __syncthreads();
  if (wave != 0) return;
  // lane owns x row 16 t + fr and candidate slots 16 b + 4 fq + e
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    u16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[t][e] + ((part[0][t][e][lane] + part[1][t][e][lane]) + part[2][t][e][lane]));
    const int r = t * 16 + fr;
    if (r < R) *(u16x4*)(out + (size_t)r * CAND_LD + blockIdx.x * 16 + 4 * fq) = o;
  }
}

// SK_ARGMAX_LSE's finisher: the lm-head's per-slab pairs part[r][0 .. nslot) -> the row's log-sum-exp; thread 0 writes idx / val (the
// packed key's, as unpack_argmax_kernel) and logprob = val - lse.  Candidates are optional (cand == nullptr, C = 0): thread c < C writes
// cand_logit[r][c] - lse, NaN for an id outside [0, V).  TOPK: the row's k largest logits, selected from the row the lm-head stored
// (row_logit[r][ldl], 8-byte aligned rows) under this log-sum-exp - so top_lp[r][0] is logprob[r], bit for bit.
template <bool TOPK>
__global__ __launch_bounds__(LSE_THREADS) void lse_finish_kernel(const unsigned long long* __restrict__ packed, const float2* __restrict__ part, int nslot,
                                                                int V, const int64_t* __restrict__ cand, int C, const bf16_t* __restrict__ cand_logit,
                                                                int64_t* __restrict__ idx, float* __restrict__ val, float* __restrict__ logprob,
                                                                float* __restrict__ cand_logprob, const bf16_t* __restrict__ row_logit = nullptr,
                                                                int ldl = 0, int k = 0, int64_t* __restrict__ top_ids = nullptr,
                                                                float* __restrict__ top_lp = nullptr) {
  const int r = blockIdx.x;
  const float2* row = part + (size_t)r * nslot;
  float m = -INFINITY, s = 0.f;
  for (int i = threadIdx.x; i < nslot; i += LSE_THREADS) {
    const float2 p = row[i];
    lse_combine(m, s, p.x, p.y);
  }
  const float lse = lse_of_block<true>(m, s);
  if ((int)threadIdx.x < C) {
    const int64_t id = cand[threadIdx.x];
    cand_logprob[(size_t)r * C + threadIdx.x] = (id < 0 || id >= V) ? __builtin_nanf("") : bf2f(cand_logit[(size_t)r * CAND_LD + threadIdx.x]) - lse;
  }
  if constexpr (TOPK) topk_of_row<true>(row_logit + (size_t)r * ldl, V, k, lse, top_ids + (size_t)r * k, top_lp + (size_t)r * k);
  if (threadIdx.x != 0) return;
  float v;
  unpack_argmax_key(packed[r], idx[r], v);
  if (val) val[r] = v;
  logprob[r] = v - lse;
}

}  // namespace

hipError_t aigv_launch_label_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* labels, float* out, hipStream_t s) {
  return launch_row_logprob(logits, rows, V, ldo, labels, 1, 1, out, s);
}

hipError_t aigv_launch_cand_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* cand, int C, float* out, hipStream_t s) {
  return launch_row_logprob(logits, rows, V, ldo, cand, 0, C, out, s);
}

hipError_t aigv_launch_topk_logprob(const bf16_t* logits, int rows, int V, int ldo, int k, int64_t* top_ids, float* top_logprob, hipStream_t s) {
  return launch_row_topk(logits, rows, V, ldo, k, top_ids, top_logprob, s);
}

size_t aigv_topk_logit_ld(int V) { return (size_t)(V + 3) / 4 * 4; }

size_t aigv_cand_logit_elems(int R) { return (size_t)R * CAND_LD; }

hipError_t aigv_launch_lm_head_argmax_logprob(const bf16_t* h, int R, int H, const bf16_t* W, int V, unsigned long long* packed, float2* part,
                                              int64_t* out_idx, float* out_val, float* out_logprob, hipStream_t s, const int64_t* cand, int C,
                                              bf16_t* cand_logit, float* out_cand, int k, bf16_t* row_logit, int ldl, int64_t* top_ids,
                                              float* top_logprob) {
  if (R <= 0) return hipSuccess;
  if (!out_idx || !out_logprob || C < 0 || C > AIGV_MAX_CANDIDATES || (C > 0 && (!cand || !cand_logit || !out_cand))) return hipErrorInvalidValue;
  if (k < 0 || k > AIGV_MAX_TOPK || k > V || (k > 0 && (!row_logit || !top_ids || !top_logprob))) return hipErrorInvalidValue;
  hipError_t e = aigv_launch_lm_head_lse_partials(h, R, H, W, V, packed, part, s, k > 0 ? row_logit : nullptr, ldl);
  if (e != hipSuccess) return e;
  if (C > 0) {
    const dim3 grid((C + 15) / 16);
#define GO(RT) hipLaunchKernelGGL(cand_gemv_kernel<RT>, grid, dim3(256), 0, s, h, H, R, W, H, V, H, cand, C, cand_logit)
    switch ((R + 15) / 16) {
      case 1: GO(1); break;
      case 2: GO(2); break;
      case 3: GO(3); break;
      default: GO(4); break;
    }
#undef GO
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (k > 0)
    hipLaunchKernelGGL(lse_finish_kernel<true>, dim3(R), dim3(LSE_THREADS), 0, s, packed, part, (int)aigv_lm_head_lse_slots(V), V, cand, C,
                       cand_logit, out_idx, out_val, out_logprob, out_cand, row_logit, ldl, k, top_ids, top_logprob);
  else
    hipLaunchKernelGGL(lse_finish_kernel<false>, dim3(R), dim3(LSE_THREADS), 0, s, packed, part, (int)aigv_lm_head_lse_slots(V), V, cand, C,
                       cand_logit, out_idx, out_val, out_logprob, out_cand);
  return hipGetLastError();
}
