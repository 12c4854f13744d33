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
#include "common.h"
#include "kernels.h"

namespace {

constexpr int CAND_LD = AIGV_MAX_CANDIDATES;   // row stride of the decode step's candidate-logit scratch [R][CAND_LD] bf16

// out[r][t] = logits[r][id] - lse(row r) with id = ids[r * id_row_stride + t], t < C: labels are (C = 1, stride 1), candidates (C, stride 0).
// An id outside [0, V) gives NaN.  VEC: every row start is 8-byte aligned (ldo % 4 == 0 and an aligned base): whole chunks come in as one
// 8-byte load.  The scalar form reads the same columns in the same order - both forms give the same bits.
template <bool VEC>
__global__ __launch_bounds__(LSE_THREADS) void row_logprob_kernel(const bf16_t* __restrict__ logits, int V, int ldo, const int64_t* __restrict__ ids,
                                                                 int id_row_stride, int C, float* __restrict__ out) {
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
  if ((int)threadIdx.x >= C) return;
  const int64_t id = ids[(size_t)r * id_row_stride + threadIdx.x];
  out[(size_t)r * C + threadIdx.x] = (id < 0 || id >= V) ? __builtin_nanf("") : bf2f(row[id]) - lse;
}

hipError_t launch_row_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* ids, int id_row_stride, int C, float* out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!logits || !ids || !out || V < 1 || ldo < V || C < 1 || C > AIGV_MAX_CANDIDATES) return hipErrorInvalidValue;
  const bool vec = ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 7) == 0;
  if (vec) hipLaunchKernelGGL(row_logprob_kernel<true>, dim3(rows), dim3(LSE_THREADS), 0, s, logits, V, ldo, ids, id_row_stride, C, out);
  else hipLaunchKernelGGL(row_logprob_kernel<false>, dim3(rows), dim3(LSE_THREADS), 0, s, logits, V, ldo, ids, id_row_stride, C, out);
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
// cand_logit[r][c] - lse, NaN for an id outside [0, V).
__global__ __launch_bounds__(LSE_THREADS) void lse_finish_kernel(const unsigned long long* __restrict__ packed, const float2* __restrict__ part, int nslot,
                                                                int V, const int64_t* __restrict__ cand, int C, const bf16_t* __restrict__ cand_logit,
                                                                int64_t* __restrict__ idx, float* __restrict__ val, float* __restrict__ logprob,
                                                                float* __restrict__ cand_logprob) {
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

size_t aigv_cand_logit_elems(int R) { return (size_t)R * CAND_LD; }

hipError_t aigv_launch_lm_head_argmax_logprob(const bf16_t* h, int R, int H, const bf16_t* W, int V, unsigned long long* packed, float2* part,
                                              int64_t* out_idx, float* out_val, float* out_logprob, hipStream_t s, const int64_t* cand, int C,
                                              bf16_t* cand_logit, float* out_cand) {
  if (R <= 0) return hipSuccess;
  if (!out_idx || !out_logprob || C < 0 || C > AIGV_MAX_CANDIDATES || (C > 0 && (!cand || !cand_logit || !out_cand))) return hipErrorInvalidValue;
  hipError_t e = aigv_launch_lm_head_lse_partials(h, R, H, W, V, packed, part, s);
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
  hipLaunchKernelGGL(lse_finish_kernel, dim3(R), dim3(LSE_THREADS), 0, s, packed, part, (int)aigv_lm_head_lse_slots(V), V, cand, C,
                     cand_logit, out_idx, out_val, out_logprob, out_cand);
  return hipGetLastError();
}
