// Label log-probabilities of bf16 logits rows: log_softmax(logits.float())[label], the per-token term of the reference's
// CrossEntropyLoss over the answer tokens (internvl_chat_eval2/modeling_internvl_chat.py:452-463, modeling_internlm2.py:1095-1096).
//
// One workgroup of 256 threads per row.  Thread t owns the 4-column chunks t, t + 256, t + 512, ... of the row and keeps an online
// (max, sum of exp(x - max)) over them in fp32, one column after the other; the 256 pairs are then combined by a butterfly inside each
// wave and the four wave results in wave order.  That mapping and that tree depend only on the vocabulary size - never on the
// number of rows, the row's position in the batch or the launch - so a row's result is the same bits alone or inside any batch.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int LP_THREADS = 256;

// VEC: every row start is 8-byte aligned (ldo % 4 == 0 and an aligned base): whole chunks come in as one 8-byte load.  The scalar
// form reads the same columns in the same order - both forms give the same bits.
template <bool VEC>
__global__ __launch_bounds__(LP_THREADS) void label_logprob_kernel(const bf16_t* __restrict__ logits, int V, int ldo,
                                                                   const int64_t* __restrict__ labels, float* __restrict__ out) {
  const int r = blockIdx.x;
  const bf16_t* row = logits + (size_t)r * ldo;
  float m = -INFINITY, s = 0.0f;
#pragma unroll 4
  for (int c = 4 * (int)threadIdx.x; c < V; c += 4 * LP_THREADS) {
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
#pragma unroll
  for (int off = AIGV_WAVE / 2; off >= 1; off >>= 1) lse_combine(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
  __shared__ float wm[LP_THREADS / AIGV_WAVE], ws[LP_THREADS / AIGV_WAVE];
  const int wave = threadIdx.x / AIGV_WAVE, lane = threadIdx.x % AIGV_WAVE;
  if (lane == 0) {
    wm[wave] = m;
    ws[wave] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  m = wm[0];
  s = ws[0];
#pragma unroll
  for (int w = 1; w < LP_THREADS / AIGV_WAVE; ++w) lse_combine(m, s, wm[w], ws[w]);
  const int64_t lab = labels[r];
  out[r] = (lab < 0 || lab >= V) ? __builtin_nanf("") : bf2f(row[lab]) - (m + logf(s));
}

}  // namespace

hipError_t aigv_launch_label_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* labels, float* out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!logits || !labels || !out || V < 1 || ldo < V) return hipErrorInvalidValue;
  const bool vec = ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 7) == 0;
  if (vec) hipLaunchKernelGGL(label_logprob_kernel<true>, dim3(rows), dim3(LP_THREADS), 0, s, logits, V, ldo, labels, out);
  else hipLaunchKernelGGL(label_logprob_kernel<false>, dim3(rows), dim3(LP_THREADS), 0, s, logits, V, ldo, labels, out);
  return hipGetLastError();
}
