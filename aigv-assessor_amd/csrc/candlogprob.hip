// Candidate-token log-probabilities: for C <= 64 chosen token ids, log_softmax(logits.float())[cand[c]] of a row's bf16 logits - the
// full-vocabulary log-probability of logprob.hip, read at C columns instead of one (the quality levels' first answer tokens:
// "The quality of the video is <level>.").  Reference arithmetic: modeling_internlm2.py:1095-1096 + log_softmax.
//
// Scoring pass (cand_logprob_kernel): label_logprob_kernel's thread -> chunk mapping and reduction tree for the log-sum-exp, then
// thread c gathers column cand[c].  A row's bits depend on the vocabulary size only - not on the rows, C or the candidates' order.
//
// Decode step: the log-sum-exp comes from the SK_ARGMAX_LSE partials of the lm-head (head.hip) as for `logprob`; the C candidate
// logits come from cand_gemv_kernel, which streams just the C chosen rows of the lm-head weight (16 per workgroup, gathered by id) with
// the skinny kernel's arithmetic: four K slices of K / 4, one MFMA 16x16x32 chain per slice in ascending k, slices summed as
// acc0 + ((p1 + p2) + p3), one bf16 rounding.  An MFMA output element depends on its own A row and B column only, so a column gets the
// bits the lm-head kernel rounds for it whatever slab it sits in there (tests/test_gpu_cand_logprob.py holds the two against each
// other).  Extra weight bytes per step: ceil16(C) x hidden x 2.  lse_finish_cand_kernel is lse_finish_kernel plus the C subtractions.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int CAND_LD = AIGV_MAX_CANDIDATES;   // row stride of the decode step's candidate-logit scratch [R][CAND_LD] bf16

// The four wave pairs -> the row's log-sum-exp, in wave order (the tail of label_logprob_kernel / lse_finish_kernel).  Every calling
// thread runs the same operations on the same values, so all of them hold the same bits.
__device__ __forceinline__ float lse_of_waves(const float* wm, const float* ws) {
  float m = wm[0], s = ws[0];
#pragma unroll
  for (int w = 1; w < LP_THREADS / AIGV_WAVE; ++w) lse_combine(m, s, wm[w], ws[w]);
  return m + logf(s);
}

// VEC as label_logprob_kernel: whole 4-column chunks as one 8-byte load; both forms read the same columns in the same order.
template <bool VEC>
__global__ __launch_bounds__(LP_THREADS) void cand_logprob_kernel(const bf16_t* __restrict__ logits, int V, int ldo,
                                                                  const int64_t* __restrict__ cand, int C, float* __restrict__ out) {
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
  if ((int)threadIdx.x >= C) return;
  const float lse = lse_of_waves(wm, ws);
  const int64_t id = cand[threadIdx.x];
  out[(size_t)r * C + threadIdx.x] = (id < 0 || id >= V) ? __builtin_nanf("") : bf2f(row[id]) - lse;
}

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

// lse_finish_kernel (head.hip) with the candidates: the same slot order and tree for the log-sum-exp, idx / val / logprob from thread 0 as
// there, and thread c < C writes cand_logit[r][c] - lse (NaN for an id outside [0, V)).
__global__ __launch_bounds__(LP_THREADS) void lse_finish_cand_kernel(const unsigned long long* __restrict__ packed, const float2* __restrict__ part,
                                                                    int nslot, int V, const int64_t* __restrict__ cand, int C,
                                                                    const bf16_t* __restrict__ cand_logit, int64_t* __restrict__ idx,
                                                                    float* __restrict__ val, float* __restrict__ logprob,
                                                                    float* __restrict__ cand_logprob) {
  const int r = blockIdx.x;
  const float2* row = part + (size_t)r * nslot;
  float m = -INFINITY, s = 0.f;
  for (int i = threadIdx.x; i < nslot; i += LP_THREADS) {
    const float2 p = row[i];
    lse_combine(m, s, p.x, p.y);
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
  if ((int)threadIdx.x >= C) return;                    // (C >= 1: thread 0 always stays)
  const float lse = lse_of_waves(wm, ws);
  const int64_t id = cand[threadIdx.x];
  cand_logprob[(size_t)r * C + threadIdx.x] = (id < 0 || id >= V) ? __builtin_nanf("") : bf2f(cand_logit[(size_t)r * CAND_LD + threadIdx.x]) - lse;
  if (threadIdx.x != 0) return;
  const unsigned long long p = packed[r];
  unsigned int u = (unsigned)(p >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  const float v = __uint_as_float(u);
  idx[r] = (int64_t)(0xFFFFFFFFu - (unsigned)(p & 0xFFFFFFFFull));
  if (val) val[r] = v;
  logprob[r] = v - lse;
}

}  // namespace

hipError_t aigv_launch_cand_logprob(const bf16_t* logits, int rows, int V, int ldo, const int64_t* cand, int C, float* out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!logits || !cand || !out || V < 1 || ldo < V || C < 1 || C > AIGV_MAX_CANDIDATES) return hipErrorInvalidValue;
  const bool vec = ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 7) == 0;
  if (vec) hipLaunchKernelGGL(cand_logprob_kernel<true>, dim3(rows), dim3(LP_THREADS), 0, s, logits, V, ldo, cand, C, out);
  else hipLaunchKernelGGL(cand_logprob_kernel<false>, dim3(rows), dim3(LP_THREADS), 0, s, logits, V, ldo, cand, C, out);
  return hipGetLastError();
}

size_t aigv_cand_logit_elems(int R) { return (size_t)R * CAND_LD; }

hipError_t aigv_launch_lm_head_argmax_cand_logprob(const bf16_t* h, int R, int H, const bf16_t* W, int V, unsigned long long* packed, float2* part,
                                                   const int64_t* cand, int C, bf16_t* cand_logit, int64_t* out_idx, float* out_val,
                                                   float* out_logprob, float* out_cand, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  if (R > 64 || H % 128 || V < 1 || !cand || !cand_logit || !out_cand || !out_idx || !out_logprob || C < 1 || C > AIGV_MAX_CANDIDATES)
    return hipErrorInvalidValue;
  hipError_t e = aigv_launch_lm_head_lse_partials(h, R, H, W, V, packed, part, s);   // the lm-head of aigv_launch_lm_head_argmax_logprob
  if (e != hipSuccess) return e;
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
  hipLaunchKernelGGL(lse_finish_cand_kernel, dim3(R), dim3(LP_THREADS), 0, s, packed, part, (int)aigv_lm_head_lse_slots(V), V, cand, C, cand_logit,
                     out_idx, out_val, out_logprob, out_cand);
  return hipGetLastError();
}
