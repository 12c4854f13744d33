// Skinny (<= 64 rows) weight-streaming GEMM for gfx950, used where the weights are read once per call and the
// kernel is HBM-bound:  the lm-head on the answer rows with a fused vocabulary argmax
// (reference: modeling_internlm2.py:1094-1096 + modeling_internvl_chat.py:451-463,488), the q_len = 1 decode
// steps of generate() (modeling_internlm2.py:1126-1163), the motion projector (M = clips), and the score head
// (modeling_internvl_chat.py:43-94).
//
// One workgroup = 4 waves = one 16-row slab of W (two slabs for SwiGLU); the waves split K four ways, stream
// their W fragments straight from global memory into MFMA A-operands (no LDS round trip: every weight byte
// is used once), keep the x fragments (L2-resident) as B-operands, and combine partial sums through LDS.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "epilogue.h"
#include "kernels.h"
#include "skinny_tiles.h"

namespace {

#ifndef SKINNY_DEPTH2
#define SKINNY_DEPTH2 8      // k-steps in flight of the two-slab one-row-tile forms (SwiGLU w1|w3, RoPE wqkv)
#endif

// SK_ARGMAX_LSE: SK_ARGMAX plus the log-sum-exp of every row (generate()'s per-token log-probabilities, modeling_internlm2.py:1095-1096 +
// log_softmax).  The argmax key is SK_ARGMAX's, bit for bit.  Besides it, every 16-column slab of W writes the (max, sum of exp(x - max))
// pair of its bf16-rounded logits to its own slot of a partials buffer [R][ceil(N / 16)] - passed as `out`, `ldo` = ceil(N / 16) float2
// per row - with no atomics: lane fq holds columns 4 fq .. 4 fq + 3 of the slab, pushed in column order, then two butterfly steps.  The
// slot layout follows the 16-row slabs, not the workgroups (one or four slabs per workgroup depending on R), so a row's partials do
// not depend on R; lse_finish_kernel (logprob.hip) merges them in a fixed order.
// (lse_push / lse_combine: common.h)

// NORM: the GEMV applies the RMSNorm in front of it (attention_norm before wqkv, ffn_norm before w1|w3; modeling_internlm2.py:138-143)
// to its x rows itself: x is the raw residual stream, every workgroup normalises the R <= 4 rows into LDS with rmsnorm_kernel's exact
// arithmetic (skinny_tiles.h) and takes its B fragments from there.  Redundant work per
// workgroup (R x K elements), but no launch: the statistics' L2 round trip and barriers run behind the first weight loads.
struct NormArgs { const bf16_t* w; float eps; };

// SK_ARGMAX_LSE_STORE: SK_ARGMAX_LSE that also keeps the bf16-rounded logits it reduces, for the top-k selection behind the finisher
// (topk_of_row, logprob.hip): a lane holds 4 consecutive columns of a slab, so each (row, slab) costs one 8-byte store into
// st.p[R][st.ld] - st.ld a multiple of 4 >= N and st.p 8-byte aligned (the launcher checks).  Key and partials are SK_ARGMAX_LSE's bits.
struct LogitStore { bf16_t* p; int ld; };

// NWV: waves per workgroup = K slices.  8 for the decode GEMVs whose N gives at most one workgroup per CU (wo, w2: 256 slabs of 16
// rows): twice the loads in flight per CU, which is what bounds a weight stream at this occupancy (in-box A/B, scripts/decode_gemv_bench.py:
// wo 7.9 -> 7.5 us, w2 26.6 -> 24.8 us = 4.7 TB/s; wqkv with 384 slabs is faster with 4 waves, 12.5 vs 13.2 us).
// NT: the weight fragments are loaded non-temporally (each byte is used once: no point in keeping it in L2 / Infinity Cache, and a
// once-read stream lands sooner with the nt policy - MI355X_MICROARCH.md 'nt-weights').
template <bool NT>
__device__ __forceinline__ bf16x8 wload(const bf16_t* p) {
  if constexpr (NT) return __builtin_nontemporal_load((const bf16x8*)p);
  else return *(const bf16x8*)p;
}

// P: sub-slab form of a decode GEMV (one x row tile, R <= 16 / P rows; geometry: skinny_tiles.h).  A width whose 16-row slabs come to a
// non-integer number of workgroups per CU (w1|w3 of InternLM2-7B: 3.5; fused wqkv: 0.75) runs at the rate of the next integer
// (scripts/gemv_balance_probe.py: 3.5 per CU 4.97 TB/s, 3 per CU 5.34, 4 per CU 5.45).
template <int RT, int EPI, int NWV = 4, bool NT = false, int NC = 0, int P = 1>   // NC: fused-norm form, K = NC x 2048 (0 = off)
__global__ __launch_bounds__(NWV * 64) void skinny_kernel(const bf16_t* __restrict__ x, int ldx, int R,
                                                     const bf16_t* __restrict__ W, int ldw, int N, int K,
                                                     const bf16_t* __restrict__ bias, const bf16_t* __restrict__ resid,
                                                     int ldr, bf16_t* __restrict__ out, int ldo,
                                                     unsigned long long* __restrict__ packed,
                                                     const bf16_t* __restrict__ ls, const AigvRopeKv rk = AigvRopeKv{},
                                                     const NormArgs na = NormArgs{}, const LogitStore st = LogitStore{}) {
  constexpr bool NORM = NC > 0;
  static_assert(!NORM || (RT == 1 && NWV == 4), "the fused norm is the decode form: one row tile, 256 threads (rmsnorm_kernel's reduction)");
  extern __shared__ __attribute__((aligned(16))) bf16_t xs[];   // NORM: the normalised x rows [R][K]
  // W slabs (16 rows each) per workgroup.  The lm-head on the answer rows (40+ x rows) is bound by re-reading the x fragments
  // from L2 once per workgroup, not by streaming W: four slabs per workgroup share them.
  constexpr bool AMAX = EPI == SK_ARGMAX || EPI == SK_ARGMAX_LSE || EPI == SK_ARGMAX_LSE_STORE;
  constexpr int NS = (EPI == SK_SWIGLU || EPI == SK_ROPE_KV) ? 2 : (AMAX && RT >= 2) ? 4 : 1;
  static_assert(P == 1 || ((P == 2 || P == 4) && RT == 1 && !AMAX), "sub-slab forms: one row tile, 8 or 4 rows per slab");
  __shared__ float part[NWV - 1][NS][RT][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const SkinnySlab<EPI, P, NS, 8> g(lane, wave, K, NWV);
  constexpr int RS = g.RS;
  const int fq = g.fq, n0 = g.n0, kper = g.kper;

  const bf16_t* wrow[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) wrow[s] = g.wfrag(W, s, N, ldw);
  const bf16_t* xrow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) xrow[t] = g.frag(x, t * 16 + g.sr, R - 1, ldx);

  f32x4 acc[NS][RT];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int t = 0; t < RT; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // DEPTH k-steps (DEPTH x 16 B per lane per operand) are loaded before their MFMAs so several loads are in flight; a decode
  // GEMV (one x row tile, few workgroups per CU when N is small) needs the deeper form to cover the HBM latency
  constexpr int DEPTH = RT == 1 ? (NS == 1 ? 16 : SKINNY_DEPTH2) : (RT == 2 && NS == 1) ? 8 : 4;   // (two row tiles: InternViT's 32 leftover rows per pass)
  int k = 0;
  const int xs_off = min(g.sr, R - 1) * K + g.kbeg + fq * 8;         // NORM: this lane's fragment origin in xs
  if constexpr (NORM) {
    // Load order matters (vmcnt retires in issue order): the x rows and the norm weight - a few L2 hits - go out FIRST, then the
    // first DEPTH weight k-steps; the statistics then wait only for the former, with the weight stream in flight behind them.
    // Rows past R repeat row R - 1 (never normalised).
    u16x8 xr[4][NC], gw[NC];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) xr[r][c] = *(const u16x8*)(x + (size_t)min(r, R - 1) * ldx + skinny_chunk(c));
#pragma unroll
    for (int c = 0; c < NC; ++c) gw[c] = *(const u16x8*)(na.w + skinny_chunk(c));
    bf16x8 wf[DEPTH][NS];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u)
#pragma unroll
      for (int s = 0; s < NS; ++s) wf[u][s] = wload<NT>(wrow[s] + 32 * u);
    {
      __shared__ float red[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r == 0 || r < R) {     // (row 0 unconditionally: hipcc otherwise sinks the norm-weight loads into the branch, behind the weight stream)
          float sq = 0.f;
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float v = bf2f(xr[r][c][e]); sq += v * v; }
          const float rstd = rsqrtf(block_sum_256(sq, red) / (float)K + na.eps);
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(skinny_normed(gw[c][e], xr[r][c][e], rstd));
            *(u16x8*)(xs + (size_t)r * K + skinny_chunk(c)) = o;
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const bf16x8 xf = *(const bf16x8*)(xs + xs_off + 32 * u);
#pragma unroll
      for (int s = 0; s < NS; ++s) acc[s][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][s], xf, acc[s][0], 0, 0, 0);
    }
    k = 32 * DEPTH;
  }
  // the rest of the K slice in groups of DEPTH, then 8 / 4 / 1 k-steps: a slice that is not a multiple of DEPTH (K = 14336 over 8
  // waves: 56 k-steps) used to finish one load at a time
  auto run = [&](auto dtag) {
    constexpr int DD = decltype(dtag)::value;
    for (; k + 32 * DD <= kper; k += 32 * DD) {
      bf16x8 wf[DD][NS], xf[DD][RT];
#pragma unroll
      for (int u = 0; u < DD; ++u) {
#pragma unroll
        for (int s = 0; s < NS; ++s) wf[u][s] = wload<NT>(wrow[s] + k + 32 * u);
#pragma unroll
        for (int t = 0; t < RT; ++t) {
          if constexpr (NORM) xf[u][t] = *(const bf16x8*)(xs + xs_off + k + 32 * u);
          else xf[u][t] = *(const bf16x8*)(xrow[t] + k + 32 * u);
        }
      }
#pragma unroll
      for (int u = 0; u < DD; ++u)
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
          for (int t = 0; t < RT; ++t)
            acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][s], xf[u][t], acc[s][t], 0, 0, 0);
    }
  };
  run(std::integral_constant<int, DEPTH>{});
  if constexpr (DEPTH > 8) run(std::integral_constant<int, 8>{});
  if constexpr (DEPTH > 4) run(std::integral_constant<int, 4>{});
  run(std::integral_constant<int, 1>{});

  SKINNY_COMBINE(acc, part, NWV, NS, RT, P, wave, lane)       // K slices and sub-slab blocks, fixed order (skinny_tiles.h)
  const bool own = g.own();

  // lane owns x row r = 16t + fr and W rows n = n0 + 4*fq + e
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int r = own ? t * 16 + g.fr : R;
    if constexpr (AMAX) {
      unsigned long long best = 0ull;
#pragma unroll
      for (int sl = 0; sl < NS; ++sl)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int n = n0 + sl * 16 + 4 * fq + e;
          if (n < N) {
            const unsigned long long key = ((unsigned long long)ord_f32(rbf(acc[sl][t][e])) << 32) | (0xFFFFFFFFu - (unsigned)n);
            best = key > best ? key : best;
          }
        }
      unsigned long long o = __shfl_xor(best, 16, 64); best = o > best ? o : best;
      o = __shfl_xor(best, 32, 64); best = o > best ? o : best;
      if (fq == 0 && r < R) atomicMax(packed + r, best);
      if constexpr (EPI == SK_ARGMAX_LSE || EPI == SK_ARGMAX_LSE_STORE) {
        float2* part = reinterpret_cast<float2*>(out);
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
          const int ns0 = n0 + sl * 16;            // the slab's first column (slot ns0 / 16)
          float m = -INFINITY, sum = 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) lse_push(m, sum, ns0 + 4 * fq + e < N ? rbf(acc[sl][t][e]) : -INFINITY);
          lse_combine(m, sum, __shfl_xor(m, 16, 64), __shfl_xor(sum, 16, 64));
          lse_combine(m, sum, __shfl_xor(m, 32, 64), __shfl_xor(sum, 32, 64));
          if (fq == 0 && r < R && ns0 < N) part[(size_t)r * ldo + ns0 / 16] = make_float2(m, sum);
          if constexpr (EPI == SK_ARGMAX_LSE_STORE) {
            if (r < R && ns0 + 4 * fq < N) {      // columns >= N of the last group are padding inside st.ld
              u16x4 o;
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[sl][t][e]);
              *(u16x4*)(st.p + (size_t)r * st.ld + ns0 + 4 * fq) = o;
            }
          }
        }
      }
    } else if constexpr (EPI == SK_ROPE_KV) {
      if (r < R) SKINNY_ROPE_KV_STORE(RS, acc[0][t], acc[1][t], rk, r, fq, out, ldo)
    } else if constexpr (EPI == SK_SWIGLU) {
      if (r < R) *(u16x4*)(out + (size_t)r * ldo + g.swiglu_col()) = epi_swiglu4(acc[0][t], acc[1][t]);
    } else {
      const int n = n0 + 4 * fq;
      if (r < R && n < N) {
        // This kernel's own text of epilogue.h's linear chain (epi_acc4 then epi_row4 for SK_STORE / _GELU / _LS_RESID / _RESID, with a zero added where
        // there is no bias; SK_RELU is the score head's).  Through the shared functions three of the 3- and 4-row-tile residual forms take two more
        // VGPRs and one of them loses a wave of occupancy (profiles/gemm_epilogue_kernel_resources.txt), so the text stays; scripts/gemm_epilogue_bits.py
        // and test_gelu_and_swiglu_bits_agree_on_every_route hold it in step with the other kernels.
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[0][t][e] + (bias ? bf2f(bias[n + e]) : 0.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
        if constexpr (EPI == SK_GELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rbf(gelu_fast(v[e]));
        }
        if constexpr (EPI == SK_RELU) {   // a NaN stays a NaN, as through F.relu (fmaxf would return the 0)
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];
        }
        if constexpr (EPI == SK_LS_RESID) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] * bf2f(ls[n + e]));
        }
        if constexpr (EPI == SK_RESID || EPI == SK_LS_RESID) {
          const u16x4 rr = *(const u16x4*)(resid + (size_t)r * ldr + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rbf(bf2f(rr[e]) + v[e]);
        }
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
        *(u16x4*)(out + (size_t)r * ldo + n) = o;
      }
    }
  }
}

__global__ void unpack_argmax_kernel(const unsigned long long* __restrict__ packed, int64_t* __restrict__ idx,
                                     float* __restrict__ val, int R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  float v;
  unpack_argmax_key(packed[r], idx[r], v);
  if (val) val[r] = v;
}

// ---- score head ------------------------------------------------------------------------------------------
// x = hidden[:, -4, :] (post final norm); if ANY NaN is present in the batch slice the reference applies
// nan_to_num(nan=0, posinf=1e9, neginf=-1e9) to every row (modeling_internvl_chat.py:469-473); then a chain
// of Linear+ReLU with a bf16 rounding after each Linear (:82-94).  Without a NaN the guard leaves an Inf alone: the row then turns
// into NaN / Inf in the Linears, and the ReLUs pass a NaN on as F.relu does.  The wide layers run on the skinny GEMM
// (weights streamed once for all clips); the narrow tail (fan-in < 128) runs in one small kernel.
// The guard: workgroup g guards ITS batch slice - the B rows at x + g * group_stride, leading dimension ldx - under its own flag, as the reference
// would guard G batch slices one after the other; out is dense [G * B, H].  (aigv_launch_score_head: G = 1)
__global__ __launch_bounds__(256) void score_guard_groups_kernel(const bf16_t* __restrict__ x, int ldx, size_t group_stride, int B, int H,
                                                                 bf16_t* __restrict__ out) {
  const bf16_t* xg = x + (size_t)blockIdx.x * group_stride;
  bf16_t* og = out + (size_t)blockIdx.x * B * H;
  __shared__ int any_nan;
  if (threadIdx.x == 0) any_nan = 0;
  __syncthreads();
  int nan_here = 0;
  for (int i = threadIdx.x; i < B * H; i += 256) {
    const float v = bf2f(xg[(size_t)(i / H) * ldx + (i % H)]);
    nan_here |= (v != v);
  }
  if (nan_here) atomicOr(&any_nan, 1);
  __syncthreads();
  const bool fix = any_nan != 0;
  for (int i = threadIdx.x; i < B * H; i += 256) {
    float v = bf2f(xg[(size_t)(i / H) * ldx + (i % H)]);
    if (fix) {
      if (v != v) v = 0.f;
      else if (isinf(v)) v = v > 0 ? 1e9f : -1e9f;
    }
    og[i] = f2bf(v);
  }
}

// remaining narrow layers: one workgroup per clip; activations ping-pong in LDS (all dims <= 1024 here)
__global__ __launch_bounds__(256) void score_tail_kernel(const ScoreHeadArgs a, int first_layer) {
  __shared__ float buf[2][1024];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d0 = a.dims[first_layer];
  for (int i = threadIdx.x; i < d0; i += 256) buf[0][i] = bf2f(a.x[(size_t)b * a.ldx + i]);
  __syncthreads();
  int cur = 0;
  for (int L = first_layer; L < a.n_layers; ++L) {
    const int din = a.dims[L], dout = a.dims[L + 1];
    const bf16_t* w = a.w[L];
    const bf16_t* bb = a.b[L];
    for (int o = wave; o < dout; o += 4) {
      float s = 0.f;
      for (int i = lane; i < din; i += 64) s += bf2f(w[(size_t)o * din + i]) * buf[cur][i];
      s = wave_sum(s);
      const float y = rbf(s + bf2f(bb[o]));
      if (lane == 0) buf[cur ^ 1][o] = y < 0.f ? 0.f : y;   // ReLU that keeps a NaN (F.relu does; fmaxf would not)
    }
    __syncthreads();
    cur ^= 1;
  }
  if (threadIdx.x == 0) a.score[b] = buf[cur][0];
}

template <int EPI>
hipError_t launch_skinny(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, const bf16_t* bias,
                         const bf16_t* resid, int ldr, bf16_t* out, int ldo, unsigned long long* packed,
                         hipStream_t s, const bf16_t* ls = nullptr, int p = 1, LogitStore st = LogitStore{}) {
  const int rt = (R + 15) / 16;
  auto go = [&](auto rtag, auto wtag, auto ptag, int blocks) {
    constexpr int RT = decltype(rtag)::value, NWV = decltype(wtag)::value, P = decltype(ptag)::value;
    hipLaunchKernelGGL((skinny_kernel<RT, EPI, NWV, false, 0, P>), dim3(blocks), dim3(NWV * 64), 0, s, x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, packed, ls,
                       AigvRopeKv{}, NormArgs{}, st);
    return hipGetLastError();
  };
  if (p > 1) {   // sub-slab forms of the decode GEMVs (skinny_kernel's P): 16 / p rows per workgroup and slab
    const int rs = 16 / p;
    if ((p != 2 && p != 4) || R > rs || K % (128 * p) || N % (EPI == SK_SWIGLU ? 32 : rs)) return hipErrorInvalidValue;
    if constexpr (EPI == SK_STORE || EPI == SK_RESID || EPI == SK_SWIGLU)
      return with_int<2, 4>(p, [&](auto pp) { return go(int_c<1>{}, int_c<4>{}, pp, EPI == SK_SWIGLU ? N / 32 * p : N / rs); });
    else
      return hipErrorInvalidValue;
  }
  const int ns = (EPI == SK_SWIGLU) ? 2 : ((EPI == SK_ARGMAX || EPI == SK_ARGMAX_LSE || EPI == SK_ARGMAX_LSE_STORE) && rt >= 2) ? 4 : 1;   // = NS of the kernel
  const int blocks = (N + 16 * ns - 1) / (16 * ns);
  // (non-temporal weight loads were measured SLOWER on the 8B decode shapes - wqkv 12.5 -> 14.8 us, w2 24.9 -> 29.9 us, w1|w3 47.9 -> 54.9 us -
  //  and the form was removed: plain cache policy everywhere)
  if constexpr (EPI == SK_STORE || EPI == SK_RESID) {
    constexpr int max8 = 256;   // at most one slab per CU
    // a decode GEMV with about one slab per CU: 8 K slices per workgroup (p == 0: the caller wants ONE form for every row count)
    if (rt == 1 && K % 256 == 0 && blocks <= max8 && p != 0) return go(int_c<1>{}, int_c<8>{}, int_c<1>{}, blocks);
  }
  return with_int<1, 2, 3, 4>(rt, [&](auto t) { return go(t, int_c<4>{}, int_c<1>{}, blocks); });
}

}  // namespace

// widths the fused-norm GEMVs are built for (K = 2 x 2048: InternLM2-7B, 3 x 2048: InternLM2-20B)
bool aigv_skinny_norm_fusable(int K) { return K == 4096 || K == 6144; }

// the decode step's wqkv projection with RoPE + KV-cache append in the epilogue (SK_ROPE_KV above); x rows = one new token per sequence
hipError_t aigv_launch_skinny_rope_kv(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, bf16_t* qkv, int ldo,
                                      const int32_t* pos, const int32_t* seq, const bf16_t* cos, const bf16_t* sin, bf16_t* kc, bf16_t* vc,
                                      int g, int n_kv, int cap, int head_dim, hipStream_t s, const bf16_t* norm_w, float norm_eps, int p) {
  if (R <= 0) return hipSuccess;
  if (R > 64 || K % 128 || (ldx % 8) || (ldw % 8) || (ldo % 4) || head_dim != 128 || N != n_kv * (g + 2) * 128 || !pos || !seq || !cos ||
      !sin || !kc || !vc)
    return hipErrorInvalidValue;
  const AigvRopeKv rk{pos, seq, cos, sin, kc, vc, g, n_kv, cap};
  const int rt = (R + 15) / 16, blocks = N / 32 * p;
  if ((p != 1 && p != 2 && p != 4) || R > (p == 1 ? 64 : 16 / p) || K % (128 * p)) return hipErrorInvalidValue;
  auto go = [&](auto rtag, auto nctag, auto ptag) {   // NC > 0: x = the raw residual rows; attention_norm applied by the kernel (NormArgs above)
    constexpr int RT = decltype(rtag)::value, NC = decltype(nctag)::value, P = decltype(ptag)::value;
    hipLaunchKernelGGL((skinny_kernel<RT, SK_ROPE_KV, 4, false, NC, P>), dim3(blocks), dim3(256), NC ? (size_t)R * K * sizeof(bf16_t) : 0, s, x, ldx, R, W, ldw, N, K,
                       nullptr, nullptr, 0, qkv, ldo, nullptr, nullptr, rk, NormArgs{norm_w, norm_eps});
    return hipGetLastError();
  };
  if (norm_w) {
    if (R > 4 || !aigv_skinny_norm_fusable(K)) return hipErrorInvalidValue;
    return with_int<2, 3>(K / 2048, [&](auto nc) { return with_int<1, 2, 4>(p, [&](auto pp) { return go(int_c<1>{}, nc, pp); }); });
  }
  if (p != 1) return with_int<2, 4>(p, [&](auto pp) { return go(int_c<1>{}, int_c<0>{}, pp); });
  return with_int<1, 2, 3, 4>(rt, [&](auto t) { return go(t, int_c<0>{}, int_c<1>{}); });
}

// decode: SwiGLU(x_n W13^T) with x_n = RMSNorm(x) * norm_w computed by the kernel itself (R <= 4 rows; NormArgs above)
hipError_t aigv_launch_skinny_swiglu_normed(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K, bf16_t* out, int ldo,
                                            const bf16_t* norm_w, float norm_eps, hipStream_t s, int p) {
  if (R <= 0) return hipSuccess;
  if (R > 4 || !aigv_skinny_norm_fusable(K) || (ldx % 8) || (ldw % 8) || (ldo % 4) || (N % 32) || !norm_w || (p != 1 && p != 2 && p != 4)) return hipErrorInvalidValue;
  return with_int<2, 3>(K / 2048, [&](auto nc) {
    return with_int<1, 2, 4>(p, [&](auto pp) {
      hipLaunchKernelGGL((skinny_kernel<1, SK_SWIGLU, 4, false, decltype(nc)::value, decltype(pp)::value>), dim3(N / 32 * p), dim3(256), (size_t)R * K * sizeof(bf16_t), s,
                         x, ldx, R, W, ldw, N, K, nullptr, nullptr, 0, out, ldo, nullptr, nullptr, AigvRopeKv{}, NormArgs{norm_w, norm_eps});
      return hipGetLastError();
    });
  });
}

// epi: 0 store(+bias) | 1 residual(+bias) | 2 swiglu (16-row interleaved w1/w3, out is N/2 wide) | 3 gelu(+bias)
//      6 layer-scale + residual (+bias)
hipError_t aigv_launch_skinny_gemm(const bf16_t* x, int ldx, int R, const bf16_t* W, int ldw, int N, int K,
                                   const bf16_t* bias, const bf16_t* resid, int ldr, bf16_t* out, int ldo, int epi,
                                   hipStream_t s, const bf16_t* ls, int p) {
  if (R <= 0) return hipSuccess;
  if (R > 64 || K % 128 || (ldx % 8) || (ldw % 8) || (ldo % 4)) return hipErrorInvalidValue;
  if (epi != SK_SWIGLU && N % 4) return hipErrorInvalidValue;
  if (epi == SK_SWIGLU && N % 32) return hipErrorInvalidValue;
  if (p > 1 && epi != SK_STORE && epi != SK_RESID && epi != SK_SWIGLU) return hipErrorInvalidValue;
  switch (epi) {
    case SK_STORE: return launch_skinny<SK_STORE>(x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, nullptr, s, nullptr, p);
    case SK_RESID: return launch_skinny<SK_RESID>(x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, nullptr, s, nullptr, p);
    case SK_SWIGLU: return launch_skinny<SK_SWIGLU>(x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, nullptr, s, nullptr, p);
    case SK_GELU: return launch_skinny<SK_GELU>(x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, nullptr, s);
    case SK_LS_RESID:
      if (!ls || !resid) return hipErrorInvalidValue;
      return launch_skinny<SK_LS_RESID>(x, ldx, R, W, ldw, N, K, bias, resid, ldr, out, ldo, nullptr, s, ls);
  }
  return hipErrorInvalidValue;
}

// lm-head logits of R rows as the reference holds them before its .float(): the bf16 output of the matmul (modeling_internlm2.py:
// 1095-1096).  out is [R, ldo] bf16 with ldo >= V rounded up to 4 (the store epilogue writes 4 columns per lane; columns >= V of a
// row are padding).  Used where the whole distribution is needed - sampling in generate() - the greedy paths use the fused argmax.
hipError_t aigv_launch_lm_head_logits(const bf16_t* h, int R, int H, const bf16_t* W, int V, bf16_t* out, int ldo, hipStream_t s,
                                      bool one_form, int ldh) {
  if (R <= 0) return hipSuccess;
  if (ldh == 0) ldh = H;
  if (R > 64 || H % 128 || ldo < ((V + 3) / 4) * 4 || (ldo % 4) || ldh < H || ldh % 8) return hipErrorInvalidValue;
  return launch_skinny<SK_STORE>(h, ldh, R, W, H, V, H, nullptr, nullptr, 0, out, ldo, nullptr, s, nullptr, one_form ? 0 : 1);
}

hipError_t aigv_launch_lm_head_argmax(const bf16_t* h, int R, int H, const bf16_t* W, int V,
                                      unsigned long long* packed, int64_t* out_idx, float* out_val, hipStream_t s) {
  if (R <= 0) return hipSuccess;
  if (R > 64 || H % 128) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(packed, 0, sizeof(unsigned long long) * R, s);
  if (e != hipSuccess) return e;
  e = launch_skinny<SK_ARGMAX>(h, H, R, W, H, V, H, nullptr, nullptr, 0, nullptr, 0, packed, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unpack_argmax_kernel, dim3((R + 63) / 64), dim3(64), 0, s, packed, out_idx, out_val, R);
  return hipGetLastError();
}

size_t aigv_lm_head_lse_slots(int V) { return (size_t)(V + 15) / 16; }

// the lm-head in its SK_ARGMAX_LSE form alone: the packed argmax keys and the per-slab log-sum-exp partials, for lse_finish_kernel (logprob.hip) to read
// logits != nullptr: the SK_ARGMAX_LSE_STORE form - the same keys and partials, and the bf16 logits themselves into logits[R][ldl]
hipError_t aigv_launch_lm_head_lse_partials(const bf16_t* h, int R, int H, const bf16_t* W, int V, unsigned long long* packed, float2* part,
                                            hipStream_t s, bf16_t* logits, int ldl) {
  if (R <= 0) return hipSuccess;
  if (R > 64 || H % 128 || V < 1 || !packed || !part) return hipErrorInvalidValue;
  if (logits && (ldl % 4 || ldl < (V + 3) / 4 * 4 || (reinterpret_cast<uintptr_t>(logits) & 7))) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(packed, 0, sizeof(unsigned long long) * R, s);
  if (e != hipSuccess) return e;
  if (logits)
    return launch_skinny<SK_ARGMAX_LSE_STORE>(h, H, R, W, H, V, H, nullptr, nullptr, 0, reinterpret_cast<bf16_t*>(part), (int)aigv_lm_head_lse_slots(V), packed, s,
                                              nullptr, 1, LogitStore{logits, ldl});
  return launch_skinny<SK_ARGMAX_LSE>(h, H, R, W, H, V, H, nullptr, nullptr, 0, reinterpret_cast<bf16_t*>(part), (int)aigv_lm_head_lse_slots(V), packed, s);
}

// G batch slices of B rows each in one go (the depth lens: one slice per depth): slice g = rows x + g * group_stride (leading dimension
// a.ldx), guarded on its own; the GEMM layers then run over all G * B rows in chunks of at most 64 - a row's bits do not depend on how many
// rows share its launch - and the tail kernel over all of them.  a.score: [G * B].  scratch: 3 * G * B * max(dims) bf16 (guarded input + two
// ping-pong activations).
hipError_t aigv_launch_score_head_groups(const ScoreHeadArgs& a, int G, size_t group_stride, bf16_t* scratch, hipStream_t s) {
  if (a.B <= 0 || G <= 0) return hipSuccess;
  if (a.n_layers < 1 || a.n_layers > 8 || a.B > 64 || !scratch) return hipErrorInvalidValue;
  int maxd = 0;
  for (int i = 0; i <= a.n_layers; ++i) {
    if (a.dims[i] <= 0) return hipErrorInvalidValue;
    maxd = a.dims[i] > maxd ? a.dims[i] : maxd;
  }
  int L = 0;
  while (L < a.n_layers && a.dims[L] % 128 == 0 && a.dims[L + 1] % 4 == 0) ++L;
  if (L == a.n_layers) return hipErrorInvalidValue;   // the last layer (fan-out 1) always runs in the tail kernel
  for (int i = L; i <= a.n_layers; ++i)
    if (a.dims[i] > 1024) return hipErrorInvalidValue;
  const int rows = G * a.B;
  bf16_t* xg = scratch;
  bf16_t* pp[2] = {scratch + (size_t)rows * maxd, scratch + (size_t)2 * rows * maxd};
  hipLaunchKernelGGL(score_guard_groups_kernel, dim3(G), dim3(256), 0, s, a.x, a.ldx, group_stride, a.B, a.dims[0], xg);
  const bf16_t* cur = xg;
  int ld = a.dims[0], flip = 0;
  for (int l = 0; l < L; ++l) {
    const int din = a.dims[l], dout = a.dims[l + 1];
    for (int r0 = 0; r0 < rows; r0 += 64) {
      hipError_t e = launch_skinny<SK_RELU>(cur + (size_t)r0 * ld, ld, std::min(64, rows - r0), a.w[l], din, dout, din, a.b[l], nullptr, 0,
                                            pp[flip] + (size_t)r0 * dout, dout, nullptr, s);
      if (e != hipSuccess) return e;
    }
    cur = pp[flip];
    ld = dout;
    flip ^= 1;
  }
  ScoreHeadArgs t = a;
  t.x = cur;
  t.ldx = ld;
  hipLaunchKernelGGL(score_tail_kernel, dim3(rows), dim3(256), 0, s, t, L);
  return hipGetLastError();
}

// one batch slice: scratch 3 * B * max(dims) bf16.  (A chain without a tail layer, or with a tail dimension above 1024, is refused before anything is launched.)
hipError_t aigv_launch_score_head(const ScoreHeadArgs& a, bf16_t* scratch, hipStream_t s) { return aigv_launch_score_head_groups(a, 1, 0, scratch, s); }
