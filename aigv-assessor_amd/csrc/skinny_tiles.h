// What the two weight-streaming kernels - skinny_kernel (head.hip, bf16) and skinny8_kernel (head8.hip, e4m3) - have in common, stated once:
// the slab geometry, the K-slice combine with the sub-slab fold, the fused RMSNorm's row value, the RoPE / KV-append epilogue and the SwiGLU
// column; and with_int, the host helper that turns a runtime (row tiles, p, K / 2048) into template arguments.  The K loops are NOT here: they
// differ in MFMA, operand width, prefetch shape and where x comes from.
//
// Geometry.  A workgroup = NWV waves = NWV K slices of NS slabs of RS = 16 / P rows of W.  Lane (fr, fq) = (lane & 15, lane >> 4) feeds A row fr /
// B column fr of a 16 x 16 MFMA with quarter fq of every k-step.  P > 1 (sub-slab forms, one x row tile of R <= RS rows): A row m = W row
// (m mod RS) over K sub-range (m / RS), B column n = x row (n mod RS) over sub-range (n / RS), so D[m][n] is a partial product wherever
// m / RS == n / RS and the result is the sum of those P diagonal blocks (SKINNY_COMBINE's fold).  Every lane still loads distinct weight bytes;
// what changes is the GRID: N / RS workgroups of 1 / P the bytes.
//
// The summation order of SKINNY_COMBINE is a bit-level contract: p = 0 is batch-invariant, and the e4m3 path is checked against oracle/fp8.py.
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

// E: elements of a k-step per lane (bf16: 32 / 4 = 8, 16 bytes; e4m3: 128 / 4 = 32 bytes)
template <int EPI, int P, int NS, int E>
struct SkinnySlab {
  static constexpr int RS = 16 / P;                             // W rows per slab (= x rows the form can take)
  static constexpr int STEP = EPI == SK_ROPE_KV ? 64 : 16;      // rows between the workgroup's slabs
  int fr, fq, sr, sp, n0;                                       // sr / sp: this lane's slab row / x row, and its K sub-range (P == 1: fr, 0)
  int kper, kbeg;                                               // the lane's K range; K % (NWV * P * k-step) == 0 checked by the launchers
  // n0 = first W row of the workgroup's slab(s).  SK_ROPE_KV: block = (head slot, RS-dim group), its two slabs are 64 rows apart; SK_SWIGLU:
  // w1 / w3 alternate in 16-row blocks, block = (32-row pair, RS-row group), the slabs 16 rows apart
  __device__ __forceinline__ SkinnySlab(int lane, int wave, int K, int nwv)
      : fr(lane & 15), fq(lane >> 4), sr((lane & 15) % RS), sp((lane & 15) / RS),
        n0(EPI == SK_ROPE_KV ? (int)(blockIdx.x / (64 / RS)) * 128 + (int)(blockIdx.x % (64 / RS)) * RS
           : EPI == SK_SWIGLU ? (int)(blockIdx.x / P) * 32 + (int)(blockIdx.x % P) * RS
                              : blockIdx.x * RS * NS),
        kper(K / (nwv * P)), kbeg((wave * P + sp) * kper) {}
  // the lane's first fragment in row `row` (clamped to `last`) of the operand base[.][ld]; wfrag: in the lane's row of slab s of W [N][ldw]
  template <class T>
  __device__ __forceinline__ const T* frag(const T* base, int row, int last, int ld) const { return base + (size_t)min(row, last) * ld + kbeg + fq * E; }
  template <class T>
  __device__ __forceinline__ const T* wfrag(const T* W, int s, int N, int ldw) const { return frag(W, n0 + s * STEP + sr, N - 1, ldw); }
  __device__ __forceinline__ bool own() const { return P == 1 || (fr < RS && fq < RS / 4); }   // lanes that hold finished sums
  __device__ __forceinline__ int swiglu_col() const { return (int)(blockIdx.x / P) * 16 + (int)(blockIdx.x % P) * RS + 4 * fq; }
};

// Combine the NWV K slices: waves 1 .. NWV - 1 publish through LDS, wave 0 sums in a fixed order - (p0 + p1) + p2 added to its own sums with
// four waves, the left-to-right sum of the seven others added to them with eight - and then folds the P diagonal blocks (sub-range p lives in
// lanes fr = p RS + i, fq = p RS / 4 + j / 4), in order.  The other waves return from the kernel.  ACC: f32x4 [NS][RT]; PART: __shared__ float
// [NWV - 1][NS][RT][4][64].  A macro, not a function: through a function that takes PART hipcc issues wave 0's LDS reads in another order in
// skinny8_kernel's one-slab forms (profiles/skinny_kernels_refactor.txt).
#define SKINNY_COMBINE(ACC, PART, NWV, NS, RT, P, wave, lane)                                                              \
  if (wave > 0) {                                                                                                          \
    _Pragma("unroll") for (int s = 0; s < NS; ++s)                                                                         \
      _Pragma("unroll") for (int t = 0; t < RT; ++t)                                                                       \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) PART[wave - 1][s][t][e][lane] = ACC[s][t][e];                        \
  }                                                                                                                        \
  __syncthreads();                                                                                                         \
  if (wave != 0) return;                                                                                                   \
  _Pragma("unroll") for (int s = 0; s < NS; ++s)                                                                           \
    _Pragma("unroll") for (int t = 0; t < RT; ++t)                                                                         \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                      \
        if constexpr (NWV == 4) {                                                                                          \
          ACC[s][t][e] += (PART[0][s][t][e][lane] + PART[1][s][t][e][lane]) + PART[2][s][t][e][lane];                      \
        } else {                                                                                                           \
          float sum = 0.f;                                                                                                 \
          _Pragma("unroll") for (int w = 0; w < NWV - 1; ++w) sum += PART[w][s][t][e][lane]; /* fixed order */             \
          ACC[s][t][e] += sum;                                                                                             \
        }                                                                                                                  \
      }                                                                                                                    \
  if constexpr (P == 2) {                                                                                                  \
    _Pragma("unroll") for (int s = 0; s < NS; ++s)                                                                         \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) ACC[s][0][e] += __shfl(ACC[s][0][e], (lane + 40) & 63, 64);            \
  } else if constexpr (P == 4) {                                                                                           \
    _Pragma("unroll") for (int s = 0; s < NS; ++s)                                                                         \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                      \
        const float v = ACC[s][0][e];                                                                                      \
        ACC[s][0][e] = ((v + __shfl(v, (lane + 20) & 63, 64)) + __shfl(v, (lane + 40) & 63, 64)) + __shfl(v, (lane + 60) & 63, 64); \
      }                                                                                                                    \
  }

// The fused RMSNorm (attention_norm before wqkv, ffn_norm before w1|w3; modeling_internlm2.py:138-143) on a row of K = NC x 2048 elements by 256
// threads, with rmsnorm_kernel's arithmetic (rowops.hip): thread t holds the 8-element chunks at skinny_chunk(c), c = 0 .. NC - 1, the sum of
// squares goes through block_sum_256, and an element is gw * bf16(x * rstd) - skinny_normed, to be rounded to bf16 by the caller.  (The sum of
// squares itself stands in both kernel bodies: handing the chunk array to a function re-schedules skinny_kernel's fused-norm forms.)
__device__ __forceinline__ int skinny_chunk(int c) { return (threadIdx.x + c * 256) << 3; }

__device__ __forceinline__ float skinny_normed(bf16_t gw, bf16_t x, float rstd) { return bf2f(gw) * rbf(bf2f(x) * rstd); }

// SK_ROPE_KV: the decode step's wqkv GEMV with RoPE and the KV-cache append in its epilogue (head_dim 128).  A workgroup takes the two RS-row
// slabs of W that rotate_half pairs - dims d .. and 64 + d .. of one head slot - so a lane ends up holding x_i (lo) and x_{i+64} (hi) of the same
// token r: query slots are rotated and stored to the qkv row, the K slot is rotated and the V slot copied straight into the caches
// (modeling_internlm2.py:247-261, 397-402; the same three bf16 roundings as rope_kernel).
// LO / HI: the two slabs' f32x4 sums of x row r.  A macro like SKINNY_COMBINE: as a function it re-schedules the SK_ROPE_KV forms of both kernels
// (2 VGPRs fewer at two to four row tiles, about 180 other instructions per decode form), and the decode step measured 0.4 % slower with it.
#define SKINNY_ROPE_KV_STORE(RS, LO, HI, rk, r, fq, out, ldo)                                                                               \
  {                                                                                                                                         \
    const int hs = blockIdx.x / (64 / RS), d = (int)(blockIdx.x % (64 / RS)) * RS + 4 * fq; /* head slot; dims d .. d+3 and d+64 .. d+67 */ \
    const int slot = hs % (rk.g + 2), gi = hs / (rk.g + 2);                                                                                 \
    const int p = rk.pos[r];                                                                                                                \
    u16x4 olo, ohi;                                                                                                                         \
    if (slot <= rk.g) {                                                                                                                     \
      const u16x4 co = *(const u16x4*)(rk.cos + (size_t)p * 64 + d), si = *(const u16x4*)(rk.sin + (size_t)p * 64 + d);                     \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                                       \
        const float x1 = rbf(LO[e]), x2 = rbf(HI[e]), cc = bf2f(co[e]), ss = bf2f(si[e]);                                                   \
        olo[e] = f2bf(rbf(x1 * cc) + rbf(-x2 * ss));                                                                                        \
        ohi[e] = f2bf(rbf(x2 * cc) + rbf(x1 * ss));                                                                                         \
      }                                                                                                                                     \
    } else {                                                                                                                                \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) { olo[e] = f2bf(LO[e]); ohi[e] = f2bf(HI[e]); }                                         \
    }                                                                                                                                       \
    bf16_t* dst = slot < rk.g ? out + (size_t)r * ldo + (size_t)hs * 128 + d                                                                \
                              : (slot == rk.g ? rk.kc : rk.vc) + (((size_t)rk.seq[r] * rk.n_kv + gi) * rk.cap + p) * 128 + d;               \
    *(u16x4*)dst = olo;                                                                                                                     \
    *(u16x4*)(dst + 64) = ohi;                                                                                                              \
  }

// with_int<V0, V1, ...>(v, f) calls f(std::integral_constant<int, Vi>{}) for the Vi that equals v - only the listed values are ever instantiated -
// and returns hipErrorInvalidValue if none does (with_epi's manner, epilogue.h)
template <int V0, int... Vs, class F>
inline hipError_t with_int(int v, F&& f) {
  if (v == V0) return f(std::integral_constant<int, V0>{});
  if constexpr (sizeof...(Vs) > 0) return with_int<Vs...>(v, f);
  else return hipErrorInvalidValue;
}
template <int V>
using int_c = std::integral_constant<int, V>;
