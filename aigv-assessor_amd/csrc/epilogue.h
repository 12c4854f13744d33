// The GEMM epilogues, stated once.  The dispatcher may send any row of any linear to the 128 tile kernel (gemm.hip), the 256 tile kernel in
// its direct, LDS-staged or residual-prefetch form (gemm256.hip), the co-resident kernel (gemmco.hip), a split-K slice kernel followed by
// gemm_finalize_kernel (gemm.hip), or the weight-streaming kernels (head.hip, head8.hip): they call these functions, so a row's bits do
// not depend on the kernel that computed it - by construction, not because copies of the arithmetic were kept in step.
//
//   linear chain   acc (+ bias) -> bf16 -> [GELU -> bf16 | x ls -> bf16] -> [resid + . -> bf16 | . + pos -> bf16]
//                  `----------------- epi_acc4 / epi_acc2 ---------------'   `----- epi_row / epi_row4 / epi_row2 -----'
//   SwiGLU         bf16(bf16(silu(bf16 g)) * bf16 u)                                            epi_swiglu4 / epi_swiglu2
//
// The accumulator part is a function of the accumulator and of per-column vectors only (what the staged kernels apply before they transpose
// through LDS); the row part needs the output row (residual row, position row).  The rounding points are those of the reference's eager
// bf16 path (gemm.hip's header).  All of them take and return VALUES - the accumulator in fp32, everything else as bf16 bits - never
// pointers: a kernel keeps its addressing, its loads and its staging layout, and where a load must not be visible to the compiler
// (gemm256.hip's residual-prefetch epilogue) it hands over registers an asm statement has written.  An argument the epilogue does not use
// (bias without has_bias, ls unless EPI_LS_RESID) is passed as 0, never as an unwritten register.
//
// Each part comes in a scalar form (gelu_fast / silu_f / rbf) and a packed-pair form (gelu_fast2 / silu2 / rbf2 / pack_bf2: two bf16 in
// a uint32_t, low half first), side by side: per component the same IEEE operations (common.h), so the two forms give the same bits.  The
// fp8 kernels apply (acc * row scale) * column scale first and pass the product as `acc`.
//
// Two copies are left, by measurement: skinny_kernel's bf16 linear chain (head.hip) and gemm_finalize_kernel's epilogues (gemm.hip); see
// there.  The cross-route test (tests/test_gpu_gemm_layouts.py) and scripts/gemm_epilogue_bits.py hold them to these functions.
//
// What holds every route to round-to-nearest-even AT EACH of these rounding points is tests/test_gpu_gemm_rounding.py: its accumulators are
// exact in any summation order and sit on ties (even and odd neighbour), a sticky bit beside a tie, a carry into the exponent, a tie that
// only the second rounding sees (a stage fused onto the unrounded accumulator gives another answer), fp32 subnormals, the tie below 2^128
// and signed zeros, at every column residue mod 8 of every half tile.  Each has ONE correct bit pattern, computed on the CPU
// (tests/gemm_rounding_reference.py); truncation, round-half-up, a skipped rounding, a flush, saturation or a lost sign of zero in any
// kernel, in either form below or in one of the two copies fails there.  A change to this file should meet that test first.
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;   // four bf16: what a lane of the MFMA layout owns of one output row

template <int EPI>
constexpr bool epi_has_row = EPI == EPI_RESID || EPI == EPI_LS_RESID || EPI == EPI_PATCH;

// ---- scalar form: the four consecutive elements of one output row a lane of the MFMA layout owns, one stage at a time -------------------------
template <int EPI>
__device__ __forceinline__ u16x4 epi_acc4(const f32x4& acc, bool has_bias, const u16x4& bias, const u16x4& ls) {
  static_assert(EPI != EPI_SWIGLU, "SwiGLU pairs two accumulators: epi_swiglu4");
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = acc[e];
  if (has_bias) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += bf2f(bias[e]);
  }
  if constexpr (EPI == EPI_GELU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_fast(rbf(v[e]));
  }
  if constexpr (EPI == EPI_LS_RESID) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]) * bf2f(ls[e]);
  }
  u16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);                     // (EPI_STORE / _RESID / _PATCH: this is the Linear's rounding)
  return o;
}
// v = epi_acc's result; r = the residual element (EPI_RESID, EPI_LS_RESID) or the position-table element (EPI_PATCH)
template <int EPI>
__device__ __forceinline__ bf16_t epi_row(bf16_t v, bf16_t r) {
  if constexpr (EPI == EPI_RESID || EPI == EPI_LS_RESID) return f2bf(bf2f(r) + bf2f(v));
  else if constexpr (EPI == EPI_PATCH) return f2bf(bf2f(v) + bf2f(r));
  else return v;
}
template <int EPI>
__device__ __forceinline__ u16x4 epi_row4(const u16x4& v, const u16x4& r) {
  u16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = epi_row<EPI>(v[e], r[e]);
  return o;
}
__device__ __forceinline__ u16x4 epi_swiglu4(const f32x4& gate, const f32x4& up) {
  u16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float g = rbf(gate[e]), u = rbf(up[e]);
    o[e] = f2bf(rbf(silu_f(g)) * u);
  }
  return o;
}

// ---- packed-pair form: two adjacent elements in a v_pk_* / v_cvt_pk_bf16_f32 register pair ---------------------------------------------------
template <int EPI>
__device__ __forceinline__ uint32_t epi_acc2(f32x2 acc, bool has_bias, uint32_t bias, uint32_t ls) {
  static_assert(EPI != EPI_SWIGLU, "SwiGLU pairs two accumulators: epi_swiglu2");
  f32x2 v = acc;
  if (has_bias) v += unpack_bf2(bias);
  if constexpr (EPI == EPI_GELU) v = gelu_fast2(rbf2(v));
  if constexpr (EPI == EPI_LS_RESID) v = rbf2(v) * unpack_bf2(ls);
  return pack_bf2(v);
}
template <int EPI>
__device__ __forceinline__ uint32_t epi_row2(uint32_t v, uint32_t r) {
  const f32x2 fv = unpack_bf2(v);
  if constexpr (EPI == EPI_RESID || EPI == EPI_LS_RESID) return pack_bf2(unpack_bf2(r) + fv);
  else if constexpr (EPI == EPI_PATCH) return pack_bf2(fv + unpack_bf2(r));
  else return v;
}
__device__ __forceinline__ uint32_t epi_swiglu2(f32x2 gate, f32x2 up) {
  const f32x2 g = rbf2(gate), u = rbf2(up);
  return pack_bf2(rbf2(silu2(g)) * u);
}

// ---- host: run-time epilogue -> template argument -----------------------------------------------------------------------------------------------
// with_epi<MASK>(epi, f) calls f(std::integral_constant<int, EPI>{}) for the epilogue `epi` if bit `epi` of MASK is set - only those are ever
// instantiated - and returns hipErrorInvalidValue otherwise.  MASK states which epilogues a launcher accepts.
constexpr unsigned EPI_MASK_BODY = (1u << EPI_STORE) | (1u << EPI_GELU) | (1u << EPI_LS_RESID) | (1u << EPI_RESID) | (1u << EPI_SWIGLU);
constexpr unsigned EPI_MASK_ALL = EPI_MASK_BODY | (1u << EPI_PATCH);

template <unsigned MASK, int E = 0, class F>
inline hipError_t with_epi(int epi, F&& f) {
  if constexpr (E >= EPI_COUNT) {
    return hipErrorInvalidValue;
  } else {
    if constexpr ((MASK >> E) & 1u) {
      if (epi == E) return f(std::integral_constant<int, E>{});
    }
    return with_epi<MASK, E + 1>(epi, f);
  }
}
