// bf16 GEMM  C[M,N] = epilogue(A[M,K] · W[N,K]^T)  for gfx950: MFMA 16x16x32 bf16, fp32 accumulate.
//
// This one kernel carries ~95 % of the scorer's FLOPs (ViT qkv/proj/fc1/fc2, projector, LLM
// wqkv/wo/w1|w3/w2).  Both operands are K-contiguous (activations [M,K]; nn.Linear weights [N,K]),
// so A and W tiles are staged the same way.
//
//   tile 128x128x64, 256 threads = 4 waves (2x2), each wave a 64x64 output = 4x4 MFMA tiles
//   LDS  2 buffers x (A 16 KB + W 16 KB) = 64 KB  -> 2 workgroups per CU
//   staging: global_load_lds dwordx4 (16 B/lane, 1 KB per wave-instruction = 8 rows x 128 B).  The
//     LDS image is lane-linear, so the bank-conflict swizzle (16-B chunk ^= row&7) is applied to the
//     per-lane SOURCE address and again on the ds_read_b128 fragment reads (guide rule 21 / T2).
//   pipeline: tile t+1 is in flight (LDS-DMA) while tile t is multiplied; one barrier per K step.
//   MFMA operand order is swapped (W first) so that a lane owns 4 consecutive output COLUMNS of one
//     row: epilogue loads/stores are 8-byte vectors and per-column vectors (bias, layer-scale) are
//     one 8-byte load.
//   blockIdx -> tile: XCD-aware bijective remap (blocks b, b+8 share an XCD/L2), then groups of 8
//     row-tiles sweep the column tiles so co-resident workgroups share A and W panels in L2.
//
// Epilogues reproduce the rounding points of the reference's eager bf16 path:
// every Linear output rounds to bf16 (bias added in fp32 first), activations round, layer-scale
// rounds, residual adds round.
#include "common.h"
#include "epilogue.h"
#include "kernels.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;          // 16 KB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;      // A + W
constexpr int GROUP_M = 8;

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- tile mapping -------------------------------------------------------------------------
  // rows: tile tm covers rows [tm * 128, ..) of the matrix, or - with a half-tile table (GemmArgs::row_tab, the per-sequence row plans
  // of dispatch.hip) - the table's half tm: `valid` rows from its base row
  const int nbm = p.row_tab ? p.tab_halves : (p.M + BM - 1) / BM, nbn = p.N / BN;
  const int nwg = nbm * nbn;
  int wg;
  {
    const int bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int per_group = GROUP_M * nbn;
  const int group = wg / per_group, first_m = group * GROUP_M;
  const int gsz = min(nbm - first_m, GROUP_M);
  const int in_g = wg - group * per_group;
  const int tm = first_m + in_g % gsz, tn = in_g / gsz;
  const int n0 = tn * BN;
  int m0 = tm * BM, mend = p.M;
  if (p.row_tab) {
    m0 = __builtin_amdgcn_readfirstlane(p.row_tab[2 * tm]);
    mend = m0 + __builtin_amdgcn_readfirstlane(p.row_tab[2 * tm + 1]);
  }

  // ---- staging addresses ----------------------------------------------------------------------
  // wave-instruction i of this wave fills rows (wave*4+i)*8 .. +7 of the tile; lane -> row lane>>3,
  // 16-B chunk lane&7 of the LDS row; it fetches global chunk (lane&7) ^ (row&7).
  const int lr = lane >> 3;
  const int lc = (lane & 7) ^ lr;
  const bf16_t* srcA[4];
  const bf16_t* srcW[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rl = (wave * 4 + i) * 8 + lr;
    const int ra = min(m0 + rl, mend - 1);  // clamp: rows past the end are computed on a copy, never stored
    srcA[i] = p.A + (size_t)ra * p.lda + lc * 8;
    srcW[i] = p.W + (size_t)(n0 + rl) * p.ldw + lc * 8;
  }
  auto stage = [&](int buf, int k0) {
    char* base = smem + buf * STAGE_BYTES + wave * 4 * 1024;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(srcA[i] + k0, base + i * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(srcW[i] + k0, base + TILE_BYTES + i * 1024);
  };

  // ---- fragment read addresses ------------------------------------------------------------------
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  // row (within the 128-row tile) of fragment t of this wave: w*64 + t*16 + fr ; (row & 7) == (fr & 7)
  const int sw = fr & 7;
  int offA[2], offW[2];  // byte offset inside a tile for k-half 0/1, fragment 0 (add t*16*128 per fragment)
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    const int phys = (kh * 4 + fq) ^ sw;
    offA[kh] = (wm * 64 + fr) * 128 + phys * 16;
    offW[kh] = (wn * 64 + fr) * 128 + phys * 16;
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // split-K (EPI_PARTIAL): blockIdx.y picks the K slice
  const int nk = (EPI == EPI_PARTIAL) ? p.K / BK / p.k_slices : p.K / BK;
  const int kbase = (EPI == EPI_PARTIAL) ? (int)blockIdx.y * nk * BK : 0;
  stage(0, kbase);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile t landed for every wave; everyone is done reading the other buffer
    if (t + 1 < nk) stage((t + 1) & 1, kbase + (t + 1) * BK);
    const char* sA = smem + (t & 1) * STAGE_BYTES;
    const char* sW = sA + TILE_BYTES;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      bf16x8 a[4], w[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *(const bf16x8*)(sA + offA[kh] + i * 16 * 128);
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = *(const bf16x8*)(sW + offW[kh] + j * 16 * 128);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[j], a[i], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue: lane owns C[m][n .. n+3], m = ..+fr, n = ..+4*fq ---------------------------------
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + fr;
    if (m >= mend) continue;
    if constexpr (EPI == EPI_PARTIAL) {
      float* slab = p.part + ((size_t)blockIdx.y * p.M + m) * p.N;
#pragma unroll
      for (int j = 0; j < 4; ++j) *(f32x4*)(slab + n0 + wn * 64 + j * 16 + fq * 4) = acc[i][j];
    } else if constexpr (EPI == EPI_SWIGLU) {
      // W rows are interleaved in 16-row blocks: even block = w1 (gate), odd block = w3 (up)
#pragma unroll
      for (int jp = 0; jp < 2; ++jp) {
        const int n = (n0 + wn * 64) / 2 + jp * 16 + fq * 4;
        *(u16x4*)(p.C + (size_t)m * p.ldc + n) = epi_swiglu4(acc[i][2 * jp], acc[i][2 * jp + 1]);
      }
    } else {
      size_t orow = (size_t)m;
      const bf16_t* rrow = nullptr;                      // the row epi_row adds: residual or position row
      if constexpr (EPI == EPI_PATCH) {
        const int f = m / p.np, pi = m - f * p.np;
        orow = (size_t)m + f + 1;                      // skip one class-token row per frame
        rrow = p.pos + (size_t)(pi + 1) * p.N;
      }
      if constexpr (EPI == EPI_LS_RESID || EPI == EPI_RESID) rrow = p.resid + (size_t)m * p.ldr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + wn * 64 + j * 16 + fq * 4;
        u16x4 b{}, s{}, r{};
        if (p.bias) b = *(const u16x4*)(p.bias + n);
        if constexpr (EPI == EPI_LS_RESID) s = *(const u16x4*)(p.ls + n);
        const u16x4 v = epi_acc4<EPI>(acc[i][j], p.bias != nullptr, b, s);
        if constexpr (epi_has_row<EPI>) r = *(const u16x4*)(rrow + n);
        *(u16x4*)(p.C + orow * p.ldc + n) = epi_row4<EPI>(v, r);
      }
    }
  }
}

template <int EPI>
hipError_t launch(const GemmArgs& a, hipStream_t s) {
  static LdsAttrOnce lds_attr;
  if (hipError_t e = lds_attr.ensure((const void*)gemm_bf16_kernel<EPI>, 2 * STAGE_BYTES); e != hipSuccess) return e;
  if (a.row_tab && (EPI == EPI_PARTIAL || EPI == EPI_PATCH)) return hipErrorInvalidValue;   // the table form has no slab / patch row mapping here
  const int nbm = a.row_tab ? a.tab_halves : (a.M + BM - 1) / BM, nbn = a.N / BN;
  if (nbm <= 0) return hipSuccess;
  hipLaunchKernelGGL(gemm_bf16_kernel<EPI>, dim3(nbm * nbn), dim3(256), 2 * STAGE_BYTES, s, a);
  return hipGetLastError();
}

// ---- split-K finalize: sum the slabs in slice order, then the same epilogues as the GEMM kernels ------------------
template <int EPI>
__global__ __launch_bounds__(256) void gemm_finalize_kernel(const GemmArgs p, const float* __restrict__ part, int S) {
  const int nq = p.N / 4;                       // float4 groups per row
  // slab rows: the output rows themselves, or (GemmArgs::row_tab, the 256 kernel's half-tile table) compact rows half * 128 + r
  const size_t srows = p.row_tab ? (size_t)((p.tab_halves + 1) / 2) * 256 : (size_t)p.M;
  const size_t total = (p.row_tab ? (size_t)p.tab_halves * 128 : (size_t)p.M) * nq, slab = srows * p.N;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int sm = (int)(i / nq), n = (int)(i - (size_t)sm * nq) * 4;
    int m = sm;
    if (p.row_tab) {
      const int h = sm >> 7, r = sm & 127;
      if (r >= p.row_tab[2 * h + 1]) continue;
      m = p.row_tab[2 * h] + r;
    }
    f32x4 a = *(const f32x4*)(part + (size_t)sm * p.N + n);
    for (int sidx = 1; sidx < S; ++sidx) {
      const f32x4 b = *(const f32x4*)(part + sidx * slab + (size_t)sm * p.N + n);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] += b[e];
    }
    if constexpr (EPI == EPI_SWIGLU) {
      // 16-row interleave: columns [32b, 32b+16) gate, [32b+16, 32b+32) up -> output column 16b + (n % 16)
      const int blk = n >> 5, within = n & 31;
      if (within >= 16) continue;               // the gate thread also reads its up partner
      f32x4 u = *(const f32x4*)(part + (size_t)sm * p.N + n + 16);
      for (int sidx = 1; sidx < S; ++sidx) {
        const f32x4 b = *(const f32x4*)(part + sidx * slab + (size_t)sm * p.N + n + 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] += b[e];
      }
      u16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(rbf(silu_f(rbf(a[e]))) * rbf(u[e]));
      *(u16x4*)(p.C + (size_t)m * p.ldc + blk * 16 + within) = o;
    } else {
      // This kernel's own text of epilogue.h's chains (epi_acc4 then epi_row4; epi_swiglu4 above).  Through the shared functions the kernel
      // measured 0.07 ms per step behind the parent's in the benched step (profiles/gemm_epilogue_bench_ab.txt), so the text stays;
      // scripts/gemm_epilogue_bits.py and test_gelu_and_swiglu_bits_agree_on_every_route hold it in step with the other kernels.
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = a[e];
      if (p.bias) {
        const u16x4 b = *(const u16x4*)(p.bias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += bf2f(b[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = rbf(v[e]);
      if constexpr (EPI == EPI_GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(gelu_fast(v[e]));
      }
      if constexpr (EPI == EPI_LS_RESID) {
        const u16x4 sc = *(const u16x4*)(p.ls + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(v[e] * bf2f(sc[e]));
      }
      if constexpr (EPI == EPI_LS_RESID || EPI == EPI_RESID) {
        const u16x4 r = *(const u16x4*)(p.resid + (size_t)m * p.ldr + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = rbf(bf2f(r[e]) + v[e]);
      }
      u16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
      *(u16x4*)(p.C + (size_t)m * p.ldc + n) = o;
    }
  }
}

// (no patch epilogue in split-K: the slabs have no class-token row mapping)
hipError_t launch_finalize(const GemmArgs& a, int epi, const float* part, int S, hipStream_t s) {
  return with_epi<EPI_MASK_BODY>(epi, [&](auto E) {
    const size_t total = (a.row_tab ? (size_t)a.tab_halves * 128 : (size_t)a.M) * (a.N / 4);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(gemm_finalize_kernel<decltype(E)::value>, dim3(blocks), dim3(256), 0, s, a, part, S);
    return hipGetLastError();
  });
}

}  // namespace

const char* aigv_gemm_check(const GemmArgs& a, int epi) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return "gemm: empty problem";
  if (a.N % BN) return "gemm: N must be a multiple of 128";
  if (a.K % BK) return "gemm: K must be a multiple of 64";
  if (a.lda < a.K || a.ldw < a.K || (a.lda % 8) || (a.ldw % 8)) return "gemm: bad leading dimension (lda and ldw: at least K, multiples of 8)";
  // Row strides of C and of the residual.  The dispatcher may put any rows of a call on any tile kernel, so ONE rule covers the widest access
  // of them all: the 128 kernel stores and reads 8 bytes (the u16x4 at C + orow * ldc + n and at resid + m * ldr + n above), the 256 and
  // the co-resident kernels 16 (store_row_segment's u16x8 at C + m * ldc + n in gemm256.hip / gemmco.hip, and the residual's 16-byte
  // LDS-direct prefetch resid_dma from resid + hb * ldr + n0).  Every width of the models is a multiple of 8.
  const int n_out = epi == EPI_SWIGLU ? a.N / 2 : a.N;
  if (a.ldc < n_out) return epi == EPI_SWIGLU ? "gemm: swiglu output is N/2 wide: ldc is below it (rows would overlap)" : "gemm: ldc is below N (rows would overlap)";
  if (a.ldc % 8) return "gemm: ldc must be a multiple of 8 (the tile kernels store 16 bytes at C + row * ldc + n)";
  if (a.resid && a.ldr < n_out) return "gemm: ldr is below the width of the residual rows";
  if (a.resid && (a.ldr % 8)) return "gemm: ldr must be a multiple of 8 (the tile kernels read 16 bytes at resid + row * ldr + n)";
  if (!a.A || !a.W || !a.C) return "gemm: null operand";
  if ((epi == EPI_LS_RESID) && (!a.ls || !a.resid)) return "gemm: layer-scale/residual epilogue needs ls and resid";
  if ((epi == EPI_RESID) && !a.resid) return "gemm: residual epilogue needs resid";
  if ((epi == EPI_PATCH) && (!a.pos || a.np <= 0 || a.M % a.np)) return "gemm: patch epilogue needs pos, np | M";
  if (epi < 0 || epi >= EPI_COUNT) return "gemm: unknown epilogue";
  return nullptr;
}

// the fp8 form's split-K: scaled fp32 slabs from the e4m3 kernel, then the same fixed-order finalize pass as the bf16 path
hipError_t aigv_launch_gemm_splitk_fp8(const GemmArgs& a, int epi, int k_slices, float* ws, hipStream_t s) {
  if (k_slices < 2 || !ws) return hipErrorInvalidValue;
  GemmArgs b = a;
  b.part = ws;
  b.k_slices = k_slices;
  hipError_t e = aigv_launch_gemm256_fp8_partial(b, s);
  if (e != hipSuccess) return e;
  return launch_finalize(a, epi, ws, k_slices, s);
}

// the second half of a split-K GEMM on its own: sum the k_slices slabs in slice order + epilogue `epi` (a.row_tab / a.tab_halves = the rows
// the slabs hold, as the slice launch addressed them)
hipError_t aigv_launch_gemm_finalize(const GemmArgs& a, int epi, int k_slices, const float* ws, hipStream_t s) {
  if (k_slices < 2 || !ws) return hipErrorInvalidValue;
  return launch_finalize(a, epi, ws, k_slices, s);
}

hipError_t aigv_launch_gemm_splitk(const GemmArgs& a, int epi, int k_slices, float* ws, hipStream_t s, bool tile256) {
  if (k_slices < 2 || (a.K / BK) % k_slices || !ws || epi == EPI_PATCH || epi >= EPI_COUNT) return hipErrorInvalidValue;
  if (!tile256 && a.row_tab) return hipErrorInvalidValue;   // the 128 kernel's slabs have no table mapping
  if (tile256) {
    GemmArgs b = a;
    b.part = ws;
    b.k_slices = k_slices;
    hipError_t e = aigv_launch_gemm256_partial(b, s);
    if (e != hipSuccess) return e;
    return launch_finalize(a, epi, ws, k_slices, s);
  }
  static LdsAttrOnce lds_attr;
  if (hipError_t e = lds_attr.ensure((const void*)gemm_bf16_kernel<EPI_PARTIAL>, 2 * STAGE_BYTES); e != hipSuccess) return e;
  GemmArgs b = a;
  b.part = ws;
  b.k_slices = k_slices;
  const int nbm = (a.M + BM - 1) / BM, nbn = a.N / BN;
  hipLaunchKernelGGL(gemm_bf16_kernel<EPI_PARTIAL>, dim3(nbm * nbn, k_slices), dim3(256), 2 * STAGE_BYTES, s, b);
  return launch_finalize(a, epi, ws, k_slices, s);
}

hipError_t aigv_launch_gemm(const GemmArgs& a, int epi, hipStream_t s) {
  return with_epi<EPI_MASK_ALL>(epi, [&](auto E) { return launch<decltype(E)::value>(a, s); });
}
