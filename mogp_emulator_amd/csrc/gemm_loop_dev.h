// The 2 x 2-wave fp64 MFMA main loop of the tile kernels (kernels_gemm.hip) and of the active-learning kernels (kernels_alc.hip):
// gemm_mainloop<WT, A_KMAJ, B_KMAJ>, its LDS layout, the accumulator iteration and the decode of a 1-D grid into (slot, tile).
// kernels_gemm.hip describes the layouts at its head.
#pragma once
#include "launch.h"
#include "gemm_dev.h"

namespace mogp {

template <int WT>
struct Cfg {
  static constexpr int BM = 32 * WT;            // block tile edge
  static constexpr int WM = 16 * WT;            // wave tile edge
  static constexpr int LDM = BM + 16;
  static constexpr int CH = BM * 8 / 256;       // 16-byte chunks per thread per operand tile
  static constexpr int OPSZ = (BM * LDK > BK * LDM) ? BM * LDK : BK * LDM;
  static constexpr int SMEM_DOUBLES = 4 * OPSZ; // 2 buffers x (A, B)
};

// Global -> register staging of one operand tile.  A thread's chunks q = 0 .. CH-1 lie a whole number of rows apart, so it needs ONE
// 32-bit byte offset (g2r_off) against wave-uniform bases g + q * ROWS * ld: scalar base + vector offset addressing, no 64-bit address
// arithmetic per load and fewer address registers than per-thread pointers (predictive variance: 65.4 -> 66.0 TFLOP/s with the same change).
template <int WT, bool KMAJ>
__device__ __forceinline__ unsigned g2r_off(int ld) {
  const int t = threadIdx.x;
  const int off = KMAJ ? (t >> 3) * ld + (t & 7) * 2 : (t / (Cfg<WT>::BM / 2)) * ld + (t % (Cfg<WT>::BM / 2)) * 2;
  return (unsigned)(off * (int)sizeof(double));
}
template <int WT, bool KMAJ>
__device__ __forceinline__ void g2r(const double* __restrict__ g, int ld, unsigned off, v2d (&r)[Cfg<WT>::CH]) {
  constexpr int ROWS = KMAJ ? 32 : 256 / (Cfg<WT>::BM / 2);     // rows between a thread's consecutive chunks
#pragma unroll
  for (int q = 0; q < Cfg<WT>::CH; ++q) r[q] = *reinterpret_cast<const v2d*>(reinterpret_cast<const char*>(g + (size_t)q * ROWS * ld) + off);
}

template <int WT, bool KMAJ>
__device__ __forceinline__ void r2s(double* s, const v2d (&r)[Cfg<WT>::CH]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Cfg<WT>::CH; ++q) {
    const int c = t + 256 * q;
    if (KMAJ) {
      const int row = c >> 3, kc = (c & 7) * 2;
      *reinterpret_cast<v2d*>(s + row * LDK + kc) = r[q];
    } else {
      const int krow = c / (Cfg<WT>::BM / 2), mc = (c % (Cfg<WT>::BM / 2)) * 2;
      *reinterpret_cast<v2d*>(s + krow * Cfg<WT>::LDM + mc) = r[q];
    }
  }
}

template <int WT, bool KMAJ>
__device__ __forceinline__ double frag(const double* s, int row, int k) {
  return KMAJ ? s[row * LDK + k] : s[k * Cfg<WT>::LDM + row];
}

// Ag: K-major -> &A[i0*lda + k0] ; M-major -> &A[k0*lda + i0].  nk = number of 16-deep steps.
template <int WT, bool AK, bool BKM>
__device__ __forceinline__ void gemm_mainloop(const double* __restrict__ Ag, int lda, const double* __restrict__ Bg,
                                              int ldb, int nk, v4d (&acc)[WT][WT], double* smem) {
  using C = Cfg<WT>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[i][j] = (v4d){0., 0., 0., 0.};
  if (nk <= 0) return;

  const size_t stepA = AK ? (size_t)BK : (size_t)BK * lda;
  const size_t stepB = BKM ? (size_t)BK : (size_t)BK * ldb;
  v2d ra[C::CH], rb[C::CH];
  const unsigned offA = g2r_off<WT, AK>(lda), offB = g2r_off<WT, BKM>(ldb);
  g2r<WT, AK>(Ag, lda, offA, ra);
  g2r<WT, BKM>(Bg, ldb, offB, rb);
  r2s<WT, AK>(smem, ra);
  r2s<WT, BKM>(smem + C::OPSZ, rb);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const double* sA = smem + (kt & 1) * 2 * C::OPSZ;
    const double* sB = sA + C::OPSZ;
    const bool more = (kt + 1 < nk);
    if (more) {
      Ag += stepA;
      Bg += stepB;
      g2r<WT, AK>(Ag, lda, offA, ra);
      g2r<WT, BKM>(Bg, ldb, offB, rb);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double a[WT], b[WT];
      const int k = kk * 4 + fk;
#pragma unroll
      for (int i = 0; i < WT; ++i) a[i] = frag<WT, AK>(sA, wr * C::WM + i * 16 + fr, k);
#pragma unroll
      for (int j = 0; j < WT; ++j) b[j] = frag<WT, BKM>(sB, wc * C::WM + j * 16 + fr, k);
#pragma unroll
      for (int i = 0; i < WT; ++i)
#pragma unroll
        for (int j = 0; j < WT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      double* dA = smem + ((kt + 1) & 1) * 2 * C::OPSZ;
      r2s<WT, AK>(dA, ra);
      r2s<WT, BKM>(dA + C::OPSZ, rb);
    }
    __syncthreads();
  }
}

// iterate the accumulator fragment: f(row_in_tile, col_in_tile, value&)
template <int WT, typename F>
__device__ __forceinline__ void for_each_acc(v4d (&acc)[WT][WT], F f) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int i = 0; i < WT; ++i)
#pragma unroll
    for (int j = 0; j < WT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        f(wr * Cfg<WT>::WM + i * 16 + (lane >> 4) + 4 * r, wc * Cfg<WT>::WM + j * 16 + (lane & 15), acc[i][j][r]);
}

__device__ __forceinline__ int slot_to_emu(const int* idx, int z) { return idx ? idx[z] : z; }

// Decode a 1-D grid into (batch slot z, tile id).  When the slot count is a multiple of 8 each
// XCD (block id % 8) works through whole emulators one after another, so an emulator's panels
// and trailing matrix stay inside one 4 MiB L2 instead of being spread over all eight.
__device__ __forceinline__ void decode_block(int nb, int ntiles, int& z, int& tile, int L = (int)blockIdx.x) {
  if ((nb & 7) == 0) {
    const int xcd = L & 7, w = L >> 3;
    z = (w / ntiles) * 8 + xcd;
    tile = w % ntiles;
  } else {
    z = L / ntiles;
    tile = L % ntiles;
  }
}

}  // namespace mogp
