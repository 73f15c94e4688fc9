// Joint posterior draws f(X*) ~ N(mu*, Sigma~) of a fitted emulator (sample_posterior, DESIGN.md section 3 "Sampling"):
// Sigma~ = Sigma* + shift I = L L^T is factored by the engine's batched Cholesky in a scratch engine of m rows, and a draw is mu* + L z.
//   sample_gather_kernel   Sigma* (m x m dense) -> the factor-matrix layout of a scratch-engine slot (launch.h), the shift on the diagonal
//   sample_polish_kernel   the factor's diagonal recomputed from its finished rows with the correctly rounded square root
//   sample_normals_kernel  z from a counter-based generator (philox_dev.h): a value depends on (seed, stream, draw, point) alone
//   sample_apply_kernel    Y^T tile (128 points x 64 draws) = L[tile rows, 0 .. end of the diagonal block] Z^T + mu on fp64 MFMA
// Every output has one writer, the k sum of an output runs in a fixed order that depends on its row tile alone, nothing is atomic: the
// same call returns the same bits, and cutting the draws into other chunks changes none.
#include "launch.h"
#include "devmem.h"
#include "gemm_dev.h"
#include "philox_dev.h"

namespace mogp {

namespace {

// One 64 x 64 tile of the factor matrix of batch entry blockIdx.z (slot idx[z] of the scratch engine): thread (ty, tx) = (t >> 5, t & 31)
// owns rows 8 ty .. 8 ty + 7 and columns 2 tx, 2 tx + 1, so that one store instruction of a wave is two whole 512-byte rows of the tile
// (cv_gather_kernel's shape).  One writer per element.  Tiles above the diagonal are exact zeros: the factorisation reads the lower
// triangle only and zeroes the strict upper triangle of its 64 x 64 diagonal tiles (chol128_dev.h), so that afterwards every 128 x 128
// diagonal block of A is L's with zeros above the diagonal -- what sample_apply_kernel reads.
__global__ __launch_bounds__(256) void sample_gather_kernel(const int* __restrict__ idx, double* __restrict__ A, int NPs,
                                                            const double* __restrict__ cov, const int* __restrict__ src,
                                                            const double* __restrict__ shift, int m) {
  const int slot = idx ? idx[blockIdx.z] : (int)blockIdx.z;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int sc = src[slot];
  const double sh = shift[slot];
  const double* C = cov + (size_t)max(sc, 0) * m * m;
  double* Az = A + (size_t)slot * NPs * NPs;
  const int ty = threadIdx.x >> 5, tx = threadIdx.x & 31;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int i = i0 + 8 * ty + a;
    double out[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = j0 + 2 * tx + b;
      const int hi = max(i, j);
      double x;
      if (j0 > i0) x = 0.0;
      else if (sc >= 0 && hi < m) x = C[(size_t)i * m + j] + (i == j ? sh : 0.0);
      else if (sc >= 0 && hi == m) x = (i == j) ? PAD_BIG : 0.0;          // target row (and its mirror column): neutral
      else x = (i == j) ? 1.0 : 0.0;
      out[b] = x;
    }
    *reinterpret_cast<double2*>(Az + (size_t)i * NPs + j0 + 2 * tx) = make_double2(out[0], out[1]);
  }
}

// One wave per row j (blockIdx.x) of slot blockIdx.y, behind the factorisation: L[j][j] <- sqrt(Sigma~[j][j] - sum_{k<j} L[j][k]^2), the
// sum taken as 64 lane-strided partial sums combined by a butterfly (a fixed order), Sigma~[j][j] formed as the gather formed it.  Kept as
// it is where that is not a positive finite number (a slot that failed, cancellation in a numerically singular row).
__global__ __launch_bounds__(64) void sample_polish_kernel(double* __restrict__ A, int NPs, const double* __restrict__ cov,
                                                           const int* __restrict__ src, const double* __restrict__ shift, int m) {
  const int j = blockIdx.x, slot = blockIdx.y, lane = threadIdx.x;
  const int sc = src[slot];
  if (sc < 0) return;
  double* row = A + (size_t)slot * NPs * NPs + (size_t)j * NPs;
  double s = 0.;
  for (int k = lane; k < j; k += 64) s = __builtin_fma(row[k], row[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane != 0) return;
  const double d = (cov[(size_t)sc * m * m + (size_t)j * m + j] + shift[slot]) - s;
  const double l = sqrt(d);
  if (d > 0. && l > 0. && l < 1e300) row[j] = l;
}

// One thread per (draw, pair of points): row blockIdx.y of slot blockIdx.z, pair p -> Z[2p], Z[2p + 1] in one 16-byte store.  An odd m
// drops the last sine (a zero is stored: column m is padding).  Columns >= roundup(m, 2) are never written: they hold the zeros of the
// buffer's memset.
__global__ __launch_bounds__(256) void sample_normals_kernel(double* __restrict__ Z, long zrows, int MP, int m, long s0, unsigned long long seed,
                                                             const unsigned* __restrict__ streams) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (2 * p >= m) return;
  const int r = blockIdx.y, slot = blockIdx.z;
  double z0, z1;
  philox_normal_pair(seed, streams[slot], (uint32_t)(s0 + r), (uint32_t)p, z0, z1);
  if (2 * p + 1 >= m) z1 = 0.0;
  *reinterpret_cast<double2*>(Z + ((size_t)slot * zrows + r) * MP + 2 * p) = make_double2(z0, z1);
}

// Workgroup (x, y, z) = (row tile of 128 points, longest first; tile of 64 draws; slot).  A operand: rows i0 .. i0 + 127 of the factor,
// columns 0 .. end of the diagonal block -- lower triangular, so the structurally zero sub-tiles of the diagonal block and the sub-tiles
// below row m are skipped (mainloop_w<.., TRIA>).  B operand: 64 rows of Z, K-major as stored.  With TRIA and 2 x 2 waves, accumulator
// acc[i][j][r] of wave (wr, wc) is point (2 i + wr) 16 + (lane >> 4) + 4 r, draw (2 wc + j) 16 + (lane & 15) of the tile.  The tile goes
// through LDS transposed, so that a wave stores 64 consecutive points of one draw; mu is added there.  Rows >= m and draws >= sc are
// masked; for rows < m the columns k >= m of the factor (its target row's mirror column, the padding) are in the strict upper triangle
// -- zeros -- and meet zeros of Z.
using SampleCfg = WCfg<128, 64, 2, 2>;
constexpr int SAMPLE_YLD = 129;
constexpr int SAMPLE_LDS_DOUBLES = SampleCfg::SMEM_DOUBLES > 64 * SAMPLE_YLD ? SampleCfg::SMEM_DOUBLES : 64 * SAMPLE_YLD;

__global__ __launch_bounds__(256, 2) void sample_apply_kernel(const double* __restrict__ A, int NPs, const double* __restrict__ Z, long zrows,
                                                              int MP, const double* __restrict__ mu, int m, int sc, double* __restrict__ Y,
                                                              long yrows) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int nti = MP / 128;
  const int i0 = (nti - 1 - (int)blockIdx.x) * 128, d0 = blockIdx.y * 64, slot = blockIdx.z;
  const double* L = A + (size_t)slot * NPs * NPs;
  const double* Zs = Z + (size_t)slot * zrows * MP;
  v4d acc[SampleCfg::TI][SampleCfg::TJ];
  const int nk = min(i0 + 128, (m + 15) & ~15) / BK;
  mainloop_w<128, 64, 2, 2, true, true, true>(L + (size_t)i0 * NPs, NPs, Zs + (size_t)d0 * MP, MP, nk, acc, smem, i0 / BK, m - i0);
  // (the main loop ends behind a barrier: the operand tiles are dead)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
#pragma unroll
  for (int i = 0; i < SampleCfg::TI; ++i)
#pragma unroll
    for (int j = 0; j < SampleCfg::TJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        smem[((2 * wc + j) * 16 + (lane & 15)) * SAMPLE_YLD + (2 * i + wr) * 16 + (lane >> 4) + 4 * r] = acc[i][j][r];
  __syncthreads();
  const double* mus = mu + (size_t)slot * m;
  double* Ys = Y + (size_t)slot * yrows * m;
  for (int d = wave; d < 64; d += 4) {
    const int draw = d0 + d;
    if (draw >= sc) break;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = h * 64 + lane, j = i0 + row;
      if (j < m) Ys[(size_t)draw * m + j] = mus[j] + smem[d * SAMPLE_YLD + row];
    }
  }
}

}  // namespace

void launch_sample_gather(const BatchView& sv, const double* cov, const int* src, const double* shift, int m, hipStream_t s) {
  if (sv.nb <= 0) return;
  prof_begin("sample_gather", s);
  hipLaunchKernelGGL(sample_gather_kernel, dim3(sv.NP / 64, sv.NP / 64, sv.nb), dim3(256), 0, s, sv.idx, sv.A, sv.NP, cov, src, shift, m);
  HIPCK(hipGetLastError());
  prof_end("sample_gather", s, 0., (double)sv.nb * sv.NP * sv.NP * 8.0);
}

void launch_sample_polish(double* A, int NPs, int nslots, const double* cov, const int* src, const double* shift, int m, hipStream_t s) {
  if (nslots <= 0 || m <= 0) return;
  prof_begin("sample_polish", s);
  hipLaunchKernelGGL(sample_polish_kernel, dim3(m, nslots), dim3(64), 0, s, A, NPs, cov, src, shift, m);
  HIPCK(hipGetLastError());
  prof_end("sample_polish", s, 0., (double)nslots * m * m * 4.0);
}

void launch_sample_normals(double* Z, int nslots, long zrows, int MP, int m, int sc, long s0, unsigned long long seed, const unsigned* streams,
                           hipStream_t s) {
  if (nslots <= 0 || sc <= 0 || m <= 0) return;
  const int pairs = (m + 1) / 2;
  prof_begin("sample_normals", s);
  hipLaunchKernelGGL(sample_normals_kernel, dim3((pairs + 255) / 256, sc, nslots), dim3(256), 0, s, Z, zrows, MP, m, s0, seed, streams);
  HIPCK(hipGetLastError());
  prof_end("sample_normals", s, 0., (double)nslots * sc * m * 8.0);
}

void launch_sample_apply(const double* A, int NPs, const double* Z, long zrows, int MP, const double* mu, int m, int sc, int nslots,
                         double* Y, long yrows, hipStream_t s) {
  if (nslots <= 0 || sc <= 0 || m <= 0) return;
  prof_begin("sample_apply", s);
  hipLaunchKernelGGL(sample_apply_kernel, dim3(MP / 128, (sc + 63) / 64, nslots), dim3(256), SAMPLE_LDS_DOUBLES * sizeof(double), s, A, NPs, Z,
                     zrows, MP, mu, m, sc, Y, yrows);
  HIPCK(hipGetLastError());
  prof_end("sample_apply", s, (double)nslots * sc * (double)m * m, (double)nslots * ((double)m * m * 4.0 + 2.0 * sc * m * 8.0));
}

}  // namespace mogp
