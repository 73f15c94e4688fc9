// Variance-based sensitivity analysis (first-order and total-effect Sobol indices) behind the batched prediction.
//
// A, B are two independent (N, D) sample matrices, AB_i is A with column i taken from B, f the predictive mean of one emulator:
//   f0   = mean(concat(fA, fB))                         V = mean((concat(fA, fB) - f0)^2)        (two passes, population variance)
//   S_i  = mean((fB - f0) (fAB_i - fA)) / V             (Saltelli 2010)
//   ST_i = mean((fA - fAB_i)^2) / (2 V)                 (Jansen)
// The kernels here are the three consumers around the mean path of Engine::predict: pick_freeze writes a chunk of AB_i, the row-sum
// kernel gives f0, V and the mean predictive variance, the pair-sum kernel the two numerators of a chunk.  Every one is bound by HBM.
//
// Reductions: every thread adds its grid-strided elements in ascending order, a wave reduces by shuffles, the four waves of a workgroup
// through LDS, and the workgroup writes ONE partial into a scratch slot of its own; a final kernel adds the slots of one quantity in a
// fixed order.  No floating-point atomics anywhere: the same inputs (and the same chunking) give the same bits in every call.
#include <algorithm>
#include <stdexcept>

#include "launch.h"

namespace mogp {

namespace {

// sum over the 256 threads of a workgroup, valid in thread 0: shuffles inside a wave, then LDS across the four waves
__device__ __forceinline__ double block_sum(double v, double* wsum) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __syncthreads();                                  // wsum may still be read from the previous call
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// out (rows, D) = A[r0 .. r0 + rows) with column `col` taken from B
__global__ __launch_bounds__(256) void sobol_pick_freeze_kernel(const double* __restrict__ A, const double* __restrict__ B, long r0,
                                                                int rows, int D, int col, double* __restrict__ out) {
  const long total = (long)rows * D;
  const long stride = (long)gridDim.x * 256;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int d = (int)(e % D);
    const long src = r0 * D + e;
    out[e] = (d == col) ? B[src] : A[src];
  }
}

// partial[k * gridDim.x + w] = the sum over the elements j of workgroup w, with c = prm[k * pstride], of
//   mode 0: x[k][j]      mode 1: (x[k][j] - c)^2      mode 2: max(x[k][j] + c, 0)  (a predictive variance plus its nugget, clipped as predict clips it)
template <int MODE>
__global__ __launch_bounds__(256) void sobol_row_sum_kernel(const double* __restrict__ x, long ld, long m, const double* __restrict__ prm,
                                                            int pstride, double* __restrict__ partial) {
  __shared__ double wsum[4];
  const int k = blockIdx.y;
  const double* xr = x + (size_t)k * ld;
  const long stride = (long)gridDim.x * 256;
  const double c = MODE == 0 ? 0. : prm[(size_t)k * pstride];
  double s = 0.;
  for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < m; j += stride) {
    const double v = xr[j];
    if (MODE == 0) s += v;
    else if (MODE == 1) s += (v - c) * (v - c);
    else s += fmax(v + c, 0.);
  }
  s = block_sum(s, wsum);
  if (threadIdx.x == 0) partial[(size_t)k * gridDim.x + blockIdx.x] = s;
}

// the two numerators of one chunk of base rows: fA / fB (nb, ld) at the chunk's first row, fAB (nb, ldab); f0 = stats[k * sstride]
//   partial[((k * D + col) * nslot + slot0 + w) * 2 + {0, 1}] = sum (fB - f0) (fAB - fA),  sum (fA - fAB)^2
__global__ __launch_bounds__(256) void sobol_pair_sum_kernel(const double* __restrict__ fA, const double* __restrict__ fB, long ld,
                                                             const double* __restrict__ fAB, long ldab, int rows,
                                                             const double* __restrict__ stats, int sstride, double* __restrict__ partial,
                                                             int D, int col, long nslot, long slot0) {
  __shared__ double wsum[4];
  const int k = blockIdx.y;
  const double* a = fA + (size_t)k * ld;
  const double* b = fB + (size_t)k * ld;
  const double* ab = fAB + (size_t)k * ldab;
  const double f0 = stats[(size_t)k * sstride];
  const int stride = gridDim.x * 256;
  double s1 = 0., s2 = 0.;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < rows; j += stride) {
    const double va = a[j], vab = ab[j];
    const double d = va - vab;
    s1 += (b[j] - f0) * (vab - va);
    s2 += d * d;
  }
  s1 = block_sum(s1, wsum);
  s2 = block_sum(s2, wsum);
  if (threadIdx.x == 0) {
    double* p = partial + (((size_t)k * D + col) * nslot + slot0 + blockIdx.x) * 2;
    p[0] = s1;
    p[1] = s2;
  }
}

// out[q * ostride + c] = scale * (sum of the nslot partials of quantity q, component c < ncomp), slots added in a fixed order:
// thread t takes slots t, t + 256, ... in ascending order, then the workgroup reduction above.  One workgroup per quantity.
__global__ __launch_bounds__(256) void sobol_final_kernel(const double* __restrict__ partial, long nslot, int ncomp, double scale,
                                                          double* __restrict__ out, long ostride) {
  __shared__ double wsum[4];
  const size_t q = blockIdx.x;
  for (int c = 0; c < ncomp; ++c) {
    double s = 0.;
    for (long t = threadIdx.x; t < nslot; t += 256) s += partial[(q * nslot + t) * ncomp + c];
    s = block_sum(s, wsum);
    if (threadIdx.x == 0) out[q * ostride + c] = scale * s;
  }
}

// workgroups of a reduction over m elements: about 2048 elements each, at most `cap`
int reduce_groups(long m, int cap) { return (int)std::max<long>(1, std::min<long>(cap, (m + 2047) / 2048)); }

}  // namespace

void launch_sobol_pick_freeze(const double* A, const double* B, long r0, int rows, int D, int col, double* out, hipStream_t s) {
  if (rows <= 0) return;
  const long total = (long)rows * D;
  const int g = (int)std::max<long>(1, std::min<long>(4096, (total + 1023) / 1024));
  prof_begin("sobol_pick_freeze", s);
  hipLaunchKernelGGL(sobol_pick_freeze_kernel, dim3(g), dim3(256), 0, s, A, B, r0, rows, D, col, out);
  prof_end("sobol_pick_freeze", s, 0., 16.0 * (double)total);
}

int sobol_groups(long m) { return reduce_groups(m, SOBOL_MAX_GROUPS); }

void launch_sobol_row_mean(int nb, int mode, const double* x, long ld, long m, const double* prm, int pstride, double* partial, double* out,
                           int ostride, hipStream_t s) {
  if (nb <= 0 || m <= 0) return;
  if (mode < 0 || mode > 2) throw std::runtime_error("sobol: unknown row reduction");
  const int g = sobol_groups(m);
  prof_begin("sobol_moments", s);
  if (mode == 0) hipLaunchKernelGGL(sobol_row_sum_kernel<0>, dim3(g, nb), dim3(256), 0, s, x, ld, m, prm, pstride, partial);
  else if (mode == 1) hipLaunchKernelGGL(sobol_row_sum_kernel<1>, dim3(g, nb), dim3(256), 0, s, x, ld, m, prm, pstride, partial);
  else hipLaunchKernelGGL(sobol_row_sum_kernel<2>, dim3(g, nb), dim3(256), 0, s, x, ld, m, prm, pstride, partial);
  hipLaunchKernelGGL(sobol_final_kernel, dim3(nb), dim3(256), 0, s, (const double*)partial, (long)g, 1, 1.0 / (double)m, out, (long)ostride);
  prof_end("sobol_moments", s, 0., 8.0 * (double)nb * (double)m);
}

void launch_sobol_pair_sum(int nb, const double* fA, const double* fB, long ld, const double* fAB, long ldab, int rows,
                           const double* stats, int sstride, double* partial, int D, int col, long nslot, long slot0, int groups,
                           hipStream_t s) {
  if (nb <= 0 || rows <= 0) return;
  if (groups < 1 || slot0 < 0 || slot0 + groups > nslot || col < 0 || col >= D) throw std::runtime_error("sobol: partial slots out of range");
  prof_begin("sobol_reduce", s);
  hipLaunchKernelGGL(sobol_pair_sum_kernel, dim3(groups, nb), dim3(256), 0, s, fA, fB, ld, fAB, ldab, rows, stats, sstride, partial, D, col,
                     nslot, slot0);
  prof_end("sobol_reduce", s, 0., 24.0 * (double)nb * (double)rows);
}

void launch_sobol_pair_final(int nq, const double* partial, long nslot, double scale, double* out, hipStream_t s) {
  if (nq <= 0) return;
  prof_begin("sobol_reduce", s);
  hipLaunchKernelGGL(sobol_final_kernel, dim3(nq), dim3(256), 0, s, partial, nslot, 2, scale, out, 2L);
  prof_end("sobol_reduce", s, 0., 16.0 * (double)nq * (double)nslot);
}

}  // namespace mogp
