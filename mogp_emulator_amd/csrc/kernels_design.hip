// Maximin Latin hypercube scoring (mogp_emulator/ExperimentalDesign.py:663-668): the smallest pairwise Euclidean distance of each of T
// candidate designs, every design an (n, D) row-major block of one (T, n, D) array.  One workgroup per (design, 64 x 64 tile of the lower
// triangle of the pair matrix, diagonal tiles included, where only i > j counts): the two 64-row blocks of the design are staged in LDS
// as the covariance kernels stage them (cov_dev.h stage_rows), every thread keeps the running minimum of the SQUARED distance of its
// 4 x 4 pairs, the waves reduce theirs by shuffles, and one vector atomic minimum per workgroup combines the workgroups of a design: the
// bit patterns of non-negative IEEE doubles are ordered as unsigned 64-bit integers, and a minimum does not depend on the order of its
// operands, so the result is the same bits in every run.  The square root is taken once, of the minimum (sqrt is monotone and
// correctly rounded: sqrt(min) == min(sqrt)).
// The squared distance is the sum over ascending d of the ROUNDED squares (contraction to FMA is off in this file's device sum): the
// value scipy's pdist computes wherever the host build does not fuse either.
#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>

#include "cov_dev.h"
#include "engine.h"

namespace mogp {

namespace {

constexpr unsigned long long INF_BITS = 0x7FF0000000000000ull;      // +infinity: above every finite squared distance

__global__ __launch_bounds__(256) void design_init_kernel(unsigned long long* __restrict__ best, int T) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < T) best[t] = INF_BITS;
}

__global__ __launch_bounds__(256) void design_min_r2_kernel(const double* __restrict__ X, int n, int D,
                                                            unsigned long long* __restrict__ best) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double wmin[4];
  const int tile = blockIdx.x;
  int ti = (int)((sqrt(8.0 * tile + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > tile) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const int i0 = ti * 64, j0 = tj * 64;
  const double* Xt = X + (size_t)blockIdx.y * n * D;
  double* si = sm;
  double* sj = sm + 64 * D;
  stage_rows(Xt, n, D, i0, si);
  stage_rows(Xt, n, D, j0, sj);
  __syncthreads();
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double r2[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
  for (int d = 0; d < D; ++d) {
    double xi[4], xj[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) xi[a] = si[d * 64 + 4 * ty + a];
#pragma unroll
    for (int b = 0; b < 4; ++b) xj[b] = sj[d * 64 + 4 * tx + b];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const double df = xi[a] - xj[b];
        const double sq = df * df;            // rounded on its own: no FMA (see the head of the file)
        r2[a][b] = r2[a][b] + sq;
      }
  }
  const double inf = __longlong_as_double((long long)INF_BITS);
  double m = inf;
  // INTERIOR: a tile strictly below the diagonal whose rows are all points of the design -- every pair counts
  if (ti > tj && i0 + 64 <= n) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) m = fmin(m, r2[a][b]);
  } else {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = i0 + 4 * ty + a, j = j0 + 4 * tx + b;
        if (i > j && i < n) m = fmin(m, r2[a][b]);
      }
  }
  // a NaN coordinate: fmin drops it, as np.min would not -- the caller passes finite designs (mogp_hip.h; the Python shim checks)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmin(fmin(wmin[0], wmin[1]), fmin(wmin[2], wmin[3]));
    if (m < inf) atomicMin(best + blockIdx.y, (unsigned long long)__double_as_longlong(m));      // m >= +0.0: a sum of squares from 0.0
  }
}

__global__ __launch_bounds__(256) void design_finish_kernel(const unsigned long long* __restrict__ best, int T, double* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < T) out[t] = sqrt(__longlong_as_double((long long)best[t]));
}

}  // namespace

void design_min_pdist(const double* designs, int T, int n, int D, double* out) {
  if (!designs || !out) throw std::runtime_error("design_min_pdist: null pointer");
  if (T < 1) throw std::runtime_error("design_min_pdist: at least one design is needed");
  if (n < 2) throw std::runtime_error("design_min_pdist: a design needs at least two points");
  if (D < 1 || D > MAX_D) throw std::runtime_error("design_min_pdist: number of input dimensions must be between 1 and " + std::to_string(MAX_D));
  const long nt = ((long)n + 63) / 64;
  const long ntiles = nt * (nt + 1) / 2;
  // one workgroup of 256 threads per tile: the launch must stay below 2^32 work-items in its first dimension
  static_assert((long)(DESIGN_MAX_N / 64) * (DESIGN_MAX_N / 64 + 1) / 2 <= (long)(std::numeric_limits<unsigned>::max() / 256), "grid too large");
  if (n > DESIGN_MAX_N)
    throw std::runtime_error("design_min_pdist: too many points in a design (at most " + std::to_string(DESIGN_MAX_N) + ")");
  const size_t per = (size_t)n * D * sizeof(double);
  // designs per pass: DESIGN_SCRATCH_BYTES of staged designs (one design where a single one is larger), at most DESIGN_MAX_PASS (grid.y)
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>({(size_t)T, DESIGN_SCRATCH_BYTES / per, (size_t)DESIGN_MAX_PASS}));
  DevBuf<double> dX((size_t)chunk * n * D), dOut(chunk);
  DevBuf<unsigned long long> dBest(chunk);
  hipStream_t st = nullptr;
  const size_t lds = (size_t)128 * D * sizeof(double);
  for (int t0 = 0; t0 < T; t0 += chunk) {
    const int nb = std::min(chunk, T - t0);
    HIPCK(hipMemcpyAsync(dX, designs + (size_t)t0 * n * D, (size_t)nb * per, hipMemcpyHostToDevice, st));
    prof_begin("design_min_pdist", st);
    hipLaunchKernelGGL(design_init_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, dBest.get(), nb);
    hipLaunchKernelGGL(design_min_r2_kernel, dim3((unsigned)ntiles, nb), dim3(256), lds, st, (const double*)dX.get(), n, D,
                       dBest.get());
    hipLaunchKernelGGL(design_finish_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, (const unsigned long long*)dBest.get(), nb, dOut.get());
    HIPCK(hipGetLastError());
    // algorithmic: a subtraction, a product and an addition per pair and dimension; every design read once
    prof_end("design_min_pdist", st, 1.5 * (double)nb * n * ((double)n - 1.0) * D, (double)nb * per);
    HIPCK(hipMemcpyAsync(out + t0, dOut, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
}

}  // namespace mogp
