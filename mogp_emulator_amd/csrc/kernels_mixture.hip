// Mixture prediction over hyperparameter samples (predict_mixture): the reduction over samples behind the batched prediction.
// With normalised weights w_s, predictive means mu_s and variances v_s of the S samples of one emulator at one query point, and the
// pivot mu_0 (the mean of the first sample that factorised), d_s = mu_s - mu_0:
//   mean = mu_0 + sum w_s d_s,   within = sum w_s v_s,   between = max(sum w_s d_s^2 - (sum w_s d_s)^2, 0)      (law of total variance)
// The samples of an emulator arrive over several passes (slot groups) and the points over several chunks, so the three sums live in
// device memory, (E, 3, m) doubles, between the passes.  Both kernels are streaming: one thread per (emulator, point), consecutive
// threads on consecutive points, so every load and store of a wave is one contiguous 512-byte run; no LDS, no waits, no atomics.
// A point's sums are updated in slot (= sample) order with one rounded multiply and one rounded add per sample: contraction to FMA is
// off in this file, so the bits do not depend on what the compiler prefers, nor on the pass or chunk a sample or a point falls into.
#include "launch.h"
#include "devmem.h"

namespace mogp {

namespace {

__global__ __launch_bounds__(256) void mixture_accumulate_kernel(const double* __restrict__ mu, const double* __restrict__ var, long ld,
                                                                 int mc, const int* __restrict__ etab, const int* __restrict__ rows,
                                                                 const double* __restrict__ prm, double* __restrict__ acc,
                                                                 double* __restrict__ pivot, long m, long c0) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= mc) return;
  const int* t = etab + 4 * blockIdx.y;
  const int e = t[0], first = t[1], cnt = t[2], prow = t[3];
  const size_t pt = (size_t)c0 + j;
  double* pv = pivot + (size_t)e * m + pt;
  double mu0;
  if (prow >= 0) {
    mu0 = mu[(size_t)prow * ld + j];
    *pv = mu0;
  } else {
    mu0 = *pv;
  }
  double* a = acc + (size_t)e * 3 * m + pt;
  double s1 = a[0], s2 = a[m], s3 = a[2 * m];
  for (int k = first; k < first + cnt; ++k) {
    const int r = rows[k];
    if (r < 0) continue;                      // the sample did not factorise: weight 0, and its row does not exist
    const double w = prm[2 * k], nug = prm[2 * k + 1];
    const double d = mu[(size_t)r * ld + j] - mu0;
    const double v = fmax(var[(size_t)r * ld + j] + nug, 0.0);
    const double wd = w * d;
    const double wv = w * v;
    const double dd = d * d;
    const double wdd = w * dd;
    s1 = s1 + wd;
    s2 = s2 + wv;
    s3 = s3 + wdd;
  }
  a[0] = s1;
  a[m] = s2;
  a[2 * m] = s3;
}

__global__ __launch_bounds__(256) void mixture_finalise_kernel(long m, const int* __restrict__ alive, const double* __restrict__ pivot,
                                                               double* __restrict__ acc) {
#pragma clang fp contract(off)
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int e = blockIdx.y;
  double* a = acc + (size_t)e * 3 * m + j;
  if (!alive[e]) {
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    a[0] = nan;
    a[m] = nan;
    a[2 * m] = nan;
    return;
  }
  const double s1 = a[0];
  const double sq = s1 * s1;
  a[0] = pivot[(size_t)e * m + j] + s1;
  a[2 * m] = fmax(a[2 * m] - sq, 0.0);
}

}  // namespace

void launch_mixture_accumulate(const double* mu, const double* var, long ld, int mc, int nemu, const int* etab, const int* rows,
                               const double* prm, double* acc, double* pivot, long m, long c0, hipStream_t s) {
  if (mc <= 0 || nemu <= 0) return;
  prof_begin("mixture_accumulate", s);
  hipLaunchKernelGGL(mixture_accumulate_kernel, dim3((mc + 255) / 256, nemu), dim3(256), 0, s, mu, var, ld, mc, etab, rows, prm, acc, pivot,
                     m, c0);
  HIPCK(hipGetLastError());
  prof_end("mixture_accumulate", s, 0., 0.);
}

void launch_mixture_finalise(int E, long m, const int* alive, const double* pivot, double* acc, hipStream_t s) {
  if (E <= 0 || m <= 0) return;
  hipLaunchKernelGGL(mixture_finalise_kernel, dim3((unsigned)((m + 255) / 256), E), dim3(256), 0, s, m, alive, pivot, acc);
  HIPCK(hipGetLastError());
}

}  // namespace mogp
