// Cross-validation of a fitted emulator at its fitted hyperparameters (cross_validate): leave-one-out and k-fold predictive
// errors from what a fit leaves on the device, without refitting.  Q = sigma^2 C + eta I is the factored matrix, alpha = Q^-1 r.  For a
// fold F (an index set) with S = (Q^-1)_FF = L_S L_S^T and y = L_S^-1 alpha_F:
//   e_F = S^-1 alpha_F  (held-out error t_F - mu_-F(X_F)),   Sigma_F = S^-1  (held-out covariance of the observations, nugget included),
//   var_i = sum_k (L_S^-1)[k][i]^2,   mahalanobis_F = y^T y,   log_score_F = -1/2 y^T y + 1/2 log|S| - |F|/2 log 2 pi.
// Leave-one-out is |F| = 1: q_ii = sum_{k >= i} L^-1[k][i]^2, e_i = alpha_i / q_ii, var_i = 1 / q_ii -- one pass over L^-1 (cv_loo_kernel).
// k-fold: cv_gather_kernel writes S and alpha_F of every (emulator, fold) slot of a pass into the factor buffer of a sub-engine (launch.h
// layout), the engine's batched Cholesky, trtri, log-determinant and L^-T y launchers run on it, and cv_finish_kernel scatters the results
// to the caller-order rows.  Plain vector code: every output has one writer, the column sums are split over the four waves as in
// loo_variance_kernel and added in a fixed order, nothing is atomic -- the same call returns the same bits.
#include "launch.h"
#include "devmem.h"

namespace mogp {

namespace {

constexpr double HALF_LOG_2PI = 0.918938533204672741780329736406;

__device__ __forceinline__ double cv_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// One workgroup per 64 columns of L^-1 of slot blockIdx.y (emulator idx[slot]); out rows (slot, n), scalars (slot, k = n) at the point's label
__global__ __launch_bounds__(256) void cv_loo_kernel(BatchView v, const int* __restrict__ labels, const double* __restrict__ targets,
                                                     const double* __restrict__ eta, int include_nugget, double* __restrict__ mean,
                                                     double* __restrict__ var, double* __restrict__ maha, double* __restrict__ log_score,
                                                     int* __restrict__ ok) {
  __shared__ double red[4][64];
  const int slot = blockIdx.y;
  const int emu = v.idx ? v.idx[slot] : slot;
  const int ld = v.LD, n = v.n;
  const double* Li = v.Linv + (size_t)emu * v.MS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 64, i = i0 + lane;       // (i < NP: the columns of the last tile beyond n are read, in bounds, and dropped)
  double s = 0.;
#pragma unroll 8
  for (int k = i0 + wave; k < n; k += 4) {
    const double x = Li[(size_t)k * ld + i];
    s = __builtin_fma(x, x, s);
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0 || i >= n) return;
  const double q = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
  const double a = v.alpha[(size_t)emu * v.RA * ld + i];
  const double e = a / q, vi = 1.0 / q, m2 = a * e;
  const size_t o = (size_t)slot * n;
  mean[o + i] = targets[o + i] - e;
  var[o + i] = include_nugget ? vi : fmax(vi - eta[slot], 0.0);
  const int f = labels[i];
  maha[o + f] = m2;
  log_score[o + f] = -0.5 * m2 + 0.5 * log(q) - HALF_LOG_2PI;
  ok[o + f] = 1;
}

// Slot table of a pass, four ints per slot: { source emulator (engine index; -1: the slot is not used), caller row, fold, fold size }.
// folds (k, nsub): the training indices of every fold, -1 where a fold is shorter than nsub.
//
// One 64 x 64 tile of the factor matrix of slot blockIdx.z: thread (ty, tx) = (t >> 5, t & 31) owns rows 8 ty .. 8 ty + 7 and columns
// 2 tx, 2 tx + 1, so that one store instruction of a wave is two whole 512-byte rows of the tile (cov_build_kernel's shape).  The reads
// are gathers from the lower tiles of K^-1, mirrored on load.
__global__ __launch_bounds__(256) void cv_gather_kernel(BatchView v, const int* __restrict__ folds, const int* __restrict__ tab,
                                                        double* __restrict__ subA, int nsub, int NPsub) {
  __shared__ int fi[64], fj[64];
  const int* t = tab + 4 * blockIdx.z;
  const int emu = t[0], fold = t[2];
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  if (threadIdx.x < 128) {
    const int c = (threadIdx.x < 64 ? i0 : j0) + (threadIdx.x & 63);
    const int p = (emu >= 0 && c < nsub) ? folds[(size_t)fold * nsub + c] : -1;
    (threadIdx.x < 64 ? fi : fj)[threadIdx.x & 63] = p;
  }
  __syncthreads();
  const int ld = v.LD;
  const double* Kinv = v.Kinv + (size_t)max(emu, 0) * v.MS;
  const double* alpha = v.alpha + (size_t)max(emu, 0) * v.RA * ld;
  double* A = subA + (size_t)blockIdx.z * NPsub * NPsub;
  const int ty = threadIdx.x >> 5, tx = threadIdx.x & 31;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    const int r = 8 * ty + a, i = i0 + r;
    double out[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int c = 2 * tx + b, j = j0 + c;
      const int hi = max(i, j), lo = min(i, j);
      // the point at the smaller position (the only one there is when hi is the target row)
      const int plo = (i <= j) ? fi[r] : fj[c];
      double x;
      if (hi < nsub) {
        const int phi = (i <= j) ? fj[c] : fi[r];
        if (plo >= 0 && phi >= 0) x = Kinv[(size_t)max(plo, phi) * ld + min(plo, phi)];
        else x = (i == j) ? 1.0 : 0.0;                               // a missing point of a short fold: exactly neutral
      } else if (hi == nsub) {
        x = (lo == hi) ? PAD_BIG : (plo >= 0 ? alpha[plo] : 0.0);    // target row (and its mirror column)
      } else {
        x = (i == j) ? 1.0 : 0.0;
      }
      out[b] = x;
    }
    *reinterpret_cast<double2*>(A + (size_t)i * NPsub + j0 + 2 * tx) = make_double2(out[0], out[1]);
  }
}

// One workgroup per 64 columns of L_S^-1 of slot blockIdx.y: var_i = sum_k L_S^-1[k][i]^2 (loo_variance_kernel's split), e from the
// sub-engine's solution row; workgroup 0 of the slot also writes the fold's scalars from the sub-engine's log-determinant / Gram words.
// info[slot] != 0 (S did not factorise): NaN, ok = 0 -- and nothing of the slot's L^-1 is read.
__global__ __launch_bounds__(256) void cv_finish_kernel(const int* __restrict__ folds, const int* __restrict__ tab, const double* __restrict__ Linv,
                                                        const double* __restrict__ sol, const double* __restrict__ res,
                                                        const int* __restrict__ info, int nsub, int NPsub, const double* __restrict__ targets,
                                                        const double* __restrict__ eta, int include_nugget, int n, int k,
                                                        double* __restrict__ mean, double* __restrict__ var, double* __restrict__ maha,
                                                        double* __restrict__ log_score, int* __restrict__ ok) {
  __shared__ double red[4][64];
  const int slot = blockIdx.y;
  const int* t = tab + 4 * slot;
  const int row = t[1], fold = t[2], size = t[3];
  if (t[0] < 0) return;                                   // (uniform)
  const bool bad = info[slot] != 0;                       // (uniform)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = blockIdx.x * 64, i = i0 + lane;
  double s = 0.;
  if (!bad) {
    const double* Li = Linv + (size_t)slot * NPsub * NPsub;
#pragma unroll 8
    for (int r = i0 + wave; r < nsub; r += 4) {
      const double x = Li[(size_t)r * NPsub + i];
      s = __builtin_fma(x, x, s);
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave != 0) return;
  if (blockIdx.x == 0 && lane == 0) {
    const double* r = res + (size_t)slot * RES_STRIDE;
    const size_t o = (size_t)row * k + fold;
    maha[o] = bad ? cv_nan() : r[2];
    log_score[o] = bad ? cv_nan() : -0.5 * r[2] + 0.5 * r[0] - (double)size * HALF_LOG_2PI;
    ok[o] = bad ? 0 : 1;
  }
  if (i >= nsub) return;
  const int p = folds[(size_t)fold * nsub + i];
  if (p < 0) return;
  const size_t o = (size_t)row * n + p;
  const double vi = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
  mean[o] = bad ? cv_nan() : targets[o] - sol[(size_t)slot * NPsub + i];
  var[o] = bad ? cv_nan() : (include_nugget ? vi : fmax(vi - eta[row], 0.0));
}

}  // namespace

void launch_cv_loo(const BatchView& v, const int* labels, const double* targets, const double* eta, bool include_nugget, double* mean,
                   double* var, double* maha, double* log_score, int* ok, hipStream_t s) {
  if (v.nb <= 0) return;
  prof_begin("cv_loo", s);
  hipLaunchKernelGGL(cv_loo_kernel, dim3((v.n + 63) / 64, v.nb), dim3(256), 0, s, v, labels, targets, eta, include_nugget ? 1 : 0, mean, var,
                     maha, log_score, ok);
  HIPCK(hipGetLastError());
  prof_end("cv_loo", s, 0., (double)v.nb * v.n * v.n * 4.0);
}

void launch_cv_gather(const BatchView& v, const int* folds, const int* tab, int nslots, double* subA, int nsub, int NPsub, hipStream_t s) {
  if (nslots <= 0) return;
  prof_begin("cv_gather", s);
  hipLaunchKernelGGL(cv_gather_kernel, dim3(NPsub / 64, NPsub / 64, nslots), dim3(256), 0, s, v, folds, tab, subA, nsub, NPsub);
  HIPCK(hipGetLastError());
  prof_end("cv_gather", s, 0., (double)nslots * NPsub * NPsub * 8.0);
}

void launch_cv_finish(const int* folds, const int* tab, int nslots, const double* Linv, const double* sol, const double* res, const int* info,
                      int nsub, int NPsub, const double* targets, const double* eta, bool include_nugget, int n, int k, double* mean,
                      double* var, double* maha, double* log_score, int* ok, hipStream_t s) {
  if (nslots <= 0) return;
  prof_begin("cv_finish", s);
  hipLaunchKernelGGL(cv_finish_kernel, dim3((nsub + 63) / 64, nslots), dim3(256), 0, s, folds, tab, Linv, sol, res, info, nsub, NPsub, targets,
                     eta, include_nugget ? 1 : 0, n, k, mean, var, maha, log_score, ok);
  HIPCK(hipGetLastError());
  prof_end("cv_finish", s, 0., (double)nslots * nsub * nsub * 4.0);
}

}  // namespace mogp
