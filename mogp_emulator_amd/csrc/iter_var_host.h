// The small dense arithmetic of the variance bound's cache (engine_iter.hip IterSolver::var_build), on the host: matrices of the order of the
// preconditioner's rank (<= 1024), row-major, plain loops in one fixed order.  Host code only; tests/c/iter_var_host_check.cpp checks it.
//
//   prefix_cholesky      G[:r, :r] = C C^T in NATURAL column order, stopped at the first column whose pivot is not above `floor`: the rank
//                        r it returns makes every smaller rank a prefix of it.  (No pivoting: the columns of the factor it is applied to
//                        are ordered by importance already.)
//   upper_inverse        T = C^-T, upper triangular: right-multiplying by it orthonormalises, M T has M^T M -> I when M^T M = C C^T
//   right_multiply_upper Out = M T for a tall M, every entry summed over s in ascending order -- what the device's tri_right_kernel computes
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace mogp {

// the first prefix stops at a pivot <= ITER_VAR_TAU G[0][0]: what is left of a column of L there is rounding noise of the columns before it
constexpr double ITER_VAR_TAU = 1e-10;

// G (n, n) symmetric, ld n; C (n, n), ld n: rows < r hold the lower triangular factor, everything else is zero.  Returns r.
inline int prefix_cholesky(const double* G, int n, double floor, std::vector<double>& C) {
  C.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    double* ci = &C[(size_t)i * n];
    for (int j = 0; j <= i; ++j) {
      const double* cj = &C[(size_t)j * n];
      double s = G[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s -= ci[k] * cj[k];
      if (i == j) {
        if (!(s > floor) || !std::isfinite(s)) {
          for (int k = 0; k < i; ++k) ci[k] = 0.0;
          return i;
        }
        ci[j] = std::sqrt(s);
      } else {
        ci[j] = s / cj[j];
      }
    }
  }
  return n;
}

// T (r, r) with row stride ldt >= r: T[s][c] = (C^-T)[s][c] for s <= c, zero below the diagonal and in the columns r .. ldt - 1.
// C: the factor of prefix_cholesky with row stride ldc.
inline void upper_inverse(const double* C, int ldc, int r, std::vector<double>& T, int ldt) {
  T.assign((size_t)std::max(r, 1) * ldt, 0.0);
  for (int j = 0; j < r; ++j) {                   // row j of T is column j of C^-1: forward substitution on e_j
    double* u = &T[(size_t)j * ldt];
    for (int i = j; i < r; ++i) {
      const double* ci = &C[(size_t)i * ldc];
      double s = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= ci[k] * u[k];
      u[i] = s / ci[i];
    }
  }
}

// Out (N, r) = M (N, r) T, row-major with row strides ldm and ldo; T as upper_inverse leaves it
inline void right_multiply_upper(const double* M, long N, int ldm, const double* T, int ldt, int r, double* Out, int ldo) {
  for (long i = 0; i < N; ++i)
    for (int c = 0; c < r; ++c) {
      double s = 0.0;
      for (int k = 0; k <= c; ++k) s = std::fma(M[(size_t)i * ldm + k], T[(size_t)k * ldt + c], s);
      Out[(size_t)i * ldo + c] = s;
    }
}

}  // namespace mogp
