// Host check of csrc/iter_var_host.h: the prefix Cholesky on a rank-deficient Gram matrix, the inverse of its factor and the triangular
// product, against properties that hold whatever the rounding (to a stated tolerance) and against a plain product; exits non-zero at the
// first that fails.  tests/test_variance_bound_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "iter_var_host.h"

static int checks = 0;

static bool check(bool ok, const char* what) {
  ++checks;
  if (!ok) std::printf("FAILED %s\n", what);
  return ok;
}

int main() {
  using namespace mogp;
  const int N = 40, n = 6;
  // B (N, n): a fixed pattern of full rank, then column 4 made a combination of columns 0 and 2
  std::vector<double> B((size_t)N * n);
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < n; ++c) B[(size_t)i * n + c] = std::sin(1.0 + 0.7 * i * (c + 1)) + (i == c ? 2.0 : 0.0);
  for (int i = 0; i < N; ++i) B[(size_t)i * n + 4] = B[(size_t)i * n + 0] - 2.0 * B[(size_t)i * n + 2];
  std::vector<double> G((size_t)n * n, 0.0);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      for (int i = 0; i < N; ++i) G[(size_t)a * n + b] += B[(size_t)i * n + a] * B[(size_t)i * n + b];
  std::vector<double> C;
  const int r = prefix_cholesky(G.data(), n, ITER_VAR_TAU * G[0], C);
  if (!check(r == 4, "the prefix stops at the dependent column")) return 1;
  double worst = 0.0;
  for (int a = 0; a < r; ++a)
    for (int b = 0; b < r; ++b) {
      double s = 0.0;
      for (int k = 0; k < r; ++k) s += C[(size_t)a * n + k] * C[(size_t)b * n + k];
      worst = std::fmax(worst, std::fabs(s - G[(size_t)a * n + b]));
    }
  if (!check(worst <= 1e-12 * G[0], "C C^T is the leading block")) return 1;
  bool zero = true;
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      if ((a >= r || b > a) && C[(size_t)a * n + b] != 0.0) zero = false;
  if (!check(zero, "nothing is stored outside the factor")) return 1;
  // a prefix: the factor of the leading 3 x 3 block is the leading block of the factor, bit for bit
  std::vector<double> G3(9), C3;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) G3[(size_t)a * 3 + b] = G[(size_t)a * n + b];
  bool same = prefix_cholesky(G3.data(), 3, 0.0, C3) == 3;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) same = same && C3[(size_t)a * 3 + b] == C[(size_t)a * n + b];
  if (!check(same, "the factor of a leading block is a leading block of the factor")) return 1;
  std::vector<double> I2 = {2.0, 1.0, 1.0, 2.0}, C2;
  if (!check(prefix_cholesky(I2.data(), 2, 0.0, C2) == 2, "a positive definite matrix reaches its order")) return 1;
  std::vector<double> Z2 = {0.0, 0.0, 0.0, 1.0};
  if (!check(prefix_cholesky(Z2.data(), 2, 0.0, C2) == 0 && C2[0] == 0.0 && C2[3] == 0.0, "a non-positive first pivot gives rank 0")) return 1;
  // T = C^-T with a row stride of 8: C^T T = I, zeros below the diagonal and in the padding
  const int ldt = 8;
  std::vector<double> T;
  upper_inverse(C.data(), n, r, T, ldt);
  worst = 0.0;
  bool shape = T.size() == (size_t)r * ldt;
  for (int a = 0; a < r; ++a)
    for (int b = 0; b < ldt; ++b) {
      if ((b < a || b >= r) && T[(size_t)a * ldt + b] != 0.0) shape = false;
      if (b >= r) continue;
      double s = 0.0;                                  // (C^T T)_ab = sum_k C_ka T_kb
      for (int k = 0; k < r; ++k) s += C[(size_t)k * n + a] * T[(size_t)k * ldt + b];
      worst = std::fmax(worst, std::fabs(s - (a == b ? 1.0 : 0.0)));
    }
  if (!check(shape && worst <= 1e-13, "T is the upper triangular inverse of C^T")) return 1;
  // Q = B[:, :r] T has orthonormal columns, and equals the plain product
  std::vector<double> Q((size_t)N * r);
  right_multiply_upper(B.data(), N, n, T.data(), ldt, r, Q.data(), r);
  worst = 0.0;
  for (int a = 0; a < r; ++a)
    for (int b = 0; b < r; ++b) {
      double s = 0.0;
      for (int i = 0; i < N; ++i) s += Q[(size_t)i * r + a] * Q[(size_t)i * r + b];
      worst = std::fmax(worst, std::fabs(s - (a == b ? 1.0 : 0.0)));
    }
  if (!check(worst <= 1e-12, "B T has orthonormal columns")) return 1;
  worst = 0.0;
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < r; ++c) {
      double s = 0.0, mag = 0.0;
      for (int k = 0; k < r; ++k) {
        s += B[(size_t)i * n + k] * T[(size_t)k * ldt + c];
        mag += std::fabs(B[(size_t)i * n + k] * T[(size_t)k * ldt + c]);
      }
      worst = std::fmax(worst, std::fabs(s - Q[(size_t)i * r + c]) / (mag + 1e-300));
    }
  if (!check(worst <= 8 * 2.3e-16, "the triangular product is the plain product")) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
