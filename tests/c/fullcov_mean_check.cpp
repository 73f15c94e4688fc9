// Host check of the analytic mean's terms of predict(full_cov=True) (csrc/hostmath.h, fullcov_mean_terms).  stdin: q m, beta (q),
// LA (q x q, row-major), Hs (q x m), dots ((1 + q) x m), C (m x m).  mu starts as row 0 of dots, as in Engine::predict_full_cov.
// stdout, one line each: mu (m), rm (q x m), C (m x m).
#include <cstdio>
#include <vector>

#include "hostmath.h"

static bool read(std::vector<double>& v) {
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}
static void print(const std::vector<double>& v) {
  for (double x : v) std::printf("%.17g ", x);
  std::printf("\n");
}

int main() {
  int q = 0, m = 0;
  if (std::scanf("%d %d", &q, &m) != 2 || q < 1 || m < 1) return 2;
  std::vector<double> beta(q), LA((size_t)q * q), Hs((size_t)q * m), dots((size_t)(1 + q) * m), C((size_t)m * m);
  if (!read(beta) || !read(LA) || !read(Hs) || !read(dots) || !read(C)) return 2;
  std::vector<double> mu(dots.begin(), dots.begin() + m), rm((size_t)q * m);
  mogp::fullcov_mean_terms(q, m, beta.data(), LA.data(), Hs.data(), dots.data(), mu.data(), rm.data(), C.data());
  print(mu);
  print(rm);
  print(C);
  return 0;
}
