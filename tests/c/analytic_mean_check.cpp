// Host check of the analytic-mean algebra (csrc/hostmath.h, analytic_mean).  stdin: q n informative, the 8 x 8 Gram block G (row-major),
// and with informative = 1 the mean priors b (q), B^-1 (q x q), B^-1 b (q), log|B|.  stdout, one line each: ok, quad, logdetA, n_coeff,
// beta (q), LA (q x q), M ((q + 2) x 8); after ok = 0 only LA follows.
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
  constexpr int RMAX = 8;
  int q = 0, n = 0, informative = 0;
  if (std::scanf("%d %d %d", &q, &n, &informative) != 3 || q < 1 || q >= RMAX) return 2;
  std::vector<double> G(RMAX * RMAX), b, Binv, Binvb;
  double logdetB = 0.;
  if (!read(G)) return 2;
  if (informative) {
    b.resize(q); Binv.resize((size_t)q * q); Binvb.resize(q);
    if (!read(b) || !read(Binv) || !read(Binvb) || std::scanf("%lf", &logdetB) != 1) return 2;
  }
  mogp::AnalyticMean am;
  mogp::analytic_mean(G.data(), RMAX, q, n, b, Binv, Binvb, logdetB, am);
  std::printf("%d\n", am.ok ? 1 : 0);
  if (!am.ok) {
    print(am.LA);
    return 0;
  }
  std::printf("%.17g\n%.17g\n%d\n", am.quad, am.logdetA, am.n_coeff);
  print(am.beta);
  print(am.LA);
  print(am.M);
  return 0;
}
