// Priors::d2logpdtheta2 of csrc/hostmath.h compiled for the host.  Input (stdin): D, nugget type, then per prior (D correlation, covariance,
// nugget) "type shape scale", then theta (D + 2 values).  Output: one line with the D + 1 (+ 1 when the nugget is fitted) second derivatives.
#include <cstdio>
#include <vector>
#include "hostmath.h"

int main() {
  int D, nug_type;
  if (std::scanf("%d %d", &D, &nug_type) != 2) return 2;
  mogp::Priors pr;
  pr.corr.resize(D);
  auto rd = [](mogp::Prior& p) { return std::scanf("%d %lf %lf", &p.type, &p.shape, &p.scale) == 3; };
  for (int d = 0; d < D; ++d)
    if (!rd(pr.corr[d])) return 2;
  if (!rd(pr.cov) || !rd(pr.nug)) return 2;
  pr.created = true;
  std::vector<double> th(D + 2), out(D + 2);
  for (double& x : th)
    if (std::scanf("%lf", &x) != 1) return 2;
  pr.d2logpdtheta2(th, D, nug_type, out.data());
  const int nd = D + 1 + (nug_type == mogp::NUG_FIT ? 1 : 0);
  for (int i = 0; i < nd; ++i) std::printf("%.17g ", out[i]);
  std::printf("\n");
  return 0;
}
