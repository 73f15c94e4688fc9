// Host check of hessian_assemble (csrc/hostmath.h): reads cases from the file named on the command line (or stdin) --
//   n D NC uniform nug_fit NPh eta
//   o (D + 3) | T ((D + 1)(D + 2)) | A (D D) | V (D NPh) | U (D NPh) | z (NPh) | alpha (n) | t (n) | dpr (P)
// -- and prints per case "ok P" or "nonfinite P" and the P x P block as Engine::hessian leaves it: the upper triangle written to both
// sides of a NaN-filled block of leading dimension P + 1 (a failed case stays NaN).  tests/test_hessian_host.py holds the cases.
#include <cmath>
#include <cstdio>
#include <vector>

#include "hostmath.h"

static bool read(std::vector<double>& v, size_t count) {
  v.resize(count);
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::freopen(argv[1], "r", stdin)) return 2;
  int n, D, NC, uniform, nug_fit, NPh;
  double eta;
  while (std::scanf("%d %d %d %d %d %d %lf", &n, &D, &NC, &uniform, &nug_fit, &NPh, &eta) == 7) {
    const int P = NC + 1 + (nug_fit ? 1 : 0), ld = P + 1;
    std::vector<double> o, T, A, V, U, z, al, t, dpr;
    if (!read(o, D + 3) || !read(T, (size_t)(D + 1) * (D + 2)) || !read(A, (size_t)D * D) || !read(V, (size_t)D * NPh) || !read(U, (size_t)D * NPh) ||
        !read(z, NPh) || !read(al, n) || !read(t, n) || !read(dpr, P))
      return 2;
    std::vector<double> Fd((size_t)(D + 2) * (D + 2)), Hm((size_t)P * P), H((size_t)ld * ld, std::nan(""));
    const bool ok = mogp::hessian_assemble(n, D, NC, uniform != 0, nug_fit != 0, eta, o.data(), T.data(), A.data(), V.data(), U.data(), NPh, z.data(),
                                           al.data(), t.data(), dpr.data(), Fd.data(), Hm.data());
    if (ok)
      for (int r = 0; r < P; ++r)
        for (int c = r; c < P; ++c) H[(size_t)r * ld + c] = H[(size_t)c * ld + r] = Hm[(size_t)r * P + c];
    std::printf("%s %d\n", ok ? "ok" : "nonfinite", P);
    for (int r = 0; r < P; ++r)
      for (int c = 0; c < P; ++c) std::printf("%.17g%c", H[(size_t)r * ld + c], c + 1 < P ? ' ' : '\n');
  }
  return 0;
}
