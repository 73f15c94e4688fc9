// Host check of the sizing rules of the prediction family (csrc/predict_plan.h): reads one case per line from stdin --
//   chunk cap_bytes nb LD m                            -> predict_chunk_points
//   sobol cap_bytes D nb R mean_kind n_poly_terms N    -> sobol_chunk_rows
//   hess  budget per_bytes n_good                      -> hessian_group_size
//   stage nb m nbasis nterm qq                         -> MeanStage: o_basis o_dbasis o_coef o_la o_int total
//   icap                                               -> implausibility_cap_bytes
// -- and prints the result of each on a line of its own (tests/test_host_boundary.py holds the table).
#include <cstdio>
#include <cstring>

#include "predict_plan.h"

int main() {
  char rule[16];
  while (std::scanf("%15s", rule) == 1) {
    if (!std::strcmp(rule, "chunk")) {
      double cap;
      int nb, LD, m;
      if (std::scanf("%lf %d %d %d", &cap, &nb, &LD, &m) != 4) return 2;
      std::printf("%d\n", mogp::predict_chunk_points(cap, nb, LD, m));
    } else if (!std::strcmp(rule, "sobol")) {
      double cap;
      int D, nb, R, kind, nterms;
      long N;
      if (std::scanf("%lf %d %d %d %d %d %ld", &cap, &D, &nb, &R, &kind, &nterms, &N) != 7) return 2;
      std::printf("%ld\n", mogp::sobol_chunk_rows(cap, D, nb, R, kind, nterms, N));
    } else if (!std::strcmp(rule, "hess")) {
      double budget, per;
      unsigned long long n_good;
      if (std::scanf("%lf %lf %llu", &budget, &per, &n_good) != 3) return 2;
      std::printf("%llu\n", (unsigned long long)mogp::hessian_group_size(budget, per, (std::size_t)n_good));
    } else if (!std::strcmp(rule, "stage")) {
      int nb, m, nbasis, nterm, qq;
      if (std::scanf("%d %d %d %d %d", &nb, &m, &nbasis, &nterm, &qq) != 5) return 2;
      const mogp::MeanStage s(nb, m, nbasis, nterm, qq);
      std::printf("%zu %zu %zu %zu %zu %zu\n", s.o_basis, s.o_dbasis, s.o_coef, s.o_la, s.o_int, s.total);
    } else if (!std::strcmp(rule, "icap")) {
      std::printf("%.17g\n", mogp::implausibility_cap_bytes);
    } else {
      return 2;
    }
  }
  return 0;
}
