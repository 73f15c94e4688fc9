// Host check of the sizing rules of the prediction family (csrc/predict_plan.h): reads one case per line from stdin --
//   chunk cap_bytes nb LD m                            -> predict_chunk_points
//   sobol cap_bytes D nb R mean_kind n_poly_terms N    -> sobol_chunk_rows
//   hess  budget per_bytes n_good                      -> hessian_group_size
//   stage nb m nbasis nterm qq                         -> MeanStage: o_basis o_dbasis o_coef o_la o_int total
//   icap                                               -> implausibility_cap_bytes
//   hscr  NPh D TG PGR                                 -> hessian_scratch_bytes
//   half  free_bytes bytes_per_slot                    -> slots_in_half_of
//   rslot MS LD NP TILE                                -> replica_slot_bytes replica_slot_bound
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
    } else if (!std::strcmp(rule, "hscr")) {
      int NPh, D, TG, PGR;
      if (std::scanf("%d %d %d %d", &NPh, &D, &TG, &PGR) != 4) return 2;
      std::printf("%.17g\n", mogp::hessian_scratch_bytes(NPh, D, TG, PGR));
    } else if (!std::strcmp(rule, "half")) {
      double free_b, per;
      if (std::scanf("%lf %lf", &free_b, &per) != 2) return 2;
      std::printf("%ld\n", mogp::slots_in_half_of(free_b, per));
    } else if (!std::strcmp(rule, "rslot")) {
      unsigned long long MS;
      int LD, NP, TILE;
      if (std::scanf("%llu %d %d %d", &MS, &LD, &NP, &TILE) != 4) return 2;
      std::printf("%.17g %ld\n", mogp::replica_slot_bytes((std::size_t)MS, LD), mogp::replica_slot_bound(NP, TILE));
    } else if (!std::strcmp(rule, "icap")) {
      std::printf("%.17g\n", mogp::implausibility_cap_bytes);
    } else {
      return 2;
    }
  }
  return 0;
}
