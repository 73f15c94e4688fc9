// Host check of the Cholesky schedule choice (csrc/chol_schedule.h): reads one case per line from stdin --
//   nb NP matrix_bytes hook forced force_legacy
// -- and prints the schedule number choose_cholesky_schedule returns for it (tests/test_host_boundary.py holds the table).
#include <cstdio>

#include "chol_schedule.h"

int main() {
  int nb, NP, hook, forced, force_legacy;
  unsigned long long bytes;
  while (std::scanf("%d %d %llu %d %d %d", &nb, &NP, &bytes, &hook, &forced, &force_legacy) == 6)
    std::printf("%d\n", mogp::choose_cholesky_schedule(nb, NP, (std::size_t)bytes, hook, forced, force_legacy != 0));
  return 0;
}
