// Host check of the padding rule of the factorisation and the triangular inverse (csrc/chol_schedule.h, real_rows): reads one case per
// line from stdin --
//   n_real row0 rows
// -- and prints the number of rows of the tile [row0, row0 + rows) that real_rows counts as real (tests/test_padding_host.py holds the
// hand-written table).  tests/test_padding_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>

#include "chol_schedule.h"

// (the rule is a constant expression: the device code may use it in one)
static_assert(mogp::real_rows(2001, 1984, 64) == 32, "last row tile of n = 2000");
static_assert(mogp::real_rows(2001, 2048, 64) == 0, "a tile behind the matrix");

int main() {
  int n_real, row0, rows;
  while (std::scanf("%d %d %d", &n_real, &row0, &rows) == 3) std::printf("%d\n", mogp::real_rows(n_real, row0, rows));
  return 0;
}
