// Host check of vecchia_plan (csrc/predict_plan.h) against a table worked out by hand: exits non-zero at the first row that differs.
// Held for the whole design: 8 cols N + 4 N + 16 cols ceil(N / 1024) bytes, cols = D + 3 with the gradient, 1 without; a workgroup's scratch
// = 8 x 34816 = 278 528 bytes without the gradient, 8 x 51200 = 409 600 with it; budget = half of the free bytes; a full grid = 4 workgroups
// per compute unit (1024 at 256 compute units).
//   timing shape     N 10^6, D 10, gradient: 13 cols -> 104e6 + 4e6 + 16 x 13 x 977 = 108 203 216 bytes, + 1024 x 409 600 = 419 430 400
//                    one launch of 10^6 points (below the cap of 2^20), 1024 workgroups, 977 blocks
//   value only       the same without the gradient: 1 col -> 8e6 + 4e6 + 16 x 977 = 12 015 632 bytes
//   pass cap         N 5 x 10^6: 2^20 points a launch, 4883 blocks
//   few points       N 130: one launch, a workgroup per point, one block
//   max_points       7 of 130 -> launches of 7 with 7 workgroups; 1000 of 130 -> 130; 1 -> 1
//   block edge       N 1024 -> 1 block, N 1025 -> 2
//   refusals         the timing shape in 1e9 free bytes (527 633 616 needed > 5e8); negative max_points
//   no compute units reported -> 4 workgroups
// tests/test_vecchia_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <stdexcept>

#include "predict_plan.h"

struct Row {
  const char* name;
  long N;
  int D;
  bool grad;
  int n_cu;
  double free_b;
  int max_points;
  bool refused;
  long points;
  int grid;
  long blocks;
};

int main() {
  const double wg0 = 8.0 * 34816, wg1 = 8.0 * 51200;
  const Row table[] = {
      {"timing shape", 1000000, 10, true, 256, 1e11, 0, false, 1000000, 1024, 977},
      {"value only", 1000000, 10, false, 256, 1e11, 0, false, 1000000, 1024, 977},
      {"pass cap", 5000000, 10, true, 256, 1e11, 0, false, 1048576, 1024, 4883},
      {"few points", 130, 3, true, 256, 1e11, 0, false, 130, 130, 1},
      {"max_points", 130, 3, true, 256, 1e11, 7, false, 7, 7, 1},
      {"max_points one", 130, 3, false, 256, 1e11, 1, false, 1, 1, 1},
      {"max_points above N", 130, 3, true, 256, 1e11, 1000, false, 130, 130, 1},
      {"block edge", 1024, 2, true, 256, 1e11, 0, false, 1024, 1024, 1},
      {"block edge + 1", 1025, 2, true, 256, 1e11, 0, false, 1025, 1024, 2},
      {"memory refused", 1000000, 10, true, 256, 1e9, 0, true, 0, 0, 0},
      {"memory fits without the gradient", 1000000, 10, false, 256, 1e9, 0, false, 1000000, 1024, 977},
      {"no compute units reported", 100, 2, true, 0, 1e9, 0, false, 100, 4, 1},
  };
  for (const Row& r : table) {
    mogp::VecchiaPlan p{0, 0, 0};
    bool threw = false;
    try {
      p = mogp::vecchia_plan(r.N, r.D, r.grad, r.n_cu, r.free_b, r.max_points, r.grad ? wg1 : wg0);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) continue;
    if (p.points != r.points || p.grid != r.grid || p.blocks != r.blocks) {
      std::printf("FAILED %s: points %ld grid %d blocks %ld\n", r.name, p.points, p.grid, p.blocks);
      return 1;
    }
    if (p.points < 1 || p.grid < 1 || p.grid > p.points ||
        mogp::vecchia_fixed_bytes(r.N, r.D, r.grad) + (double)p.grid * (r.grad ? wg1 : wg0) > 0.5 * r.free_b) {
      std::printf("FAILED %s: the plan does not fit half of the free memory\n", r.name);
      return 1;
    }
  }
  if (mogp::vecchia_fixed_bytes(1000000, 10, true) != 108203216.0 || mogp::vecchia_fixed_bytes(1000000, 10, false) != 12015632.0 ||
      mogp::vecchia_blocks(1) != 1 || mogp::vecchia_blocks(1024) != 1 || mogp::vecchia_blocks(1025) != 2) {
    std::printf("FAILED the byte counts\n");
    return 1;
  }
  bool threw = false;
  try {
    mogp::vecchia_plan(10, 2, true, 256, 1e9, -1, wg1);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  if (!threw) { std::printf("FAILED negative max_points accepted\n"); return 1; }
  std::printf("ok %d rows\n", (int)(sizeof(table) / sizeof(table[0])));
  return 0;
}
