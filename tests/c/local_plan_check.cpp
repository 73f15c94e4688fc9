// Host check of local_plan (csrc/predict_plan.h) against a table worked out by hand: exits non-zero at the first row that differs.
// bytes of a query = 8 (2 D + 3) + 4 (k + 1); a workgroup's scratch = 8 x 34816 = 278 528 bytes; budget = half of the free bytes;
// a full grid = 4 workgroups per compute unit (1024 at 256 compute units: 285 212 672 bytes of scratch).
//   timing shape     m 10^4, D 10, k 64 (444 bytes a query), free 1e11: everything in one pass, 1024 workgroups
//   few queries      m 37, D 3, k 8 (108 bytes): one pass, a workgroup per query
//   max_points       7 of 37 -> passes of 7 with 7 workgroups; 1000 of 37 -> 37
//   pass cap         m 5 x 10^6: 2^20 queries a pass
//   memory bound     m 10^6, D 80, k 126 (1812 bytes), free 1e9: (5e8 - 285 212 672) / 1812 = 118 536.05 -> 118 536
//   refusals         the same shape with max_points 500 000 (906e6 bytes of queries); a full grid's scratch in 2.5e8 bytes
//   no compute units reported -> 4 workgroups
// tests/test_local_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <stdexcept>

#include "predict_plan.h"

struct Row {
  const char* name;
  long m;
  int D, k, n_cu;
  double free_b;
  int max_points;
  bool refused;
  long points;
  int grid;
};

int main() {
  const double wg = 8.0 * 34816;
  const Row table[] = {
      {"timing shape", 10000, 10, 64, 256, 1e11, 0, false, 10000, 1024},
      {"few queries", 37, 3, 8, 256, 1e11, 0, false, 37, 37},
      {"max_points", 37, 3, 8, 256, 1e11, 7, false, 7, 7},
      {"max_points one", 37, 3, 8, 256, 1e11, 1, false, 1, 1},
      {"max_points above m", 37, 3, 8, 256, 1e11, 1000, false, 37, 37},
      {"pass cap", 5000000, 10, 64, 256, 1e11, 0, false, 1048576, 1024},
      {"memory bound", 1000000, 80, 126, 256, 1e9, 0, false, 118536, 1024},
      {"max_points refused", 1000000, 80, 126, 256, 1e9, 500000, true, 0, 0},
      {"scratch refused", 1000000, 10, 64, 256, 5e8, 0, true, 0, 0},
      {"no compute units reported", 100, 2, 5, 0, 1e9, 0, false, 100, 4},
  };
  for (const Row& r : table) {
    mogp::LocalPlan p{0, 0};
    bool threw = false;
    try {
      p = mogp::local_plan(r.m, r.D, r.k, r.n_cu, r.free_b, r.max_points, wg);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) continue;
    if (p.points != r.points || p.grid != r.grid) { std::printf("FAILED %s: points %ld grid %d\n", r.name, p.points, p.grid); return 1; }
    if (p.points < 1 || p.grid < 1 || p.grid > p.points || (double)p.points * mogp::local_point_bytes(r.D, r.k) + (double)p.grid * wg > 0.5 * r.free_b) {
      std::printf("FAILED %s: the plan does not fit half of the free memory\n", r.name);
      return 1;
    }
  }
  if (mogp::local_point_bytes(10, 64) != 444.0 || mogp::local_point_bytes(3, 8) != 108.0 || mogp::local_point_bytes(80, 126) != 1812.0) {
    std::printf("FAILED the byte counts\n");
    return 1;
  }
  bool threw = false;
  try {
    mogp::local_plan(10, 2, 5, 256, 1e9, -1, wg);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  if (!threw) { std::printf("FAILED negative max_points accepted\n"); return 1; }
  std::printf("ok %d rows\n", (int)(sizeof(table) / sizeof(table[0])));
  return 0;
}
