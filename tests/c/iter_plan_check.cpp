// Host check of the plan and the refusals of the iterative exact prediction (csrc/predict_plan.h: iter_held_bytes, iter_check_memory,
// iter_plan, iter_check_hyper, iter_check_rank, iter_check_solve) against figures worked out by hand; exits non-zero at the first that differs.
//   held doubles = N p + 2 p^2 + 257 N + 32 (ceil(N / 4096) p + 2 p + ceil(N / 1024)) + 2 ceil(N / 1024)
//     N 10^5, p 1024:  102 400 000 + 2 097 152 + 25 700 000 + 32 (25 600 + 2 048 + 98) + 196 = 131 085 220  -> 1 048 681 760 bytes
//     N 300, p 64:     19 200 + 8 192 + 77 100 + 32 (64 + 128 + 1) + 2 = 110 670                            ->       885 360 bytes
//     N 1000, p 0:     257 000 + 32 + 2 = 257 034                                                           ->     2 056 272 bytes
//   bytes of a query = 8 (2 D + 16): 288 at D 10, 176 at D 3, 1408 at D 80; budget = half of the free bytes; blocks = ceil(points / 32)
//     memory bound     m 10^6, D 80, free 1e8: 5e7 / 1408 = 35 511.36 -> 35 511 queries, 1 110 blocks
// tests/test_iterative_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>

#include "predict_plan.h"

static int checks = 0;

static bool refuses(const std::function<void()>& f, const std::string& text) {
  ++checks;
  try {
    f();
  } catch (const std::runtime_error& e) {
    if (text == e.what()) return true;
    std::printf("FAILED wrong message: got \"%s\", expected \"%s\"\n", e.what(), text.c_str());
    return false;
  }
  std::printf("FAILED accepted, expected \"%s\"\n", text.c_str());
  return false;
}

static bool accepts(const std::function<void()>& f, const char* what) {
  ++checks;
  try {
    f();
  } catch (const std::runtime_error& e) {
    std::printf("FAILED %s refused: %s\n", what, e.what());
    return false;
  }
  return true;
}

struct Row {
  const char* name;
  long m;
  int D;
  double free_b;
  int max_points;
  bool refused;
  long points, blocks;
};

int main() {
  using namespace mogp;
  // the memory held
  ++checks;
  if (iter_held_bytes(100000, 1024) != 1048681760.0 || iter_held_bytes(300, 64) != 885360.0 || iter_held_bytes(1000, 0) != 2056272.0) {
    std::printf("FAILED the held bytes: %.0f %.0f %.0f\n", iter_held_bytes(100000, 1024), iter_held_bytes(300, 64), iter_held_bytes(1000, 0));
    return 1;
  }
  if (!accepts([] { iter_check_memory("predict_exact", 100000, 1024, 2.0 * 1048681760.0, 0.); }, "exactly half of the free memory")) return 1;
  if (!refuses([] { iter_check_memory("predict_exact", 100000, 1024, 2.0 * 1048681760.0 - 2., 0.); },
               "predict_exact: 1048681760 bytes of device memory for 100000 points at preconditioner rank 1024 are more than half of the free device memory"))
    return 1;
  // what the handle holds already counts as free
  if (!accepts([] { iter_check_memory("predict_exact", 100000, 1024, 1048681760.0, 1048681760.0); }, "memory the handle holds already")) return 1;
  if (!refuses([] { iter_check_memory("precondition", 300, 64, 1e6, 0.); },
               "precondition: 885360 bytes of device memory for 300 points at preconditioner rank 64 are more than half of the free device memory"))
    return 1;
  // the passes
  const Row table[] = {
      {"timing shape", 10000, 10, 1e11, 0, false, 10000, 313},
      {"few queries", 37, 3, 1e11, 0, false, 37, 2},
      {"max_points", 37, 3, 1e11, 7, false, 7, 1},
      {"max_points one", 37, 3, 1e11, 1, false, 1, 1},
      {"max_points above m", 37, 3, 1e11, 1000, false, 37, 2},
      {"exactly one block", 32, 3, 1e11, 0, false, 32, 1},
      {"pass cap", 5000000, 10, 1e11, 0, false, 1048576, 32768},
      {"memory bound", 1000000, 80, 1e8, 0, false, 35511, 1110},
      {"max_points refused", 1000000, 80, 1e8, 50000, true, 0, 0},
      {"not one query", 10, 80, 2000., 0, true, 0, 0},
  };
  for (const Row& r : table) {
    ++checks;
    IterPlan p{0, 0};
    bool threw = false;
    try {
      p = iter_plan("predict_exact", r.m, r.D, r.free_b, r.max_points);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) continue;
    if (p.points != r.points || p.blocks != r.blocks) { std::printf("FAILED %s: points %ld blocks %ld\n", r.name, p.points, p.blocks); return 1; }
    if (p.points < 1 || p.points > r.m || (double)p.points * iter_point_bytes(r.D) > 0.5 * r.free_b || p.blocks * ITER_PLAN_COLS < p.points) {
      std::printf("FAILED %s: the plan does not fit\n", r.name);
      return 1;
    }
  }
  ++checks;
  if (iter_point_bytes(10) != 288.0 || iter_point_bytes(3) != 176.0 || iter_point_bytes(80) != 1408.0) { std::printf("FAILED the byte counts\n"); return 1; }
  if (!refuses([] { iter_plan("predict_exact", 10, 2, 1e9, -1); }, "predict_exact: max_points must not be negative")) return 1;
  if (!refuses([] { iter_plan("predict_exact", 1000000, 80, 1e8, 50000); },
               "predict_exact: 50000 queries per pass need more than half of the free device memory; use a smaller max_points"))
    return 1;
  if (!refuses([] { iter_plan("predict_exact", 10, 80, 2000., 0); }, "predict_exact: one query does not fit half of the free device memory")) return 1;
  // the refusals
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double s3[3] = {1.0, 0.5, 2.0};
  if (!accepts([&] { iter_check_hyper("precondition", 3, s3, 1.1, 1e-4); }, "good hyperparameters")) return 1;
  for (double nug : {0.0, -0.0})
    if (!refuses([&] { iter_check_hyper("precondition", 3, s3, 1.1, nug); }, "precondition: the nugget must be positive (the preconditioner divides by it)"))
      return 1;
  for (double nug : {-1e-4, inf, nan})
    if (!refuses([&] { iter_check_hyper("solve", 3, s3, 1.1, nug); }, "solve: sigma^2 must be positive and finite, nugget and jitter finite and not negative"))
      return 1;
  for (double sig : {0.0, -1.0, inf, nan})
    if (!refuses([&] { iter_check_hyper("solve", 3, s3, sig, 1e-4); }, "solve: sigma^2 must be positive and finite, nugget and jitter finite and not negative"))
      return 1;
  for (double bad : {0.0, -1.0, inf, nan}) {
    const double sb[3] = {1.0, bad, 2.0};
    if (!refuses([&] { iter_check_hyper("kmatvec", 3, sb, 1.1, 1e-4); }, "kmatvec: the scales must be positive and finite")) return 1;
  }
  for (int rank : {0, 1, 64, 300})
    if (!accepts([&] { iter_check_rank("precondition", 300, rank); }, "a rank up to N")) return 1;
  for (int rank : {-1, 301, 1024})
    if (!refuses([&] { iter_check_rank("precondition", 300, rank); }, "precondition: precond_rank must be between 0 and min(N, 1024) = 300")) return 1;
  if (!accepts([] { iter_check_rank("precondition", 100000, 1024); }, "rank 1024")) return 1;
  if (!refuses([] { iter_check_rank("precondition", 100000, 1025); }, "precondition: precond_rank must be between 0 and min(N, 1024) = 1024")) return 1;
  if (!accepts([] { iter_check_solve("solve", 1, 1e-8, 1); }, "one column, one iteration")) return 1;
  for (long c : {0L, -3L})
    if (!refuses([&] { iter_check_solve("solve", c, 1e-8, 10); }, "solve: at least one right-hand side is needed")) return 1;
  for (double rtol : {0.0, 1.0, -1e-8, 2.0, inf, nan})
    if (!refuses([&] { iter_check_solve("solve", 2, rtol, 10); }, "solve: rtol must lie between 0 and 1 (both excluded)")) return 1;
  for (int it : {0, -5})
    if (!refuses([&] { iter_check_solve("solve", 2, 1e-8, it); }, "solve: max_iter must be at least 1")) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
