// Host check of the plan and the refusals of the pathwise posterior draws (csrc/predict_plan.h: rff_check_counts, rff_fixed_bytes,
// rff_point_bytes, rff_plan) against figures worked out by hand; exits non-zero at the first that differs.
//   fixed bytes = 8 F (D + 1 + 32):  D 10, F 2048: 8 * 2048 * 43 = 704 512;   D 80, F 65536: 8 * 65536 * 113 = 59 244 544
//   bytes of a point = 8 (2 D + 32): 416 at D 10, 304 at D 3, 1536 at D 80;  budget = half of the free bytes less the fixed ones
//     memory bound   m 10^6, D 80, F 65536, free 2e8: (1e8 - 59 244 544) / 1536 = 26 533.5 -> 26 533 points
//   passes = ceil(S / 32)
// tests/test_pathwise_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <functional>
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
  int D, F;
  long S;
  double free_b;
  int max_points;
  bool refused;
  long points, passes;
};

int main() {
  using namespace mogp;
  ++checks;
  if (rff_fixed_bytes(10, 2048) != 704512.0 || rff_fixed_bytes(80, 65536) != 59244544.0 || rff_point_bytes(10) != 416.0 ||
      rff_point_bytes(3) != 304.0 || rff_point_bytes(80) != 1536.0) {
    std::printf("FAILED the byte counts: %.0f %.0f %.0f %.0f %.0f\n", rff_fixed_bytes(10, 2048), rff_fixed_bytes(80, 65536), rff_point_bytes(10),
                rff_point_bytes(3), rff_point_bytes(80));
    return 1;
  }
  const Row table[] = {
      {"timing shape", 10000, 10, 2048, 16, 1e11, 0, false, 10000, 1},
      {"one draw, one feature, one point", 1, 1, 1, 1, 1e11, 0, false, 1, 1},
      {"a second pass of draws", 37, 3, 130, 33, 1e11, 7, false, 7, 2},
      {"max_points one", 37, 3, 130, 32, 1e11, 1, false, 1, 1},
      {"max_points above m", 37, 3, 130, 17, 1e11, 1000, false, 37, 1},
      {"pass cap", 5000000, 10, 4096, 64, 1e11, 0, false, 1048576, 2},
      {"memory bound", 1000000, 80, 65536, 32, 2e8, 0, false, 26533, 1},
      {"max_points refused", 1000000, 80, 65536, 32, 2e8, 50000, true, 0, 0},
      {"not one point", 10, 80, 65536, 1, 1e8, 0, true, 0, 0},
  };
  for (const Row& r : table) {
    ++checks;
    RffPlan p{0, 0};
    bool threw = false;
    try {
      p = rff_plan("rff", r.m, r.D, r.F, r.S, r.free_b, r.max_points);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) continue;
    if (p.points != r.points || p.passes != r.passes) { std::printf("FAILED %s: points %ld passes %ld\n", r.name, p.points, p.passes); return 1; }
    if (p.points < 1 || p.points > r.m || rff_fixed_bytes(r.D, r.F) + (double)p.points * rff_point_bytes(r.D) > 0.5 * r.free_b ||
        p.passes * ITER_PLAN_COLS < r.S) {
      std::printf("FAILED %s: the plan does not fit\n", r.name);
      return 1;
    }
  }
  if (!refuses([] { rff_plan("rff", 10, 2, 64, 1, 1e9, -1); }, "rff: max_points must not be negative")) return 1;
  if (!refuses([] { rff_plan("rff", 1000000, 80, 65536, 32, 2e8, 50000); },
               "rff: 50000 points per pass need more than half of the free device memory; use a smaller max_points"))
    return 1;
  if (!refuses([] { rff_plan("rff", 10, 80, 65536, 1, 1e8, 0); },
               "rff: 59246080 bytes of device memory for 65536 features and one point are more than half of the free device memory"))
    return 1;
  for (long F : {1L, 64L, 65536L})
    if (!accepts([&] { rff_check_counts("sample_paths", F, 1, 0); }, "a feature count inside the range")) return 1;
  for (long F : {0L, -1L, 65537L})
    if (!refuses([&] { rff_check_counts("sample_paths", F, 1, 0); }, "sample_paths: n_features must be between 1 and 65536")) return 1;
  if (!refuses([] { rff_plan("rff", 10, 2, 0, 1, 1e9, 0); }, "rff: n_features must be between 1 and 65536")) return 1;
  for (long S : {0L, -4L})
    if (!refuses([&] { rff_check_counts("sample_paths", 64, S, 0); }, "sample_paths: n_draws must be at least 1")) return 1;
  if (!refuses([] { rff_check_counts("sample_paths", 64, 2, -1); }, "sample_paths: first_draw must not be negative")) return 1;
  if (!accepts([] { rff_check_counts("sample_paths", 64, 2, 2147483645L); }, "the last draw index")) return 1;
  if (!refuses([] { rff_check_counts("sample_paths", 64, 2, 2147483646L); }, "sample_paths: first_draw + n_draws must stay below 2^31")) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
