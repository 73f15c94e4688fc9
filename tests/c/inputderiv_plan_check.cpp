// Host check of the plan and the refusals of the input derivatives at large designs (csrc/predict_plan.h: inderiv_point_bytes,
// kinderiv_fixed_bytes, kinderiv_plan, rff_inderiv_plan) against figures worked out by hand; exits non-zero at the first that differs.
//   bytes of a point = 8 D (2 + 32):  272 at D 1, 816 at D 3, 2720 at D 10, 21 760 at D 80
//   fixed bytes      = 8 * 32 N for the panel of V:  256 000 at N 1000, 25 600 000 at N 10^5;  rff_fixed_bytes for the features
//   budget = half of the free bytes less the fixed ones
//     memory bound, product    m 10^6, D 80, N 10^5, free 2e8:  (1e8 - 25 600 000) / 21 760 = 3419.1 -> 3419 points
//     memory bound, features   m 10^6, D 80, F 65536, free 2e8: (1e8 - 59 244 544) / 21 760 = 1872.9 -> 1872 points
//   blocks = ceil(columns / 32), groups = ceil(D / 8)
// tests/test_inputderiv_host.py builds it with -fsanitize=address,undefined.
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

struct Row {
  const char* name;
  bool features;    // rff_inderiv_plan (size = F), else kinderiv_plan (size = N)
  long m;
  int D;
  long size, cols;
  double free_b;
  int max_points;
  bool refused;
  long points, blocks;
  int groups;
};

int main() {
  using namespace mogp;
  ++checks;
  if (INDERIV_DG != 8 || inderiv_point_bytes(1) != 272.0 || inderiv_point_bytes(3) != 816.0 || inderiv_point_bytes(10) != 2720.0 ||
      inderiv_point_bytes(80) != 21760.0 || kinderiv_fixed_bytes(1000) != 256000.0 || kinderiv_fixed_bytes(100000) != 25600000.0) {
    std::printf("FAILED the byte counts: %.0f %.0f %.0f %.0f %.0f %.0f\n", inderiv_point_bytes(1), inderiv_point_bytes(3), inderiv_point_bytes(10),
                inderiv_point_bytes(80), kinderiv_fixed_bytes(1000), kinderiv_fixed_bytes(100000));
    return 1;
  }
  const Row table[] = {
      {"timing shape, product", false, 10000, 10, 100000, 32, 1e11, 0, false, 10000, 1, 2},
      {"timing shape, features", true, 10000, 10, 1024, 32, 1e11, 0, false, 10000, 1, 2},
      {"one of everything", false, 1, 1, 1, 1, 1e11, 0, false, 1, 1, 1},
      {"a second block of columns", false, 37, 3, 130, 33, 1e11, 7, false, 7, 2, 1},
      {"eight dimensions: one group", false, 37, 8, 130, 16, 1e11, 0, false, 37, 1, 1},
      {"nine dimensions: two groups", true, 37, 9, 130, 17, 1e11, 0, false, 37, 1, 2},
      {"eighty dimensions: ten groups", false, 65, 80, 130, 1, 1e11, 64, false, 64, 1, 10},
      {"max_points one", true, 37, 3, 130, 32, 1e11, 1, false, 1, 1, 1},
      {"max_points above m", false, 37, 3, 130, 17, 1e11, 1000, false, 37, 1, 1},
      {"pass cap", false, 5000000, 2, 1000, 64, 1e11, 0, false, 1048576, 2, 1},
      {"memory bound, product", false, 1000000, 80, 100000, 32, 2e8, 0, false, 3419, 1, 10},
      {"memory bound, features", true, 1000000, 80, 65536, 32, 2e8, 0, false, 1872, 1, 10},
      {"max_points refused", false, 1000000, 80, 100000, 32, 2e8, 5000, true, 0, 0, 0},
      {"not one point, product", false, 10, 80, 100000, 1, 5.12e7, 0, true, 0, 0, 0},
      {"not one point, features", true, 10, 80, 65536, 1, 1e8, 0, true, 0, 0, 0},
  };
  for (const Row& r : table) {
    ++checks;
    InderivPlan p{0, 0, 0};
    bool threw = false;
    try {
      p = r.features ? rff_inderiv_plan("rff_inputderiv", r.m, r.D, (int)r.size, r.cols, r.free_b, r.max_points)
                     : kinderiv_plan("kmatvec_inputderiv", r.m, r.D, r.size, r.cols, r.free_b, r.max_points);
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (threw != r.refused) { std::printf("FAILED %s: refused %d, expected %d\n", r.name, (int)threw, (int)r.refused); return 1; }
    if (threw) continue;
    if (p.points != r.points || p.blocks != r.blocks || p.groups != r.groups) {
      std::printf("FAILED %s: points %ld blocks %ld groups %d\n", r.name, p.points, p.blocks, p.groups);
      return 1;
    }
    const double fixed = r.features ? rff_fixed_bytes(r.D, (int)r.size) : kinderiv_fixed_bytes(r.size);
    if (p.points < 1 || p.points > r.m || fixed + (double)p.points * inderiv_point_bytes(r.D) > 0.5 * r.free_b || p.blocks * ITER_PLAN_COLS < r.cols ||
        p.groups * INDERIV_DG < r.D || (p.groups - 1) * INDERIV_DG >= r.D) {
      std::printf("FAILED %s: the plan does not fit\n", r.name);
      return 1;
    }
  }
  if (!refuses([] { kinderiv_plan("kmatvec_inputderiv", 10, 2, 64, 1, 1e9, -1); }, "kmatvec_inputderiv: max_points must not be negative")) return 1;
  if (!refuses([] { rff_inderiv_plan("rff_inputderiv", 10, 2, 64, 1, 1e9, -1); }, "rff_inputderiv: max_points must not be negative")) return 1;
  for (long r : {0L, -3L})
    if (!refuses([&] { kinderiv_plan("kmatvec_inputderiv", 10, 2, 64, r, 1e9, 0); }, "kmatvec_inputderiv: at least one column is needed")) return 1;
  if (!refuses([] { kinderiv_plan("kmatvec_inputderiv", 1000000, 80, 100000, 32, 2e8, 5000); },
               "kmatvec_inputderiv: 5000 points per pass need more than half of the free device memory; use a smaller max_points"))
    return 1;
  if (!refuses([] { kinderiv_plan("kmatvec_inputderiv", 10, 80, 100000, 1, 5.12e7, 0); },
               "kmatvec_inputderiv: 25621760 bytes of device memory for a panel of 100000 rows and one point are more than half of the free device memory"))
    return 1;
  if (!refuses([] { rff_inderiv_plan("rff_inputderiv", 10, 80, 65536, 1, 1e8, 0); },
               "rff_inputderiv: 59266304 bytes of device memory for 65536 features and one point are more than half of the free device memory"))
    return 1;
  for (int F : {0, -1, 65537})
    if (!refuses([&] { rff_inderiv_plan("rff_inputderiv", 10, 2, F, 1, 1e9, 0); }, "rff_inputderiv: n_features must be between 1 and 65536")) return 1;
  if (!refuses([] { rff_inderiv_plan("rff_inputderiv", 10, 2, 64, 0, 1e9, 0); }, "rff_inputderiv: n_draws must be at least 1")) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
