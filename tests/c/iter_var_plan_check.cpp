// Host check of the bytes, the memory refusal and the refusal texts of the variance bound (csrc/predict_plan.h: iter_var_pad, iter_var_bytes,
// iter_var_check_memory, iter_var_check_precond, iter_var_check_rank) against figures worked out by hand; exits non-zero at the first that differs.
//   cache doubles = N pad + pad^2, pad = the rank in whole panels of 32 columns
//     N 10^5, p 1024:  102 400 000 + 1 048 576 = 103 448 576  ->  827 588 608 bytes;  with the solver's 1 048 681 760:  1 876 270 368
//     N 300, p 64:     19 200 + 4 096 = 23 296                ->      186 368 bytes;  with the solver's 885 360:            1 071 728
//     N 130, p 17:     pad 32: 4 160 + 1 024 = 5 184          ->       41 472 bytes
// tests/test_variance_bound_host.py builds it with -fsanitize=address,undefined.
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

int main() {
  using namespace mogp;
  ++checks;
  if (iter_var_bytes(100000, 1024) != 827588608.0 || iter_var_bytes(300, 64) != 186368.0 || iter_var_bytes(130, 17) != 41472.0) {
    std::printf("FAILED the cache bytes: %.0f %.0f %.0f\n", iter_var_bytes(100000, 1024), iter_var_bytes(300, 64), iter_var_bytes(130, 17));
    return 1;
  }
  ++checks;
  if (iter_var_pad(1) != 32 || iter_var_pad(32) != 32 || iter_var_pad(33) != 64 || iter_var_pad(1024) != 1024) { std::printf("FAILED the padding\n"); return 1; }
  const double both = 1876270368.0;
  if (!accepts([&] { iter_var_check_memory("variance_bound", 100000, 1024, 2.0 * both, 0.); }, "exactly half of the free memory")) return 1;
  if (!refuses([&] { iter_var_check_memory("variance_bound", 100000, 1024, 2.0 * both - 2., 0.); },
               "variance_bound: 1876270368 bytes of device memory for the solver and the variance cache of 100000 points at rank 1024 are more than "
               "half of the free device memory"))
    return 1;
  if (!accepts([&] { iter_var_check_memory("variance_bound", 100000, 1024, both, both); }, "memory the handle holds already")) return 1;
  if (!refuses([] { iter_var_check_memory("variance_bound", 300, 64, 2e6, 0.); },
               "variance_bound: 1071728 bytes of device memory for the solver and the variance cache of 300 points at rank 64 are more than half of "
               "the free device memory"))
    return 1;
  if (!refuses([] { iter_var_check_precond("variance_bound", 0); },
               "variance_bound: the variance bound is built from the preconditioner's factor: precond_rank must be at least 1"))
    return 1;
  for (int rank : {1, 64, 1024})
    if (!accepts([&] { iter_var_check_precond("variance_bound", rank); }, "a positive rank")) return 1;
  for (int request : {0, 1, 7, 18})
    if (!accepts([&] { iter_var_check_rank("variance_bound", request, 18); }, "a rank up to the rank reached")) return 1;
  for (int request : {-1, 19, 32})
    if (!refuses([&] { iter_var_check_rank("variance_bound", request, 18); },
                 "variance_bound: rank must be between 1 and the rank the preconditioner reached, 18"))
      return 1;
  if (!refuses([] { iter_var_check_rank("variance_bound", 1, 0); }, "variance_bound: rank must be between 1 and the rank the preconditioner reached, 0"))
    return 1;
  if (!accepts([] { iter_var_check_rank("variance_bound", 0, 0); }, "all of an empty cache")) return 1;
  // the partial sums of a query's chunks fit the 16 doubles that iter_point_bytes counts beside its coordinates
  ++checks;
  if (ITER_VAR_CHUNK != 64 || (ITER_MAX_RANK + ITER_VAR_CHUNK - 1) / ITER_VAR_CHUNK > 16 || iter_point_bytes(10) - 8.0 * 2.0 * 10 != 8.0 * 16) {
    std::printf("FAILED the chunks of a query do not fit its bytes\n");
    return 1;
  }
  if (!refuses([] { iter_plan("variance_bound", 10, 2, 1e9, -1); }, "variance_bound: max_points must not be negative")) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
