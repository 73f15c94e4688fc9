// Host check of the plan of the iterative exact likelihood (csrc/predict_plan.h: iter_lik_bytes, iter_lik_check_memory, iter_lik_check_probes)
// against figures worked out by hand; exits non-zero at the first that differs.
//   doubles = 32 N + 64 max_iter + 32 max(rank, 1) + (ceil(N / 64) + 32) 2 D
//     N 10^5, D 10, p 1024, 1000 iterations:  3 200 000 + 64 000 + 32 768 + 1595 * 20 = 3 328 668  -> 26 629 344 bytes
//     N 300, D 3, p 0, 5 iterations:          9 600 + 320 + 32 + 37 * 6 = 10 174                  ->     81 392 bytes
// tests/test_exact_lik_host.py builds it with -fsanitize=address,undefined.
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
  if (iter_lik_bytes(100000, 10, 1024, 1000) != 26629344.0 || iter_lik_bytes(300, 3, 0, 5) != 81392.0) {
    std::printf("FAILED the bytes: %.0f %.0f\n", iter_lik_bytes(100000, 10, 1024, 1000), iter_lik_bytes(300, 3, 0, 5));
    return 1;
  }
  if (!accepts([] { iter_lik_check_memory("loglik_exact", 100000, 10, 1024, 1000, 2.0 * 26629344.0, 0.); }, "exactly half of the free memory")) return 1;
  if (!refuses([] { iter_lik_check_memory("loglik_exact", 100000, 10, 1024, 1000, 2.0 * 26629344.0 - 2., 0.); },
               "loglik_exact: 26629344 bytes of device memory for the probe panel and the coefficient log of 100000 points and 1000 iterations are "
               "more than half of the free device memory"))
    return 1;
  if (!accepts([] { iter_lik_check_memory("loglik_exact", 100000, 10, 1024, 1000, 26629344.0, 26629344.0); }, "memory the handle holds already")) return 1;
  for (int T : {1, 15, 16, 31})
    if (!accepts([T] { iter_lik_check_probes("loglik_exact", T); }, "a number of probes inside 1 .. 31")) return 1;
  for (int T : {0, -1, 32, 1000})
    if (!refuses([T] { iter_lik_check_probes("loglik_exact", T); }, "loglik_exact: n_probes must be between 1 and 31")) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
