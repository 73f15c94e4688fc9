// Host check of the named refusals of the LocalGP handle (csrc/predict_plan.h: local_check_kernel, local_check_k, local_check_hyper,
// local_check_scales), of vecchia_held_bytes and of the LDS layout of the two tile kernels (LocalLds, local_lds_bytes): every refusal by
// its exact message under each of the three prefixes, acceptance at the edges, and the byte counts against the two sums the kernels were
// first written with, for every D and both layouts.  Exits non-zero at the first difference.
// tests/test_local_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "predict_plan.h"

static int failures = 0;

// "" = accepted
static std::string message_of(const std::function<void()>& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}
static void expect(const char* what, const std::string& got, const std::string& want) {
  if (got == want) return;
  std::printf("FAILED %s: got \"%s\", expected \"%s\"\n", what, got.c_str(), want.c_str());
  ++failures;
}

int main() {
  const int MAX_K = 126;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan(""), denorm = std::numeric_limits<double>::denorm_min();
  int checks = 0;
  for (const std::string who : {"predict_local", "vecchia_neighbours", "vecchia_loglik"}) {
    const std::string kernel = who + ": the kernel must be a function of one scaled distance (squared exponential or Matern 5/2)";
    const std::string hyper = who + ": sigma^2 must be positive and finite, nugget and jitter finite and not negative";
    const std::string scales = who + ": the scales must be positive and finite";
    for (int kt : {0, 1}) expect("kernel accepted", message_of([&] { mogp::local_check_kernel(who, kt); }), ""), ++checks;
    for (int kt : {-1, 2, 3}) expect("kernel refused", message_of([&] { mogp::local_check_kernel(who, kt); }), kernel), ++checks;

    // n_neighbours: 1 .. min(N, 126) for a prediction, 1 .. min(N - 1, 126) for the ordered lists
    for (bool vecchia : {false, true}) {
      for (long N : {1L, 2L, 9L, 126L, 127L, 128L, 1000L}) {
        const long top = std::min<long>(vecchia ? N - 1 : N, MAX_K);
        const std::string range = who + ": n_neighbours must be between 1 and " + std::to_string(top);
        for (long k : {-1L, 0L, 1L, top - 1, top, top + 1, 127L, N, N + 1}) {
          const bool fine = k >= 1 && k <= top;
          expect("n_neighbours", message_of([&] { mogp::local_check_k(who, N, (int)k, vecchia, MAX_K); }), fine ? "" : range), ++checks;
        }
      }
    }
    expect("k = 1 of one point", message_of([&] { mogp::local_check_k(who, 1, 1, false, MAX_K); }), ""), ++checks;
    expect("k = 126 of 126", message_of([&] { mogp::local_check_k(who, 126, 126, false, MAX_K); }), ""), ++checks;
    expect("k = 126 of 1000", message_of([&] { mogp::local_check_k(who, 1000, 126, false, MAX_K); }), ""), ++checks;
    expect("vecchia k = N - 1", message_of([&] { mogp::local_check_k(who, 50, 49, true, MAX_K); }), ""), ++checks;
    expect("vecchia k = N", message_of([&] { mogp::local_check_k(who, 50, 50, true, MAX_K); }), who + ": n_neighbours must be between 1 and 49"), ++checks;
    expect("vecchia of one point", message_of([&] { mogp::local_check_k(who, 1, 1, true, MAX_K); }), who + ": n_neighbours must be between 1 and 0"), ++checks;

    // sigma^2, nugget, jitter; then the scales
    const std::vector<double> ok3 = {0.5, 2.0, 1e-3};
    expect("hyper accepted", message_of([&] { mogp::local_check_hyper(who, 3, ok3.data(), 1.5, 1e-6, 1e-8); }), ""), ++checks;
    expect("nugget 0 and jitter 0", message_of([&] { mogp::local_check_hyper(who, 3, ok3.data(), 1.5, 0., 0.); }), ""), ++checks;
    expect("denormal sigma^2", message_of([&] { mogp::local_check_hyper(who, 3, ok3.data(), denorm, 0., 0.); }), ""), ++checks;
    for (double bad : {0., -1., nan, inf, -inf})
      expect("sigma^2 refused", message_of([&] { mogp::local_check_hyper(who, 3, ok3.data(), bad, 0., 0.); }), hyper), ++checks;
    for (double bad : {-1e-300, -1., nan, inf, -inf}) {
      expect("nugget refused", message_of([&] { mogp::local_check_hyper(who, 3, ok3.data(), 1., bad, 0.); }), hyper), ++checks;
      expect("jitter refused", message_of([&] { mogp::local_check_hyper(who, 3, ok3.data(), 1., 0., bad); }), hyper), ++checks;
    }
    for (int at = 0; at < 3; ++at) {
      std::vector<double> s = ok3;
      s[at] = denorm;
      expect("denormal scale", message_of([&] { mogp::local_check_hyper(who, 3, s.data(), 1., 0., 0.); }), ""), ++checks;
      expect("denormal scale alone", message_of([&] { mogp::local_check_scales(who, 3, s.data()); }), ""), ++checks;
      for (double bad : {0., -0., -1., nan, inf, -inf}) {
        s[at] = bad;
        expect("scale refused", message_of([&] { mogp::local_check_hyper(who, 3, s.data(), 1., 0., 0.); }), scales), ++checks;
        expect("scale refused alone", message_of([&] { mogp::local_check_scales(who, 3, s.data()); }), scales), ++checks;
        // sigma^2 is looked at before the scales
        expect("both bad", message_of([&] { mogp::local_check_hyper(who, 3, s.data(), nan, 0., 0.); }), hyper), ++checks;
      }
    }
  }

  // what the handle already holds: doubles of out, red and scratch, ints of ok
  if (mogp::vecchia_held_bytes(0, 0, 0, 0) != 0. || mogp::vecchia_held_bytes(1000, 20, 34816, 1000) != 8. * 35836 + 4000. ||
      mogp::vecchia_held_bytes(1, 0, 0, 0) != 8. || mogp::vecchia_held_bytes(0, 1, 0, 0) != 8. || mogp::vecchia_held_bytes(0, 0, 1, 0) != 8. ||
      mogp::vecchia_held_bytes(0, 0, 0, 1) != 4.) {
    std::printf("FAILED vecchia_held_bytes\n");
    ++failures;
  }

  // The LDS of the two kernels, in doubles: chol128_dev's 128 x 18 + 256 + 256, the table (256), the targets (128), with the gradient
  // 2 x 128 + 2 x 256 more, 128 rows of D | 1 for the points and 2 for the status word
  for (int D = 1; D <= 80; ++D) {
    const std::size_t chol = 128 * 18 + 256 + 256, ld = (std::size_t)(D | 1);
    const std::size_t predict = sizeof(double) * (chol + 256 + 128 + 128 * ld + 2);
    for (bool grad : {false, true}) {
      const std::size_t vecchia = sizeof(double) * (chol + 256 + 128 + (grad ? 2 * 128 + 2 * 256 : 0) + 128 * ld + 2);
      const mogp::LocalLds o(D, grad);
      const bool ordered = o.tab == (int)chol && o.tab < o.yv && o.yv + 128 <= o.wv && o.wv <= o.av && o.av <= o.reda && o.reda <= o.redb &&
                           o.redb <= o.pts && o.pts + 128 * o.ld == o.info && o.info + 2 == o.doubles && o.ld == (int)ld &&
                           (!grad || (o.av - o.wv == 128 && o.reda - o.av == 128 && o.redb - o.reda == 256 && o.pts - o.redb == 256)) &&
                           (grad || o.pts == o.wv);
      if (mogp::local_lds_bytes(D, grad) != vecchia || (!grad && vecchia != predict) || !ordered) {
        std::printf("FAILED the LDS layout at D %d grad %d: %zu bytes, expected %zu\n", D, (int)grad, mogp::local_lds_bytes(D, grad), vecchia);
        ++failures;
      }
      ++checks;
    }
  }
  if (failures) return 1;
  std::printf("ok %d checks\n", checks);
  return 0;
}
