// Host check of mixture_plan and mixture_weights (csrc/predict_plan.h), with its own sweep: exits non-zero at the first property that
// fails.  Over (E, S, device slots, m, max_slots, max_points):
//   * at least one slot, never more than E * S, the device slots or max_slots;
//   * walking the passes [g * slots, (g + 1) * slots) over the emulator-major, sample-ascending pairs visits every (emulator, sample)
//     exactly once, every slot holds one whole sample, and the samples of an emulator come in ascending order;
//   * at least one point per chunk, max_points honoured, and without a cap the chunk rule of predict() (predict_chunk_points).
// tests/test_marginal_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "predict_plan.h"

static int fail(const char* what, long E, long S, long dev, int m, int ms, int mp) {
  std::printf("FAILED %s: E=%ld S=%ld device_slots=%ld m=%d max_slots=%d max_points=%d\n", what, E, S, dev, m, ms, mp);
  return 1;
}

int main() {
  const long Es[] = {1, 2, 3, 7, 64}, Ss[] = {1, 2, 5, 32, 33}, devs[] = {1, 2, 5, 8, 9, 100, 4096};
  const int ms[] = {1, 37, 128, 129, 10000}, caps_s[] = {0, 1, 2, 5, 7, 1000}, caps_p[] = {0, 1, 16, 20000};
  const int LD = 2056;
  const double cap = 12e9;
  long cases = 0;
  for (long E : Es)
    for (long S : Ss)
      for (long dev : devs)
        for (int m : ms)
          for (int mxs : caps_s)
            for (int mxp : caps_p) {
              const mogp::MixturePlan p = mogp::mixture_plan(E, S, LD, dev, m, mxs, mxp, cap);
              const long pairs = E * S;
              if (p.slots < 1) return fail("at least one slot", E, S, dev, m, mxs, mxp);
              if (p.slots > pairs || p.slots > dev || (mxs > 0 && p.slots > mxs)) return fail("too many slots", E, S, dev, m, mxs, mxp);
              if (mxs == 0 && dev >= pairs && p.slots != pairs) return fail("everything fits: one pass", E, S, dev, m, mxs, mxp);
              // coverage, in order
              std::vector<int> seen(pairs, 0);
              std::vector<long> last(E, -1);
              long visited = 0;
              for (long g = 0; g * p.slots < pairs; ++g)
                for (long k = 0; k < p.slots && g * p.slots + k < pairs; ++k) {
                  const long pr = g * p.slots + k, e = pr / S, s = pr % S;
                  if (pr != visited) return fail("pairs in order", E, S, dev, m, mxs, mxp);
                  if (seen[pr]++) return fail("a pair twice", E, S, dev, m, mxs, mxp);
                  if (s != last[e] + 1) return fail("samples of an emulator ascending", E, S, dev, m, mxs, mxp);
                  last[e] = s;
                  ++visited;
                }
              if (visited != pairs) return fail("every pair once", E, S, dev, m, mxs, mxp);
              if (p.points < 1) return fail("at least one point", E, S, dev, m, mxs, mxp);
              if (mxp > 0 && (p.points > mxp || p.points > m)) return fail("max_points", E, S, dev, m, mxs, mxp);
              if (mxp == 0 && p.points != mogp::predict_chunk_points(cap, (int)p.slots, LD, m)) return fail("chunk rule", E, S, dev, m, mxs, mxp);
              ++cases;
            }
  // mixture_weights: hand cases
  {
    const double F[4] = {7., 7., 7., 7.}, q[4] = {.5, .5, .5, .5};
    const int ok[4] = {1, 1, 1, 1};
    double w[4];
    if (!mogp::mixture_weights(4, F, ok, nullptr, q, w)) return fail("equal F", 0, 0, 0, 0, 0, 0);
    for (double x : w)
      if (x != 0.25) return fail("equal F: uniform", 0, 0, 0, 0, 0, 0);
  }
  {
    const double F[3] = {5., 1., 5.}, q[3] = {0., 0., 0.}, wi[3] = {1., 5., 3.};
    const int ok[3] = {1, 0, 1};
    double w[3];
    if (!mogp::mixture_weights(3, F, ok, nullptr, q, w) || w[0] != .5 || w[1] != 0. || w[2] != .5) return fail("failed sample", 0, 0, 0, 0, 0, 0);
    if (!mogp::mixture_weights(3, F, ok, wi, nullptr, w) || w[0] != .25 || w[1] != 0. || w[2] != .75) return fail("explicit weights", 0, 0, 0, 0, 0, 0);
    const int none[3] = {0, 0, 0};
    if (mogp::mixture_weights(3, F, none, nullptr, q, w) || !std::isnan(w[0]) || !std::isnan(w[2])) return fail("all failed", 0, 0, 0, 0, 0, 0);
    const double zero[3] = {0., 0., 0.};
    if (mogp::mixture_weights(3, F, ok, zero, nullptr, w) || !std::isnan(w[1])) return fail("weights sum to zero", 0, 0, 0, 0, 0, 0);
    const double Fd[3] = {0., 800., 900.};
    const int all[3] = {1, 1, 1};
    if (!mogp::mixture_weights(3, Fd, all, nullptr, q, w) || w[0] != 1. || w[1] != 0. || w[2] != 0.) return fail("dominant sample", 0, 0, 0, 0, 0, 0);
  }
  std::printf("%ld cases ok\n", cases);
  return 0;
}
