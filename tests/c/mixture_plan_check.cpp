// Host check of mixture_plan and mixture_weights (csrc/predict_plan.h), with its own sweep: exits non-zero at the first property that
// fails.  Over (E, S, device slots, m, max_slots, max_points):
//   * at least one slot, never more than E * S, the device slots or max_slots;
//   * walking the passes [g * slots, (g + 1) * slots) over the emulator-major, sample-ascending pairs visits every (emulator, sample)
//     exactly once, every slot holds one whole sample, and the samples of an emulator come in ascending order;
//   * at least one point per chunk, max_points honoured, and without a cap the chunk rule of predict() (predict_chunk_points).
// Then mixture_weights and mixture_pass_tables on tables worked out by hand (E = 3, S = 5, four slots: four passes, emulators 0 and 1 share
// pass 1).
// tests/test_marginal_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "predict_plan.h"

static bool same(const std::vector<int>& a, std::initializer_list<int> b) { return a == std::vector<int>(b); }
static bool same(const std::vector<double>& a, std::initializer_list<double> b) { return a == std::vector<double>(b); }

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
  // mixture_pass_tables.  Pairs 0 .. 14 = (emulator, sample) emulator-major; w = (p + 1) / 128, nugget = (p + 1) / 1024 of pair p.
  //   emulator 0: sample 0 fails -> its pivot is pair 1;  emulator 1: factorises but is dead (alive = 0);
  //   emulator 2: samples 0, 1 and 3 fail -> pivot pair 12;  pairs 8 .. 11 all fail: pass 2 has nothing to predict
  {
    const int ok[15] = {0, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 0, 1}, alive[3] = {1, 0, 1}, pivot[3] = {1, 5, 12};
    double w[15], nug[15];
    for (int p = 0; p < 15; ++p) {
      w[p] = (p + 1) / 128.;
      nug[p] = (p + 1) / 1024.;
    }
    auto W = [&](int p) { return w[p]; };
    auto N = [&](int p) { return nug[p]; };
    // pass 0, pairs 0 .. 3: slot 0 failed; emulator 0 holds the four slots and its pivot is row 0 (slot 1)
    mogp::MixturePassTables t = mogp::mixture_pass_tables(0, 4, 5, ok, w, nug, true, alive, pivot);
    if (!same(t.okslots, {1, 2, 3}) || !same(t.rows, {-1, 0, 1, 2}) || !same(t.etab, {0, 0, 4, 0}) ||
        !same(t.prm, {0., 0., W(1), N(1), W(2), N(2), W(3), N(3)}))
      return fail("pass tables: pass 0", 3, 5, 4, 0, 0, 0);
    // pass 1, pairs 4 .. 7: emulator 0's last sample in slot 0, its pivot pair 1 lies in pass 0 -> -1; emulator 1 (slots 1 .. 3) is dead
    t = mogp::mixture_pass_tables(4, 4, 5, ok, w, nug, true, alive, pivot);
    if (!same(t.okslots, {0, 1, 2, 3}) || !same(t.rows, {0, 1, 2, 3}) || !same(t.etab, {0, 0, 1, -1}) ||
        !same(t.prm, {W(4), N(4), W(5), N(5), W(6), N(6), W(7), N(7)}))
      return fail("pass tables: pass 1", 3, 5, 4, 0, 0, 0);
    // pass 2, pairs 8 .. 11: no slot factorised -> skipped
    t = mogp::mixture_pass_tables(8, 4, 5, ok, w, nug, true, alive, pivot);
    if (!t.okslots.empty() || !t.etab.empty() || !same(t.rows, {-1, -1, -1, -1}) || !same(t.prm, {0., 0., 0., 0., 0., 0., 0., 0.}))
      return fail("pass tables: pass 2", 3, 5, 4, 0, 0, 0);
    // pass 3, pairs 12 .. 14 (a short pass): emulator 2, slot 1 failed, pivot = pair 12 = row 0; without the nugget
    t = mogp::mixture_pass_tables(12, 3, 5, ok, w, nug, false, alive, pivot);
    if (!same(t.okslots, {0, 2}) || !same(t.rows, {0, -1, 1}) || !same(t.etab, {2, 0, 3, 0}) || !same(t.prm, {W(12), 0., 0., 0., W(14), 0.}))
      return fail("pass tables: pass 3", 3, 5, 4, 0, 0, 0);
    // five slots, pass 1 = emulator 1 alone: slots to predict but nobody to accumulate them for -> an empty etab (skipped as well)
    t = mogp::mixture_pass_tables(5, 5, 5, ok, w, nug, true, alive, pivot);
    if (!same(t.okslots, {0, 1, 2}) || !same(t.rows, {0, 1, 2, -1, -1}) || !t.etab.empty())
      return fail("pass tables: dead emulator alone", 3, 5, 5, 0, 0, 0);
    // eight slots, pass 1 = pairs 8 .. 14: emulator 1 has no row, emulator 2 starts at slot 2 and its pivot is row 0 (slot 4)
    t = mogp::mixture_pass_tables(8, 7, 5, ok, w, nug, true, alive, pivot);
    if (!same(t.okslots, {4, 6}) || !same(t.rows, {-1, -1, -1, -1, 0, -1, 1}) || !same(t.etab, {2, 2, 5, 0}))
      return fail("pass tables: eight slots", 3, 5, 8, 0, 0, 0);
  }
  std::printf("%ld cases ok\n", cases);
  return 0;
}
