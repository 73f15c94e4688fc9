// Host check of cv_plan (csrc/predict_plan.h), with its own sweep: exits non-zero at the first property that fails.  Over
// (E, k, NPsub, device slots, max_slots):
//   * at least one slot, never more than E * k, the device slots, the batch bound of the sub-engine (cv_slot_bound) or max_slots;
//   * with no cap in the way everything goes in one pass;
//   * walking the passes [g * slots, (g + 1) * slots) over the emulator-major, fold-ascending pairs visits every (emulator, fold) exactly
//     once, in order.
// tests/test_cv_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "predict_plan.h"

static int fail(const char* what, long E, long k, int NP, long dev, int ms) {
  std::printf("FAILED %s: E=%ld k=%ld NPsub=%d device_slots=%ld max_slots=%d\n", what, E, k, NP, dev, ms);
  return 1;
}

int main() {
  const long Es[] = {1, 2, 3, 7, 64, 500}, ks[] = {2, 3, 5, 10, 33, 130, 2000}, devs[] = {0, 1, 2, 5, 8, 9, 100, 4096, 1000000};
  const int NPs[] = {128, 256, 384, 1024, 2048, 16384}, caps[] = {0, 1, 2, 3, 7, 1000, 100000};
  long cases = 0;
  for (long E : Es)
    for (long k : ks)
      for (int NP : NPs)
        for (long dev : devs)
          for (int mxs : caps) {
            const long slots = mogp::cv_plan(E, k, NP, dev, mxs);
            const long pairs = E * k, bound = mogp::cv_slot_bound(NP);
            if (slots < 1) return fail("at least one slot", E, k, NP, dev, mxs);
            if (bound < 1 || bound > 65535) return fail("batch bound", E, k, NP, dev, mxs);
            if (slots > pairs) return fail("more slots than pairs", E, k, NP, dev, mxs);
            if (slots > 1 && slots > dev) return fail("more slots than the device holds", E, k, NP, dev, mxs);
            if (slots > bound) return fail("more slots than the batch bound", E, k, NP, dev, mxs);
            if (mxs > 0 && slots > mxs) return fail("max_slots", E, k, NP, dev, mxs);
            if (mxs == 0 && dev >= pairs && bound >= pairs && slots != pairs) return fail("everything fits: one pass", E, k, NP, dev, mxs);
            std::vector<int> seen(pairs, 0);
            std::vector<long> last(E, -1);
            long visited = 0;
            for (long g = 0; g * slots < pairs; ++g)
              for (long s = 0; s < slots && g * slots + s < pairs; ++s) {
                const long pr = g * slots + s, e = pr / k, f = pr % k;
                if (pr != visited) return fail("pairs in order", E, k, NP, dev, mxs);
                if (seen[pr]++) return fail("a pair twice", E, k, NP, dev, mxs);
                if (f != last[e] + 1) return fail("folds of an emulator ascending", E, k, NP, dev, mxs);
                last[e] = f;
                ++visited;
              }
            if (visited != pairs) return fail("every pair once", E, k, NP, dev, mxs);
            ++cases;
          }
  if (mogp::cv_slot_bytes(256) != 3.0 * 256 * 256 * 8) return fail("bytes per slot", 0, 0, 256, 0, 0);
  std::printf("%ld cases ok\n", cases);
  return 0;
}
