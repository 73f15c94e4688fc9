// Host check of cv_plan (csrc/predict_plan.h), with its own sweep: exits non-zero at the first property that fails.  Over
// (E, k, NPsub, device slots, max_slots):
//   * at least one slot, never more than E * k, the device slots, the batch bound of the scratch factorisation (cv_slot_bound) or max_slots;
//   * with no cap in the way everything goes in one pass;
//   * walking the passes [g * slots, (g + 1) * slots) over the emulator-major, fold-ascending pairs visits every (emulator, fold) exactly
//     once, in order.
// Then cv_folds (n = 7, k = 3, unequal folds, and its three refusals) and cv_pass_table (a padded last pass) on tables worked out by hand.
// tests/test_cv_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "predict_plan.h"

static int fail(const char* what, long E, long k, int NP, long dev, int ms) {
  std::printf("FAILED %s: E=%ld k=%ld NPsub=%d device_slots=%ld max_slots=%d\n", what, E, k, NP, dev, ms);
  return 1;
}

// the message cv_folds refuses the labels with ("" when it does not)
static std::string refusal(const std::vector<int>& labels, int k) {
  try {
    mogp::cv_folds(labels.data(), (int)labels.size(), k);
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
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
  // the padded size of a scratch matrix: the rows and one right-hand side in whole tiles of 128 -- 127 rows fill one tile, 128 need two
  for (long rows : {1L, 127L, 128L, 255L, 256L})
    if (mogp::scratch_np(rows) != (rows + 1 + 127) / 128 * 128) return fail("scratch_np = roundup(rows + 1, 128)", rows, 0, 0, 0, 0);
  if (mogp::scratch_np(127) != 128 || mogp::scratch_np(128) != 256) return fail("scratch_np at the tile edge", 127, 0, 0, 0, 0);
  {
    const std::vector<int> labels = {2, 0, 2, 1, 2, 0, 2};
    const mogp::CvFolds c = mogp::cv_folds(labels.data(), 7, 3);
    if (c.size != std::vector<int>{2, 1, 4} || c.nsub != 4 || c.folds != std::vector<int>{1, 5, -1, -1, 3, -1, -1, -1, 0, 2, 4, 6})
      return fail("cv_folds: n = 7, k = 3", 1, 3, 0, 0, 0);
    const mogp::CvFolds one = mogp::cv_folds(std::vector<int>{1, 0, 2}.data(), 3, 3);      // every fold a single point
    if (one.nsub != 1 || one.folds != std::vector<int>{1, 0, 2}) return fail("cv_folds: leave-one-out", 1, 3, 0, 0, 0);
    if (refusal({2, 0, -1, 1}, 3) != "cross_validate: fold label -1 of point 2 is outside [0, 3)") return fail("cv_folds: negative label", 1, 3, 0, 0, 0);
    if (refusal({2, 0, 1, 3}, 3) != "cross_validate: fold label 3 of point 3 is outside [0, 3)") return fail("cv_folds: label = k", 1, 3, 0, 0, 0);
    if (refusal({2, 0, 2, 0}, 3) != "cross_validate: fold 1 is empty") return fail("cv_folds: empty fold", 1, 3, 0, 0, 0);
    if (refusal({3, 0, 2, 0}, 3) != "cross_validate: fold label 3 of point 0 is outside [0, 3)") return fail("cv_folds: the label comes first", 1, 3, 0, 0, 0);
    // two emulators (5 and 9 of the engine), these folds, four slots: six pairs, the second pass padded with identities
    const int ids[2] = {5, 9};
    std::vector<int> tab(16, 77);
    mogp::cv_pass_table(0, 4, 4, 3, ids, c.size.data(), tab.data());
    if (tab != std::vector<int>{5, 0, 0, 2, 5, 0, 1, 1, 5, 0, 2, 4, 9, 1, 0, 2}) return fail("cv_pass_table: pass 0", 2, 3, 0, 0, 4);
    mogp::cv_pass_table(4, 2, 4, 3, ids, c.size.data(), tab.data());
    if (tab != std::vector<int>{9, 1, 1, 1, 9, 1, 2, 4, -1, 0, 0, 0, -1, 0, 0, 0}) return fail("cv_pass_table: padded pass", 2, 3, 0, 0, 4);
  }
  std::printf("%ld cases ok\n", cases);
  return 0;
}
