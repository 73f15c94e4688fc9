// Host check of sample_plan and the jitter ladder of sample_posterior (csrc/predict_plan.h), with its own sweep: exits non-zero at the
// first property that fails.  Over (E, m, S, n, free bytes, max_slots, max_draws):
//   * a plan is either refused -- and then one slot with one tile of draws really does not fit half of the free memory, or one emulator
//     trips the 64 GB rule of predict_full_cov -- or slots * sample_slot_bytes(draws) stays within half of the free memory;
//   * at least one slot and one draw, never more than E slots, S draws, max_slots, max_draws, SAMPLE_MAX_DRAWS or the batch bound;
//   * walking the passes [p0, p0 + slots) and inside them the chunks [s0, s0 + draws) visits every (emulator, draw) exactly once;
//   * negative max_slots / max_draws are refused.
// Then the ladder: rung t adds 10^-6 * 10^t * (mean diagonal), t = 0 .. 4.
// tests/test_sample_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "predict_plan.h"

static int fail(const char* what, long E, int m, long S, int NP, double free_b, int ms, int md) {
  std::printf("FAILED %s: E=%ld m=%d S=%ld NP=%d free=%.4g max_slots=%d max_draws=%d\n", what, E, m, S, NP, free_b, ms, md);
  return 1;
}

int main() {
  const long Es[] = {1, 3, 64, 500}, Ss[] = {1, 3, 65, 1000, 100000};
  const int ms[] = {1, 127, 128, 129, 300, 2000, 20000}, NPs[] = {256, 2048}, cap_s[] = {0, 1, 3, 1000}, cap_d[] = {0, 1, 7, 64, 100000};
  const double frees[] = {1e6, 1e8, 4e9, 2.5e11};
  long cases = 0, refused = 0;
  for (long E : Es)
    for (int m : ms)
      for (long S : Ss)
        for (int NP : NPs)
          for (double free_b : frees)
            for (int mxs : cap_s)
              for (int mxd : cap_d) {
                const int LD = NP, R = 1;
                const double budget = 0.5 * free_b;
                mogp::SamplePlan p{0, 0};
                bool threw = false;
                try {
                  p = mogp::sample_plan(E, m, S, LD, NP, R, free_b, mxs, mxd);
                } catch (const std::runtime_error&) {
                  threw = true;
                }
                const bool must_refuse = mogp::sample_slot_bytes(m, LD, NP, R, 1) > budget || mogp::fullcov_rule_bytes(m, LD) > 64.0e9;
                if (threw != must_refuse) return fail(threw ? "refused what fits" : "accepted what does not fit", E, m, S, NP, free_b, mxs, mxd);
                ++cases;
                if (threw) {
                  ++refused;
                  continue;
                }
                if (p.slots < 1 || p.draws < 1) return fail("at least one slot and one draw", E, m, S, NP, free_b, mxs, mxd);
                if (p.slots > E || p.draws > S) return fail("more slots than emulators or draws than asked", E, m, S, NP, free_b, mxs, mxd);
                if (mxs > 0 && p.slots > mxs) return fail("max_slots", E, m, S, NP, free_b, mxs, mxd);
                if (mxd > 0 && p.draws > mxd) return fail("max_draws", E, m, S, NP, free_b, mxs, mxd);
                if (p.draws > mogp::SAMPLE_MAX_DRAWS) return fail("draws per chunk above the grid bound", E, m, S, NP, free_b, mxs, mxd);
                if (p.slots > mogp::cv_slot_bound((int)mogp::sample_nps(m))) return fail("batch bound", E, m, S, NP, free_b, mxs, mxd);
                if ((double)p.slots * mogp::sample_slot_bytes(m, LD, NP, R, p.draws) > budget) return fail("byte budget", E, m, S, NP, free_b, mxs, mxd);
                if ((double)p.slots * mogp::fullcov_rule_bytes(m, LD) > 64.0e9) return fail("64 GB rule", E, m, S, NP, free_b, mxs, mxd);
                // coverage: counted per emulator (E * S can be 5 * 10^7: no table of pairs)
                if (E * S <= 200000) {
                  std::vector<int> seen((size_t)(E * S), 0);
                  for (long p0 = 0; p0 < E; p0 += p.slots)
                    for (long e = p0; e < std::min(E, p0 + p.slots); ++e)
                      for (long s0 = 0; s0 < S; s0 += p.draws)
                        for (long s = s0; s < std::min(S, s0 + p.draws); ++s) seen[(size_t)(e * S + s)] += 1;
                  for (int c : seen)
                    if (c != 1) return fail("every (emulator, draw) exactly once", E, m, S, NP, free_b, mxs, mxd);
                }
              }
  if (refused == 0 || refused == cases) return fail("the sweep must hold both refused and accepted plans", 0, 0, 0, 0, 0, 0, 0);
  for (int bad = 0; bad < 2; ++bad) {
    bool threw = false;
    try {
      mogp::sample_plan(3, 100, 10, 256, 256, 1, 1e10, bad == 0 ? -1 : 0, bad == 1 ? -1 : 0);
    } catch (const std::runtime_error& e) {
      threw = std::string(e.what()).find("must not be negative") != std::string::npos;
    }
    if (!threw) return fail("negative max_slots / max_draws refused", 3, 100, 10, 256, 1e10, bad == 0 ? -1 : 0, bad == 1 ? -1 : 0);
  }
  {   // 64 GB rule: one emulator at m = 100000 points beside n = 2000
    bool threw = false;
    try {
      mogp::sample_plan(1, 100000, 1, 2048, 2048, 1, 1e13, 0, 0);
    } catch (const std::runtime_error& e) {
      threw = std::string(e.what()).find("64 GB") != std::string::npos;
    }
    if (!threw) return fail("64 GB rule refused", 1, 100000, 1, 2048, 1e13, 0, 0);
  }
  // bytes of a slot: m = 300 beside n = 130 (NP = 256): MP = 384, NPs = 384, one tile of draws
  if (mogp::sample_mp(300) != 384 || mogp::sample_nps(300) != 384 || mogp::sample_nps(128) != 256 || mogp::sample_mp(128) != 128 ||
      mogp::sample_draw_rows(65) != 128 || mogp::sample_draw_bytes(300, 65) != 2.0 * 8.0 * 128 * 384)
    return fail("layout sizes", 0, 300, 65, 256, 0, 0, 0);
  for (int rows : {1, 127, 128, 255, 256})
    if (mogp::scratch_np(rows) != (rows + 1 + 127) / 128 * 128 || mogp::sample_nps(rows) != mogp::scratch_np(rows))
      return fail("sample_nps = scratch_np = roundup(rows + 1, 128)", 0, rows, 0, 0, 0, 0, 0);
  if (mogp::scratch_np(127) != 128 || mogp::scratch_np(128) != 256) return fail("scratch_np at the tile edge", 0, 127, 0, 0, 0, 0, 0);
  if (mogp::sample_fixed_bytes(300, 256, 256, 1) != 8.0 * (384.0 * 256 + 256.0 * 384 + 300.0 * 300 + 300 + 384.0 * 384 + 16.0 * 384 + 300))
    return fail("bytes per slot", 0, 300, 0, 256, 0, 0, 0);
  // the ladder: 10^-6 * 10^t * mean diagonal, t = 0 .. 4
  if (mogp::SAMPLE_LADDER_RUNGS != 5) return fail("five rungs", 0, 0, 0, 0, 0, 0, 0);
  const double dbars[] = {1.0, 0.37, 2.5e-3, 4.0e7};
  for (double dbar : dbars)
    for (int t = 0; t < mogp::SAMPLE_LADDER_RUNGS; ++t) {
      const double want = 1e-6 * std::pow(10.0, t) * dbar, got = mogp::sample_ladder_delta(t, dbar);
      if (!(std::fabs(got - want) <= 8 * 2.220446049250313e-16 * want)) return fail("ladder schedule", t, 0, 0, 0, dbar, 0, 0);
    }
  std::printf("%ld cases ok (%ld refused)\n", cases, refused);
  return 0;
}
