// Host check of the cached-state transitions of GPState (csrc/gp_state.h), with its own sweep: exits non-zero at the first property that
// fails.  Every sequence of up to DEPTH steps over the transitions -- drop_factor, unfit, set_fit(true / false), priors_changed and the
// three "built from the factor" marks have_alpha, have_linv, have_kinv(split / not) -- from a fresh state, and after every step:
//   * alpha, linv and kinv are never set without factored, and kinv never without linv;
//   * drop_factor and unfit clear all three (unfit also has_data); set_fit(false) leaves no factor and nothing built from one;
//   * set_fit(true) leaves what was built -- alpha, linv, kinv as they were -- and says factored and has_data;
//   * priors_changed touches logpost_stale alone;
//   * a mark without a factor (or K^-1 without L^-1) throws std::logic_error and changes nothing; have_linv drops K^-1 (the inversion
//     uses its buffer as scratch).
// tests/test_gp_state_host.py builds it with -fsanitize=address,undefined.
#include <cstdio>
#include <stdexcept>

#include "gp_state.h"

using mogp::GPState;

namespace {

struct Flags {
  bool has_data, factored, linv, kinv, alpha, stale, split;
  explicit Flags(const GPState& g)
      : has_data(g.has_data), factored(g.factored), linv(g.linv), kinv(g.kinv), alpha(g.alpha), stale(g.logpost_stale), split(g.kinv_split) {}
  bool operator==(const Flags& o) const {
    return has_data == o.has_data && factored == o.factored && linv == o.linv && kinv == o.kinv && alpha == o.alpha && stale == o.stale &&
           split == o.split;
  }
};

enum Step { DROP, UNFIT, FIT_OK, FIT_BAD, PRIORS, ALPHA, LINV, KINV, KINV_SPLIT, NSTEPS };
const char* const NAMES[NSTEPS] = {"drop_factor", "unfit", "set_fit(true)", "set_fit(false)", "priors_changed", "have_alpha", "have_linv",
                                   "have_kinv(false)", "have_kinv(true)"};
constexpr int DEPTH = 6;
long g_checked = 0;
int g_path[DEPTH];

int fail(const char* what, int depth) {
  std::printf("FAILED %s after:", what);
  for (int k = 0; k <= depth; ++k) std::printf(" %s", NAMES[g_path[k]]);
  std::printf("\n");
  return 1;
}

// applies step s to g; returns 0 when every property of that step holds
int apply_and_check(GPState& g, int s, int depth) {
  const Flags before(g);
  bool threw = false;
  try {
    switch (s) {
      case DROP: g.drop_factor(); break;
      case UNFIT: g.unfit(); break;
      case FIT_OK: g.set_fit(true); break;
      case FIT_BAD: g.set_fit(false); break;
      case PRIORS: g.priors_changed(); break;
      case ALPHA: g.have_alpha(); break;
      case LINV: g.have_linv(); break;
      case KINV: g.have_kinv(false); break;
      case KINV_SPLIT: g.have_kinv(true); break;
    }
  } catch (const std::logic_error&) {
    threw = true;
  }
  const Flags after(g);
  g_checked += 1;
  // the invariants of every state
  if ((after.alpha || after.linv || after.kinv) && !after.factored) return fail("alpha / L^-1 / K^-1 without a factor", depth);
  if (after.kinv && !after.linv) return fail("K^-1 without L^-1", depth);
  const bool is_mark = s == ALPHA || s == LINV || s == KINV || s == KINV_SPLIT;
  const bool must_throw = is_mark && (!before.factored || ((s == KINV || s == KINV_SPLIT) && !before.linv));
  if (threw != must_throw) return fail(must_throw ? "a mark without what it is built from did not throw" : "a legal step threw", depth);
  if (threw) return after == before ? 0 : fail("a refused mark changed the state", depth);
  switch (s) {
    case DROP:
      if (after.factored || after.alpha || after.linv || after.kinv) return fail("drop_factor left something", depth);
      if (after.has_data != before.has_data || after.stale != before.stale) return fail("drop_factor touched has_data / logpost_stale", depth);
      break;
    case UNFIT:
      if (after.has_data || after.factored || after.alpha || after.linv || after.kinv) return fail("unfit left something", depth);
      break;
    case FIT_OK:
      if (!after.has_data || !after.factored) return fail("set_fit(true) without has_data / factored", depth);
      // (what was built is only kept where there was a factor to build it from: by the invariant the flags were clear otherwise)
      if (after.alpha != before.alpha || after.linv != before.linv || after.kinv != before.kinv) return fail("set_fit(true) changed what was built", depth);
      break;
    case FIT_BAD:
      if (after.has_data || after.factored || after.alpha || after.linv || after.kinv) return fail("set_fit(false) left something", depth);
      break;
    case PRIORS: {
      Flags want = before;
      want.stale = true;
      if (!(after == want)) return fail("priors_changed touched more than logpost_stale", depth);
      break;
    }
    case ALPHA: {
      Flags want = before;
      want.alpha = true;
      if (!(after == want)) return fail("have_alpha touched more than alpha", depth);
      break;
    }
    case LINV:
      if (!after.linv || after.kinv) return fail("have_linv: L^-1 set and K^-1 (its scratch) dropped", depth);
      if (after.alpha != before.alpha || after.factored != before.factored || after.has_data != before.has_data) return fail("have_linv touched alpha / factored / has_data", depth);
      break;
    case KINV:
    case KINV_SPLIT:
      if (!after.kinv || after.split != (s == KINV_SPLIT)) return fail("have_kinv: K^-1 and its split mark", depth);
      if (after.alpha != before.alpha || after.linv != before.linv || after.factored != before.factored) return fail("have_kinv touched alpha / L^-1 / factored", depth);
      break;
  }
  return 0;
}

int sweep(const GPState& g, int depth) {
  if (depth == DEPTH) return 0;
  for (int s = 0; s < NSTEPS; ++s) {
    GPState h = g;
    g_path[depth] = s;
    if (apply_and_check(h, s, depth)) return 1;
    if (sweep(h, depth + 1)) return 1;
  }
  return 0;
}

}  // namespace

int main() {
  const GPState fresh;
  const Flags f(fresh);
  if (f.has_data || f.factored || f.linv || f.kinv || f.alpha || f.stale) {
    std::printf("FAILED a fresh state holds something\n");
    return 1;
  }
  if (sweep(fresh, 0)) return 1;
  std::printf("%ld cases ok\n", g_checked);
  return 0;
}
