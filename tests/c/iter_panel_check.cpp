// Host check of csrc/iter_panel.h: rows_to_panel and panel_to_rows against the index formula written out, over the shapes and column
// windows the solver's entry points use -- a single entry, a second panel of one column (r = 33), the probes' window one column into the
// panel -- with leading dimensions larger than the column and row counts, and canary values everywhere in the destination: nothing outside
// the window may change.  Exits non-zero at the first that fails.  tests/test_iterative_host.py builds it with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "iter_panel.h"

static int checks = 0;

static bool check(bool ok, const char* what, size_t N, size_t r, size_t c0, size_t ncols, size_t pc0) {
  ++checks;
  if (!ok) std::printf("FAILED %s at N %zu r %zu source columns [%zu, %zu) panel column %zu\n", what, N, r, c0, c0 + ncols, pc0);
  return ok;
}

static double source_value(size_t i, size_t c) { return 1.0 + (double)i * 64.0 + (double)c; }      // distinct, exact and never the canary

// one window, both directions: source columns [c0, c0 + ncols) of the row-major (N, r) matrix <-> panel columns [pc0, pc0 + ncols)
static bool window(size_t N, size_t r, size_t c0, size_t ncols, size_t pc0) {
  using namespace mogp;
  const double canary = -7.25;
  const size_t ldr = r + 3, ldp = N + 2, pcols = pc0 + ncols + 1;        // a leading dimension beyond the counts, and a column behind the window
  std::vector<double> rows(N * ldr, canary), panel(pcols * ldp, canary);
  for (size_t i = 0; i < N; ++i)
    for (size_t c = 0; c < r; ++c) rows[i * ldr + c] = source_value(i, c);
  rows_to_panel(rows.data(), N, ldr, c0, ncols, panel.data(), ldp, pc0);
  bool in = true, out = true;
  for (size_t pc = 0; pc < pcols; ++pc)
    for (size_t i = 0; i < ldp; ++i) {
      const double got = panel[pc * ldp + i];
      if (pc >= pc0 && pc < pc0 + ncols && i < N) in = in && got == source_value(i, c0 + (pc - pc0));
      else out = out && got == canary;
    }
  if (!check(in, "rows_to_panel: entry (i, c) of the window at [c * ld + i]", N, r, c0, ncols, pc0)) return false;
  if (!check(out, "rows_to_panel: nothing outside the window is written", N, r, c0, ncols, pc0)) return false;
  // back into a matrix of canaries: the window holds the source again, everything else is untouched
  std::vector<double> back(N * ldr, canary);
  panel_to_rows(back.data(), N, ldr, c0, ncols, panel.data(), ldp, pc0);
  in = out = true;
  for (size_t i = 0; i < N; ++i)
    for (size_t c = 0; c < ldr; ++c) {
      const double got = back[i * ldr + c];
      if (c >= c0 && c < c0 + ncols) in = in && got == source_value(i, c);
      else out = out && got == canary;
    }
  if (!check(in, "panel_to_rows: entry [c * ld + i] of the window at (i, c)", N, r, c0, ncols, pc0)) return false;
  return check(out, "panel_to_rows: nothing outside the window is written", N, r, c0, ncols, pc0);
}

int main() {
  const size_t shapes[3][2] = {{1, 1}, {5, 33}, {130, 7}};
  for (const auto& s : shapes) {
    const size_t N = s[0], r = s[1];
    // the column windows [0, 32) and [32, 33) of the passes of 32, cut to the columns the matrix has
    for (size_t c0 = 0; c0 < r; c0 += 32)
      if (!window(N, r, c0, std::min<size_t>(32, r - c0), 0)) return 1;
    // [1, 1 + T): the T probe columns behind the data column -- as the panel's window (the source's columns from 0) and as the source's
    const size_t T = std::min<size_t>(r, 31);
    if (!window(N, r, 0, T, 1)) return 1;
    if (r > 1 && !window(N, r, 1, std::min<size_t>(T, r - 1), 0)) return 1;
    if (!window(N, r, 0, 0, 0)) return 1;                                 // an empty window writes nothing
  }
  std::printf("ok %d checks\n", checks);
  return 0;
}
