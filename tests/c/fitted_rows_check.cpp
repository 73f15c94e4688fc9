// Host check of with_rows (csrc/fitted_rows.h), with its own sweep: exits non-zero at the first property that fails.  Over B in
// {1, 2, 5, 8}, every subset of the B emulators as ids, and two sets of row lengths (with 0 and 1 among them), with seven arrays -- a
// NaN-filled and an untouched double output of different row length, a null output, a 0-filled and an untouched int output, a gathered
// input and a null input -- and a run that writes a known function of (emulator, column):
//   * with every emulator in ids, run sees the caller's pointers themselves;
//   * with none, run is not called and the fills are applied;
//   * otherwise run gets compact rows that are not the caller's, the inputs arrive in ids order, every output row lands at ids[k] and
//     nowhere else, the other rows are NaN / 0 where a fill was asked for and keep their sentinel where not;
//   * a null array is null inside run, and the caller's input is never written.
// tests/test_fitted_rows_host.py builds it with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fitted_rows.h"

using mogp::Rows;

static const double SENT = -7.5;
static const int ISENT = -9;
static double val(int array, int emulator, size_t col) { return 1000. * array + 10. * emulator + (double)col + 0.25; }

static int fail(const char* what, int B, unsigned mask, int lens) {
  std::printf("FAILED %s: B=%d ids mask=0x%x row lengths set %d\n", what, B, mask, lens);
  return 1;
}

int main() {
  const int Bs[] = {1, 2, 5, 8};
  const size_t lens[2][5] = {{3, 1, 2, 1, 4}, {0, 5, 1, 0, 1}};      // rows of: NaN-filled double, untouched double, 0-filled int, untouched int, input
  long cases = 0;
  for (int B : Bs)
    for (unsigned mask = 0; mask < (1u << B); ++mask)
      for (int L = 0; L < 2; ++L) {
        const size_t r0 = lens[L][0], r1 = lens[L][1], r2 = lens[L][2], r3 = lens[L][3], r4 = lens[L][4];
        std::vector<int> ids;
        for (int i = 0; i < B; ++i)
          if (mask >> i & 1) ids.push_back(i);
        const size_t nf = ids.size();
        // exactly sized, so that the address sanitiser sees any write past a row
        std::vector<double> o0(B * r0, SENT), o1(B * r1, SENT), in(B * r4);
        std::vector<int> o2(B * r2, ISENT), o3(B * r3, ISENT);
        for (int i = 0; i < B; ++i)
          for (size_t c = 0; c < r4; ++c) in[i * r4 + c] = val(4, i, c);
        const std::vector<double> in0 = in;
        const std::vector<Rows> arrays = {Rows::out(o0.data(), r0, true),       Rows::out(o1.data(), r1, false), Rows::out((double*)nullptr, 3, true),
                                          Rows::out(o2.data(), r2, true),       Rows::out(o3.data(), r3, false), Rows::in(in.data(), r4),
                                          Rows::in(nullptr, 2)};
        int calls = 0;
        const char* bad = nullptr;
        mogp::with_rows(B, ids, arrays, [&](const std::vector<Rows>& a) {
          ++calls;
          if (a.size() != arrays.size()) { bad = "run gets every array"; return; }
          if (a[2].p || a[6].p) { bad = "a null array is null inside run"; return; }
          for (size_t j = 0; j < a.size(); ++j) {
            if (a[j].kind != arrays[j].kind || a[j].row != arrays[j].row) { bad = "kind and row length are the caller's"; return; }
            const bool same = a[j].p == arrays[j].p;
            if ((int)nf == B && !same) { bad = "all emulators: the caller's own pointers"; return; }
            if ((int)nf != B && same && arrays[j].p && arrays[j].row) { bad = "some emulators: compact scratch"; return; }
          }
          for (size_t k = 0; k < nf; ++k) {
            for (size_t c = 0; c < r4; ++c)
              if (a[5].d()[k * r4 + c] != val(4, ids[k], c)) { bad = "inputs in ids order"; return; }
            for (size_t c = 0; c < r0; ++c) a[0].d()[k * r0 + c] = val(0, ids[k], c);
            for (size_t c = 0; c < r1; ++c) a[1].d()[k * r1 + c] = val(1, ids[k], c);
            for (size_t c = 0; c < r2; ++c) a[3].i()[k * r2 + c] = (int)val(2, ids[k], c);
            for (size_t c = 0; c < r3; ++c) a[4].i()[k * r3 + c] = (int)val(3, ids[k], c);
          }
        });
        if (bad) return fail(bad, B, mask, L);
        if (calls != (nf ? 1 : 0)) return fail("run is called once, and not at all without emulators", B, mask, L);
        if (in != in0) return fail("the caller's input is not written", B, mask, L);
        for (int i = 0; i < B; ++i) {
          const bool ran = mask >> i & 1;
          for (size_t c = 0; c < r0; ++c) {
            const double x = o0[i * r0 + c];
            if (ran ? x != val(0, i, c) : !std::isnan(x)) return fail("NaN-filled double output", B, mask, L);
          }
          for (size_t c = 0; c < r1; ++c)
            if (o1[i * r1 + c] != (ran ? val(1, i, c) : SENT)) return fail("untouched double output", B, mask, L);
          for (size_t c = 0; c < r2; ++c)
            if (o2[i * r2 + c] != (ran ? (int)val(2, i, c) : 0)) return fail("0-filled int output", B, mask, L);
          for (size_t c = 0; c < r3; ++c)
            if (o3[i * r3 + c] != (ran ? (int)val(3, i, c) : ISENT)) return fail("untouched int output", B, mask, L);
        }
        ++cases;
      }
  std::printf("%ld cases ok\n", cases);
  return 0;
}
