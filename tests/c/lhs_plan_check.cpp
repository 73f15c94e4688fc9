// Host check of csrc/lhs_plan.h: the LDS layout and limits of the Latin-hypercube annealer against the documented formulas
//   16-bit levels (n <= 65536): bytes = 2 n D,            accepted iff n D <= 75264
//   17-bit levels (n >  65536): bytes = 2 M + M / 8, M = n D rounded up to 32, accepted iff n D <= 70816
// and the exact overflow test (D (n - 1)^2)^q >= 2^1000.  Prints "edge ..." lines that tests/test_lhs_host.py compares with its own
// restatement, and "cases ok" at the end; exits non-zero at the first property that fails.
#include <cstdio>
#include <cstdlib>

#include "lhs_plan.h"

using namespace mogp;

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);            \
      return 1;                                                     \
    }                                                               \
  } while (0)

int main() {
  REQUIRE(LHS_NARROW_MAX_ND == 75264 && LHS_WIDE_MAX_ND == 70816 && LHS_LDS_BYTES == 163840);
  // the shapes the feature must serve
  REQUIRE(lhs_layout(2000, 10).fits && lhs_layout(5000, 10).fits && lhs_layout(65536, 1).fits && lhs_layout(70000, 1).fits);
  REQUIRE(lhs_layout(300, 80).fits && lhs_layout(2, 1).fits);
  REQUIRE(!lhs_layout(65536, 1).wide && lhs_layout(65537, 1).wide);
  // narrow: the largest accepted and the first refused n D, reached by several (n, D)
  const long narrow_ok[][2] = {{37632, 2}, {1176, 64}, {65536, 1}, {25088, 3}}, narrow_no[][2] = {{37633, 2}, {25089, 3}, {941, 80}};
  for (auto& s : narrow_ok) {
    const LhsLayout L = lhs_layout(s[0], s[1]);
    REQUIRE(L.wide == (s[0] > 65536));
    if (!L.wide) REQUIRE(L.fits && L.bytes == 2 * s[0] * s[1] && L.hi_offset == L.bytes);
  }
  for (auto& s : narrow_no) REQUIRE(!lhs_layout(s[0], s[1]).wide && !lhs_layout(s[0], s[1]).fits && s[0] * s[1] > LHS_NARROW_MAX_ND);
  // wide: only D = 1 can reach it
  REQUIRE(lhs_layout(70816, 1).fits && !lhs_layout(70817, 1).fits && !lhs_layout(65537, 2).fits);
  for (long n = 65537; n <= 90000; n += 7) {
    const LhsLayout L = lhs_layout(n, 1);
    const long M = (n + 31) / 32 * 32;
    REQUIRE(L.wide && L.cells == M && L.hi_offset == 2 * M && L.bytes == 2 * M + M / 8 && L.hi_offset % 4 == 0);
    REQUIRE(L.fits == (n <= LHS_WIDE_MAX_ND));
    REQUIRE(!L.fits || (n < (1L << 17) && L.bytes + LHS_LDS_RESERVED <= LHS_LDS_BYTES));
  }
  for (long n = 2; n <= 65536; n = n * 3 / 2 + 1)
    for (long D = 1; D <= LHS_MAX_D; D += 13) REQUIRE(lhs_layout(n, D).fits == (n * D <= LHS_NARROW_MAX_ND));
  std::printf("edge narrow %ld %d %d\n", LHS_NARROW_MAX_ND, (int)lhs_layout(LHS_NARROW_MAX_ND / 2, 2).fits, (int)lhs_layout(LHS_NARROW_MAX_ND / 2 + 1, 2).fits);
  std::printf("edge wide %ld %d %d\n", LHS_WIDE_MAX_ND, (int)lhs_layout(LHS_WIDE_MAX_ND, 1).fits, (int)lhs_layout(LHS_WIDE_MAX_ND + 1, 1).fits);
  // overflow: 2^1000 exactly is refused, one step below is not
  REQUIRE(!lhs_power_overflows(2, 1, 1000000));                     // R = 1 always
  REQUIRE(lhs_power_overflows(3, 1, 500) && !lhs_power_overflows(3, 1, 499));           // 4^500 = 2^1000
  REQUIRE(lhs_power_overflows(2, 2, 1000) && !lhs_power_overflows(2, 2, 999));          // 2^1000
  REQUIRE(lhs_power_overflows(2, 3, 631) && !lhs_power_overflows(2, 3, 630));           // 3^631 > 2^1000 > 3^630
  REQUIRE(!lhs_power_overflows(2000, 10, 5) && !lhs_power_overflows(65536, 1, 5) && lhs_power_overflows(65536, 80, 27));
  for (long q = 1; q <= 40; ++q) std::printf("pow %ld %d %d\n", q, (int)lhs_power_overflows(2000, 10, q), (int)lhs_power_overflows(70000, 1, q));
  std::printf("cases ok\n");
  return 0;
}
