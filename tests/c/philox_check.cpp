// Host build of csrc/philox_dev.h, the normal generator of sample_posterior: prints
//   kat <x0> <x1> <x2> <x3>      the block function at Random123's three known-answer inputs for philox4x32-10 (hex words)
//   z <draw> <v0> <v1> ...       the (7, 129) block of normals of seed 2024, stream 2 (%.17g: round-trip exact)
// tests/test_sample_host.py builds it with -fsanitize=address,undefined and compares the words exactly and the normals with its NumPy
// restatement.
#include <cstdio>

#include "philox_dev.h"

int main() {
  const unsigned in[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                             {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                             {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
  for (const auto& c : in) {
    const mogp::PhiloxWords w = mogp::philox4x32_10(c[0], c[1], c[2], c[3], c[4], c[5]);
    std::printf("kat %08x %08x %08x %08x\n", w.x[0], w.x[1], w.x[2], w.x[3]);
  }
  const int S = 7, m = 129;
  for (int s = 0; s < S; ++s) {
    std::printf("z %d", s);
    for (int p = 0; 2 * p < m; ++p) {
      double z0, z1;
      mogp::philox_normal_pair(2024ull, 2u, (unsigned)s, (unsigned)p, z0, z1);
      std::printf(" %.17g", z0);
      if (2 * p + 1 < m) std::printf(" %.17g", z1);
    }
    std::printf("\n");
  }
  return 0;
}
