// Limits and LDS layout of the Latin-hypercube annealer (kernels_lhs.hip; DESIGN.md section 3 "Design"), host-only arithmetic so that
// tests/c/lhs_plan_check.cpp can check it without a device, as predict_plan.h / chol_schedule.h are.
//
// One workgroup owns one chain and keeps its level matrix P (n, D) in LDS, COLUMN-major (entry (j, d) at index d n + j: the threads of a
// wave read consecutive j of one column).  Two storage widths:
//   narrow  n <= 65536: one 16-bit word per level.                                        bytes = 2 n D
//   wide    n >  65536: the low 16 bits as above, and bit 16 in a bit plane (bit (idx & 31) of word idx >> 5) behind them.  A plain 32-bit
//           word per level can never fit -- n > 65536 levels of 4 bytes are more than 256 KiB, the workgroup has 160 KiB -- and the bound
//           below keeps n < 2^17, so seventeen bits are enough.                             bytes = 2 M + M / 8,  M = n D rounded up to 32
// The workgroup may use LHS_LDS_BYTES - LHS_LDS_RESERVED for the levels (the rest: the term buffer of the sum, the wave sums and what the compiler adds):
//   narrow  n D <= 75264            wide  n D <= 70816 (only D = 1 reaches it)
// so n = 5000 x D = 10 and n = 65536 / 70000 x D = 1 are served.  Larger shapes are refused by name; a global-memory variant is out of scope.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mogp {

constexpr int LHS_THREADS = 256;                     // summing threads of a chain: they fix the order of every sum (4 waves)
constexpr int LHS_HW = 1024;                         // hardware threads of the chain's workgroup: four compute the terms of one summing thread
constexpr long LHS_LDS_BYTES = 160 * 1024;           // LDS of one CU = the most one workgroup can take
constexpr long LHS_LDS_RESERVED = 13 * 1024;         // the term buffer (2 x 3 x 256 doubles), the wave sums, and what the compiler adds
constexpr long LHS_NARROW_MAX_N = 65536;
constexpr long LHS_NARROW_MAX_ND = (LHS_LDS_BYTES - LHS_LDS_RESERVED) / 2;                  // 75264
constexpr long LHS_WIDE_MAX_ND = (LHS_LDS_BYTES - LHS_LDS_RESERVED) * 8 / 17 / 32 * 32;     // 70816
constexpr int LHS_MAX_D = 80;
constexpr int LHS_POWER_BITS = 1000;                 // (D (n - 1)^2)^q must stay below 2^1000

struct LhsLayout {
  bool wide;            // seventeen-bit levels
  long cells;           // n D (wide: rounded up to 32)
  long hi_offset;       // byte offset of the bit plane (wide), = bytes otherwise
  long bytes;           // dynamic LDS of the workgroup
  bool fits;
};

inline LhsLayout lhs_layout(long n, long D) {
  LhsLayout L;
  L.wide = n > LHS_NARROW_MAX_N;
  const long nd = n * D;
  L.cells = L.wide ? (nd + 31) / 32 * 32 : nd;
  L.hi_offset = 2 * L.cells;
  L.bytes = L.wide ? L.hi_offset + L.cells / 8 : L.hi_offset;
  L.fits = L.bytes <= LHS_LDS_BYTES - LHS_LDS_RESERVED;
  return L;
}

// true when (D (n - 1)^2)^q >= 2^LHS_POWER_BITS, exactly (a little-endian number of 32-bit limbs times a factor below 2^53)
inline bool lhs_power_overflows(long n, long D, long q) {
  const unsigned __int128 M = (unsigned __int128)D * (unsigned __int128)(n - 1) * (unsigned __int128)(n - 1);
  if (M <= 1) return false;
  if (q > LHS_POWER_BITS) return true;               // M >= 2
  std::vector<uint32_t> v{1u};
  for (long k = 0; k < q; ++k) {
    unsigned __int128 carry = 0;
    for (size_t i = 0; i < v.size(); ++i) {
      const unsigned __int128 t = (unsigned __int128)v[i] * M + carry;
      v[i] = (uint32_t)t;
      carry = t >> 32;
    }
    while (carry) {
      v.push_back((uint32_t)carry);
      carry >>= 32;
    }
    long bits = 32 * (long)(v.size() - 1);
    for (uint32_t top = v.back(); top; top >>= 1) ++bits;
    if (bits > LHS_POWER_BITS) return true;          // bits > 1000  <=>  value >= 2^1000
  }
  return false;
}

}  // namespace mogp
