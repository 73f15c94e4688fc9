// The two copies between a row-major host matrix, as a caller of the C ABI holds it, and a panel of the iterative solver (launch.h: columns
// stored one after another, entry (i, c) at [c * ld + i]).  Host-only (no HIP), so that tests/c/iter_panel_check.cpp can run them under
// the sanitisers.  Both touch the `ncols` columns of their window and the `n` rows alone: whatever else the destination holds stays.
#pragma once
#include <cstddef>

namespace mogp {

// panel[(pc0 + c) * ldp + i] = rows[i * ldr + c0 + c] for i < n, c < ncols
inline void rows_to_panel(const double* rows, size_t n, size_t ldr, size_t c0, size_t ncols, double* panel, size_t ldp, size_t pc0) {
  for (size_t i = 0; i < n; ++i)
    for (size_t c = 0; c < ncols; ++c) panel[(pc0 + c) * ldp + i] = rows[i * ldr + c0 + c];
}

// rows[i * ldr + c0 + c] = panel[(pc0 + c) * ldp + i] for i < n, c < ncols
inline void panel_to_rows(double* rows, size_t n, size_t ldr, size_t c0, size_t ncols, const double* panel, size_t ldp, size_t pc0) {
  for (size_t i = 0; i < n; ++i)
    for (size_t c = 0; c < ncols; ++c) rows[i * ldr + c0 + c] = panel[(pc0 + c) * ldp + i];
}

}  // namespace mogp
