// The rule for a partly fitted model, once and host-only: run the emulators `ids` of an engine on compact rows, scatter the results to
// their own rows of the caller's arrays and fill the rows of the others.  No HIP here: tests/c/fitted_rows_check.cpp sweeps it on the host.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <functional>
#include <limits>
#include <vector>

namespace mogp {

// One array of the caller: one row of `row` elements per emulator of the engine; p == null: not asked for, and null for the run.
struct Rows {
  enum Kind { OUT_DOUBLE, OUT_INT, IN_DOUBLE } kind;
  void* p;
  size_t row;
  bool fill;       // outputs: the rows of emulators that do not run become NaN (double) or 0 (int); false: they are left untouched
  static Rows out(double* p, size_t row, bool nan_fill) { return {OUT_DOUBLE, p, row, nan_fill}; }
  static Rows out(int* p, size_t row, bool zero_fill) { return {OUT_INT, p, row, zero_fill}; }
  static Rows in(const double* p, size_t row) { return {IN_DOUBLE, const_cast<double*>(p), row, false}; }   // gathered, never written
  double* d() const { return static_cast<double*>(p); }
  int* i() const { return static_cast<int*>(p); }
  size_t row_bytes() const { return row * (kind == OUT_INT ? sizeof(int) : sizeof(double)); }
};

// run(a) computes the emulators `ids` (ascending, out of B): a[j] is arrays[j] with ids.size() compact rows, row k for emulator ids[k] --
// inputs gathered before the run, outputs scattered after it.  With every emulator in ids, run gets the caller's arrays themselves: no
// copy, no fill.  Otherwise the fills come first, and run is not called when ids is empty.
inline void with_rows(int B, const std::vector<int>& ids, const std::vector<Rows>& arrays, const std::function<void(const std::vector<Rows>&)>& run) {
  const size_t nf = ids.size(), na = arrays.size();
  if ((int)nf == B) {
    run(arrays);
    return;
  }
  for (const Rows& a : arrays) {
    if (!a.p || !a.fill) continue;
    if (a.kind == Rows::OUT_INT) std::fill(a.i(), a.i() + (size_t)B * a.row, 0);
    else std::fill(a.d(), a.d() + (size_t)B * a.row, std::numeric_limits<double>::quiet_NaN());
  }
  if (nf == 0) return;
  std::vector<std::vector<char>> tmp(na);
  std::vector<Rows> buf = arrays;
  for (size_t j = 0; j < na; ++j) {
    const Rows& a = arrays[j];
    if (!a.p) continue;
    const size_t rb = a.row_bytes();
    tmp[j].resize(nf * rb);
    buf[j].p = tmp[j].data();
    if (a.kind == Rows::IN_DOUBLE && rb)
      for (size_t k = 0; k < nf; ++k) std::memcpy(tmp[j].data() + k * rb, static_cast<const char*>(a.p) + (size_t)ids[k] * rb, rb);
  }
  run(buf);
  for (size_t j = 0; j < na; ++j) {
    const Rows& a = arrays[j];
    const size_t rb = a.row_bytes();
    if (!a.p || a.kind == Rows::IN_DOUBLE || !rb) continue;
    for (size_t k = 0; k < nf; ++k) std::memcpy(static_cast<char*>(a.p) + (size_t)ids[k] * rb, tmp[j].data() + k * rb, rb);
  }
}

}  // namespace mogp
