// Shared by the capi*.hip units only: the handle types behind include/mogp_hip.h, the error channel, the guards that turn C++
// exceptions into (non-zero status, thread-local message), and the driver of a multi-part handle.  Everything but the handle types
// (which the C header names) sits in mogp::capi, so that the library's C symbols stay the 122 of the header.
#pragma once
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>

#include "../../include/mogp_hip.h"
#include "engine.h"
#include "fitted_rows.h"

struct mogp_meanfunc { mogp::MeanFunc mf; };
struct mogp_densegp { mogp::Engine* eng; int idx; bool owns; };
// One part of a MultiOutputGP_GPU: the engine of emulators [lo, hi) on `device`.  A handle created without a device list has one
// part on the current device; mogp_mogp_create_on_devices splits the emulators into contiguous blocks, one part per non-empty block.
struct mogp_part { std::unique_ptr<mogp::Engine> eng; int device = 0; int lo = 0, hi = 0; };
struct mogp_mogp {
  std::vector<mogp_part> parts;
  mogp::Engine* eng = nullptr;           // part 0's engine: the whole model when there is one part
  std::vector<mogp_densegp> views;       // emulator i: borrowed view into its part's engine at index i - lo
  double nug_size0;
  int nug_type0;
  bool multi() const { return parts.size() > 1; }
  ~mogp_mogp() {
    for (auto& p : parts) {
      if (!p.eng) continue;
      try {
        mogp::DeviceGuard g(p.device);
        p.eng.reset();
      } catch (...) {
        p.eng.reset();
      }
    }
  }
};

namespace mogp {
namespace capi {

// The message of the last failure on this host thread: ONE object for every unit (defined in capi.hip; mogp_last_error reads it).
extern thread_local std::string g_err;

// f(); 0, or 1 with the message stored
template <class F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return 1;
  } catch (...) {
    g_err = "unknown error";
    return 1;
  }
}
// the same with the work of a DenseGP handle (own or borrowed) on its engine's device
template <class F>
int on_engine_device(const mogp_densegp* h, F&& f) {
  return guarded([&] {
    DeviceGuard g(h->eng->device_id());
    f();
  });
}

inline void check_D(int D, const Engine* e, const char* msg = "testing points must have D columns") {
  if (D != e->D) throw std::runtime_error(msg);
}
void check_sobol_args(int D, const Engine* e, const double* S, const double* ST, const double* mean_out, const double* variance_out, int unc,
                      const double* emulator_variance_out);
void set_priors(Engine* eng, int i, int n_corr, const int* ct, const double* cp, int covt, const double* covp, int nugt, const double* nugp);

// capi_mogp.hip: running the parts of a multi-part handle
std::mutex& device_mutex(int device);
std::string part_tag(const mogp_part& p);
void for_parts(mogp_mogp* h, const std::function<void(mogp_part&, int)>& f);
mogp_part& part_of(mogp_mogp* h, int i);
std::vector<int> fitted_ids(const Engine* e);
std::vector<int> all_ids(int n);           // 0 .. n-1: every emulator of a part
int widest_n_theta(const mogp_mogp* h);

}  // namespace capi
}  // namespace mogp
