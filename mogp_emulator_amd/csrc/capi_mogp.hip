// MultiOutputGP_GPU: creation, the parts and their driver, accessors, priors, eval / fit, Hessian and the multi-start fit
#include <limits>
#include <map>
#include <thread>

#include "capi_internal.h"

using namespace mogp;
using namespace mogp::capi;

namespace mogp {
namespace capi {
// ---- running the parts of a multi-part handle ------------------------------------------------------
// One mutex per device: the parts that share a device take it for the whole operation, so that two parts never have kernels in
// flight on one device at once (the one-launch Cholesky and the back-substitution chain spin-wait on the device and assume
// they are not co-resident with another such launch).  Never destroyed (threads of other handles may still hold one at exit).
std::mutex& device_mutex(int device) {
  static std::mutex* reg = new std::mutex();
  static std::map<int, std::unique_ptr<std::mutex>>* mus = new std::map<int, std::unique_ptr<std::mutex>>();
  std::lock_guard<std::mutex> lk(*reg);
  std::unique_ptr<std::mutex>& m = (*mus)[device];
  if (!m) m.reset(new std::mutex());
  return *m;
}
std::string part_tag(const mogp_part& p) {
  return " [part on device " + std::to_string(p.device) + ", emulators [" + std::to_string(p.lo) + ", " + std::to_string(p.hi) + ")]";
}
// f(part, k) for every part, one host thread per part, each under its device's mutex and a DeviceGuard.  The first failure in part order
// is rethrown on the calling thread once every part has finished, its message naming the part.  A handle with ONE part is the plain
// single-engine model: f runs on the calling thread under a DeviceGuard -- no thread, no mutex, the message as it was thrown.
void for_parts(mogp_mogp* h, const std::function<void(mogp_part&, int)>& f) {
  const int np = (int)h->parts.size();
  if (np == 1) {
    DeviceGuard g(h->parts[0].device);
    f(h->parts[0], 0);
    return;
  }
  std::vector<std::exception_ptr> err(np);
  std::vector<std::thread> th;
  th.reserve(np);
  try {
    for (int k = 0; k < np; ++k)
      th.emplace_back([&, k] {
        mogp_part& p = h->parts[k];
        try {
          std::lock_guard<std::mutex> lk(device_mutex(p.device));
          DeviceGuard g(p.device);
          f(p, k);
        } catch (...) {
          err[k] = std::current_exception();
        }
      });
  } catch (...) {
    for (auto& t : th) t.join();
    throw;
  }
  for (auto& t : th) t.join();
  for (int k = 0; k < np; ++k) {
    if (!err[k]) continue;
    try {
      std::rethrow_exception(err[k]);
    } catch (const std::exception& e) {
      throw std::runtime_error(std::string(e.what()) + part_tag(h->parts[k]));
    } catch (...) {
      throw std::runtime_error("unknown error" + part_tag(h->parts[k]));
    }
  }
}
// work on the part that holds emulator i, on the calling thread
mogp_part& part_of(mogp_mogp* h, int i) {
  for (auto& p : h->parts)
    if (i >= p.lo && i < p.hi) return p;
  throw std::runtime_error("Invalid emulator index");
}
std::vector<int> fitted_ids(const Engine* e) {
  std::vector<int> ids;
  for (int i = 0; i < e->B; ++i)
    if (e->gp[i].has_data && e->gp[i].factored) ids.push_back(i);
  return ids;
}
std::vector<int> all_ids(int n) {
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = i;
  return ids;
}
int widest_n_theta(const mogp_mogp* h) {
  int widest = 0;
  for (const auto& v : h->views) widest = std::max(widest, v.eng->n_theta(v.idx));
  return widest;
}
}  // namespace capi
}  // namespace mogp

extern "C" {

static mogp_mogp* mogp_create(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                              const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size, bool analytic,
                              const int* devices, int n_devices) {
  try {
    MeanFunc mf;
    if (mean) mf = mean->mf;
    std::unique_ptr<mogp_mogp> h(new mogp_mogp);
    if (!devices) {
      // no device list: one engine on the current device
      h->parts.resize(1);
      mogp_part& p = h->parts[0];
      p.eng.reset(new Engine(inputs, n, D, targets, n_out, testing_size, mf, kernel_type, nugget_type, nugget_size, analytic));
      p.device = p.eng->device_id();
      p.lo = 0;
      p.hi = n_out;
    } else {
      if (n_out < 1) throw std::runtime_error("inputs must have shape (n, D) with n, D >= 1");
      const int count = mogp_device_count();
      for (int k = 0; k < n_devices; ++k)
        if (devices[k] < 0 || devices[k] >= count)
          throw std::runtime_error("device ordinal " + std::to_string(devices[k]) + " is out of range [0, " + std::to_string(count) + ")");
      // contiguous blocks of ceil(n_out / n_devices) emulators (dist.shard_bounds); empty blocks are dropped
      const int per = (n_out + n_devices - 1) / n_devices;
      for (int k = 0; k < n_devices; ++k) {
        const int lo = std::min(k * per, n_out), hi = std::min(lo + per, n_out);
        if (lo >= hi) continue;
        h->parts.emplace_back();
        mogp_part& p = h->parts.back();
        p.device = devices[k];
        p.lo = lo;
        p.hi = hi;
        DeviceGuard g(p.device);
        p.eng.reset(new Engine(inputs, n, D, targets + (size_t)lo * n, hi - lo, testing_size, mf, kernel_type, nugget_type, nugget_size,
                               analytic));
      }
    }
    h->eng = h->parts[0].eng.get();
    h->views.resize(n_out);
    for (auto& p : h->parts)
      for (int i = p.lo; i < p.hi; ++i) h->views[i] = mogp_densegp{p.eng.get(), i - p.lo, false};
    h->nug_size0 = nugget_size;
    h->nug_type0 = nugget_type;
    return h.release();
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
mogp_mogp* mogp_mogp_create(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                            const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size) {
  return mogp_create(inputs, n, D, targets, n_out, testing_size, mean, kernel_type, nugget_type, nugget_size, false, nullptr, 0);
}
mogp_mogp* mogp_mogp_create_analytic_mean(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                                          const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size) {
  return mogp_create(inputs, n, D, targets, n_out, testing_size, mean, kernel_type, nugget_type, nugget_size, true, nullptr, 0);
}
mogp_mogp* mogp_mogp_create_on_devices(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                                       const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size, int analytic_mean,
                                       const int* devices, int n_devices) {
  if (!devices || n_devices < 1) {
    g_err = "create_on_devices: at least one device is needed";
    return nullptr;
  }
  return mogp_create(inputs, n, D, targets, n_out, testing_size, mean, kernel_type, nugget_type, nugget_size, analytic_mean != 0, devices,
                     n_devices);
}
void mogp_mogp_destroy(mogp_mogp* h) { delete h; }
int mogp_mogp_n_parts(const mogp_mogp* h) { return (int)h->parts.size(); }
int mogp_mogp_part(const mogp_mogp* h, int k, int* device, int* lo, int* hi) {
  if (k < 0 || k >= (int)h->parts.size()) {
    g_err = "Invalid part index";
    return 1;
  }
  const mogp_part& p = h->parts[k];
  if (device) *device = p.device;
  if (lo) *lo = p.lo;
  if (hi) *hi = p.hi;
  return 0;
}
int mogp_mogp_n(const mogp_mogp* h) { return h->eng->n; }
int mogp_mogp_D(const mogp_mogp* h) { return h->eng->D; }
int mogp_mogp_n_emulators(const mogp_mogp* h) { return (int)h->views.size(); }
int mogp_mogp_inputs(const mogp_mogp* h, double* out) {
  std::memcpy(out, h->eng->hX.data(), h->eng->hX.size() * sizeof(double));
  return 0;
}
int mogp_mogp_targets(const mogp_mogp* h, double* out) {
  for (const auto& p : h->parts)
    std::memcpy(out + (size_t)p.lo * h->eng->n, p.eng->hT.data(), p.eng->hT.size() * sizeof(double));
  return 0;
}
mogp_densegp* mogp_mogp_emulator(mogp_mogp* h, int index) {
  if (index < 0 || index >= (int)h->views.size()) {
    g_err = "Invalid emulator index";
    return nullptr;
  }
  return &h->views[index];
}
int mogp_mogp_get_nugget_type(const mogp_mogp* h) { return h->nug_type0; }
double mogp_mogp_get_nugget_size(const mogp_mogp* h) { return h->nug_size0; }
int mogp_mogp_get_fitted_indices(const mogp_mogp* h, int* out) {
  int c = 0;
  for (int i = 0; i < (int)h->views.size(); ++i)
    if (h->views[i].eng->gp[h->views[i].idx].has_data) out[c++] = i;
  return c;
}
int mogp_mogp_get_unfitted_indices(const mogp_mogp* h, int* out) {
  int c = 0;
  for (int i = 0; i < (int)h->views.size(); ++i)
    if (!h->views[i].eng->gp[h->views[i].idx].has_data) out[c++] = i;
  return c;
}
int mogp_mogp_reset_fit_status(mogp_mogp* h) {
  for (auto& v : h->views) mogp_densegp_reset_theta_fit_status(&v);
  return 0;
}
int mogp_mogp_create_priors_for_emulator(mogp_mogp* h, int index, int n_corr, const int* ct, const double* cp, int covt, const double* covp,
                                         int nugt, const double* nugp) {
  return guarded([&] {
    if (index < 0 || index >= (int)h->views.size()) throw std::runtime_error("Invalid emulator index for setting priors");
    set_priors(h->views[index].eng, h->views[index].idx, n_corr, ct, cp, covt, covp, nugt, nugp);
  });
}
int mogp_mogp_eval(mogp_mogp* h, const double* thetas, int n_rows, int n_cols, double* logpost_out, double* grad_out, int* ok_out) {
  return guarded([&] {
    if (n_rows != (int)h->views.size()) throw std::runtime_error("thetas must have one row per emulator");
    for (const auto& v : h->views)
      if (n_cols != v.eng->n_theta(v.idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    for_parts(h, [&](mogp_part& p, int) {
      const int nb = p.hi - p.lo;
      const std::vector<int> ids = all_ids(nb);
      std::vector<const double*> th(nb);
      for (int i = 0; i < nb; ++i) th[i] = thetas + (size_t)(p.lo + i) * n_cols;
      std::vector<double> f(nb);
      std::vector<int> ok(nb);
      p.eng->eval(ids, th, grad_out != nullptr, f.data(), grad_out ? grad_out + (size_t)p.lo * n_cols : nullptr, n_cols, ok.data());
      if (logpost_out) std::memcpy(logpost_out + p.lo, f.data(), sizeof(double) * nb);
      if (ok_out) std::memcpy(ok_out + p.lo, ok.data(), sizeof(int) * nb);
    });
  });
}
int mogp_mogp_fit(mogp_mogp* h, const double* thetas, int n_rows, int n_cols) {
  return guarded([&] {
    const int B = (int)h->views.size();
    std::vector<int> ok(B);
    if (mogp_mogp_eval(h, thetas, n_rows, n_cols, nullptr, nullptr, ok.data())) throw std::runtime_error(g_err);
    for (int i = 0; i < B; ++i) {
      const GPState& g = h->views[i].eng->gp[h->views[i].idx];
      if (!ok[i] && !(g.nug_type == NUG_PIVOT && g.factored)) {
        if (g.nug_type == NUG_ADAPTIVE) throw std::runtime_error("All attempts at factorization failed. Last return code 1");
        throw std::runtime_error("Unable to factorize matrix using selected nugget type");
      }
    }
  });
}
int mogp_mogp_fit_emulator(mogp_mogp* h, int index, const double* theta, int len) {
  return guarded([&] {
    if (index < 0 || index >= (int)h->views.size()) throw std::runtime_error("Invalid emulator index");
    mogp_part& p = part_of(h, index);
    std::unique_lock<std::mutex> lk;      // (parts that share a device take turns; a single part has nobody to wait for)
    if (h->multi()) lk = std::unique_lock<std::mutex>(device_mutex(p.device));
    DeviceGuard g(p.device);
    p.eng->fit_one(index - p.lo, theta, len);
  });
}
int mogp_mogp_hessian(mogp_mogp* h, const double* thetas, int n_rows, int n_cols, double* hess_out, int* ok_out) {
  return guarded([&] {
    if (n_rows != (int)h->views.size()) throw std::runtime_error("thetas must have one row per emulator");
    if (!thetas || !hess_out) throw std::runtime_error("logpost_hessian: null buffer");
    if (n_cols != widest_n_theta(h)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    const size_t blk = (size_t)n_cols * n_cols;
    std::fill(hess_out, hess_out + (size_t)n_rows * blk, std::numeric_limits<double>::quiet_NaN());
    if (ok_out) std::fill(ok_out, ok_out + n_rows, 0);
    for_parts(h, [&](mogp_part& p, int) {
      std::vector<int> ids;
      std::vector<const double*> th;
      for (int i = 0; i < p.hi - p.lo; ++i) {
        const double* row = thetas + (size_t)(p.lo + i) * n_cols;
        if (std::isnan(row[0])) continue;
        ids.push_back(i);
        th.push_back(row);
      }
      if (ids.empty()) return;
      std::vector<double> Hs(ids.size() * blk);
      std::vector<int> ok(ids.size());
      p.eng->hessian(ids, th, Hs.data(), n_cols, ok.data());
      for (size_t k = 0; k < ids.size(); ++k) {
        if (ok[k]) std::memcpy(hess_out + (size_t)(p.lo + ids[k]) * blk, Hs.data() + k * blk, blk * sizeof(double));
        if (ok_out) ok_out[p.lo + ids[k]] = ok[k];
      }
    });
  });
}
int mogp_fit_GP_MAP(mogp_mogp* h, int n_tries, const double* theta0, int theta0_len) {
  return guarded([&] {
    // every starting point is drawn here, in the order of the unsharded model (start-major), from part 0's rng -- seeded as a single
    // engine's is -- with each emulator's own priors; each part then runs its block.  The end point of a run does not depend on the
    // batch it ran in (Engine::run_pool), so the result is the single-engine one whatever the split.  With one part this is
    // Engine::fit_map: the same checks in the same order, the same draws from the same generator.
    if (n_tries < 1) throw std::runtime_error("number of attempts must be positive");
    std::vector<std::pair<const Engine*, int>> emus;
    for (const auto& v : h->views) {
      if (theta0_len > 0 && theta0_len != v.eng->n_theta(v.idx)) throw std::runtime_error("length of theta0 must equal n_params of GP.");
      emus.emplace_back(v.eng, v.idx);
    }
    const Engine::Starts x0 = Engine::draw_starts(h->eng->random(), emus, n_tries, theta0, theta0_len);
    for_parts(h, [&](mogp_part& p, int) {
      const int nb = p.hi - p.lo;
      Engine::Starts sub(n_tries, std::vector<std::vector<double>>(nb));
      for (int s = 0; s < n_tries; ++s)
        for (int i = 0; i < nb; ++i) sub[s][i] = x0[s][p.lo + i];
      p.eng->fit_map_from(all_ids(nb), sub);
    });
  });
}

}  // extern "C"
