// extern "C" surface of libmogp_hip.so (include/mogp_hip.h).  Every entry point converts C++
// exceptions into (non-zero status, thread-local message); the Python shim raises RuntimeError
// with that message, matching the std::runtime_error -> RuntimeError mapping of pybind11 in the
// reference (bindings.cu).
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/mogp_hip.h"
#include "engine.h"

using namespace mogp;

static thread_local std::string g_err;

struct mogp_meanfunc { MeanFunc mf; };
struct mogp_densegp { Engine* eng; int idx; bool owns; };
// One part of a MultiOutputGP_GPU: the engine of emulators [lo, hi) on `device`.  A handle created without a device list has one
// part on the current device; mogp_mogp_create_on_devices splits the emulators into contiguous blocks, one part per non-empty block.
struct mogp_part { std::unique_ptr<Engine> eng; int device = 0; int lo = 0, hi = 0; };
struct mogp_mogp {
  std::vector<mogp_part> parts;
  Engine* eng = nullptr;                 // part 0's engine: the whole model when there is one part
  std::vector<mogp_densegp> views;       // emulator i: borrowed view into its part's engine at index i - lo
  double nug_size0;
  int nug_type0;
  bool multi() const { return parts.size() > 1; }
  ~mogp_mogp() {
    for (auto& p : parts) {
      if (!p.eng) continue;
      try {
        DeviceGuard g(p.device);
        p.eng.reset();
      } catch (...) {
        p.eng.reset();
      }
    }
  }
};

#define GUARD(body)                      \
  try {                                  \
    body;                                \
    return 0;                            \
  } catch (const std::exception& e) {    \
    g_err = e.what();                    \
    return 1;                            \
  } catch (...) {                        \
    g_err = "unknown error";             \
    return 1;                            \
  }
// the same with the work of a DenseGP handle (own or borrowed) on its engine's device
#define DGUARD(h, body) GUARD({ DeviceGuard dguard_((h)->eng->device_id()); body; })

static void set_priors(Engine* eng, int i, int n_corr, const int* ct, const double* cp, int covt, const double* covp, int nugt,
                       const double* nugp) {
  if (n_corr != eng->NC) throw std::runtime_error("number of correlation priors must equal the number of correlation parameters");
  Priors pr;
  pr.corr.resize(n_corr);
  for (int d = 0; d < n_corr; ++d) {
    pr.corr[d].type = ct[d];
    pr.corr[d].shape = cp[2 * d];
    pr.corr[d].scale = cp[2 * d + 1];
  }
  pr.cov.type = covt; pr.cov.shape = covp[0]; pr.cov.scale = covp[1];
  pr.nug.type = nugt; pr.nug.shape = nugp[0]; pr.nug.scale = nugp[1];
  pr.created = true;
  eng->gp[i].pri = pr;
  eng->gp[i].priors_changed();
}

static void kernel_eval_impl(int kernel_type, int what, const double* x1, int n1, const double* x2, int n2, int D, const double* params,
                             int n_params, double* out) {
  {
    if (kernel_type < 0 || kernel_type > 4) throw std::runtime_error("Unrecognized kernel type\n");
    if (what < 0 || what > 2) throw std::runtime_error("kernel_eval: what must be 0 (f), 1 (deriv) or 2 (inputderiv)");
    if (n1 < 1 || n2 < 1 || D < 1) throw std::runtime_error("kernel inputs must have shape (n, D) with n, D >= 1");
    const bool uniform = kernel_type >= 3;
    const int nc = uniform ? 1 : D;
    if (n_params != nc + 1) throw std::runtime_error("Expected params list of length " + std::to_string(nc + 1));
    const int dk = kernel_type == 3 ? 0 : (kernel_type == 4 ? 1 : kernel_type);
    std::vector<double> P(D + 1);
    for (int d = 0; d < D; ++d) P[d] = std::exp(params[uniform ? 0 : d]);
    P[D] = std::exp(params[nc]);
    const size_t planes = what == 0 ? 1 : (what == 1 ? (size_t)D + 1 : (size_t)D);
    const size_t cnt = planes * (size_t)n1 * n2;
    DevBuf<double> d1((size_t)n1 * D), d2((size_t)n2 * D), dP(P.size()), dO(cnt);
    hip_check(hipMemcpy(d1, x1, (size_t)n1 * D * 8, hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy(d2, x2, (size_t)n2 * D * 8, hipMemcpyHostToDevice), "hipMemcpy");
    hip_check(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice), "hipMemcpy");
    launch_kernel_object(dk, d1, n1, d2, n2, D, dP, what, dO, nullptr);
    std::vector<double> tmp(cnt);
    hip_check(hipMemcpy(tmp.data(), dO, cnt * 8, hipMemcpyDeviceToHost), "hipMemcpy");
    hip_check(hipGetLastError(), "kernel_object_kernel");
    if (what == 1 && uniform) {
      // one shared length scale: d/dtheta_0 = sum of the per-dimension planes (Kernel.py:338-376); then the sigma^2 plane
      const size_t pl = (size_t)n1 * n2;
      for (size_t e = 0; e < pl; ++e) {
        double s = 0.;
        for (int d = 0; d < D; ++d) s += tmp[(size_t)d * pl + e];
        out[e] = s;
        out[pl + e] = tmp[(size_t)D * pl + e];
      }
    } else {
      std::memcpy(out, tmp.data(), cnt * 8);
    }
  }
}


extern "C" {

const char* mogp_last_error(void) { return g_err.c_str(); }
const char* mogp_version(void) { return "mogp-hip 0.1 (gfx950)"; }

int mogp_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}
int mogp_have_compatible_device(void) {
  int c = mogp_device_count();
  for (int d = 0; d < c; ++d) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) return 1;
  }
  return 0;
}
int mogp_set_device(int device) { GUARD(hip_check(hipSetDevice(device), "hipSetDevice")); }

// ---- mean functions ---------------------------------------------------------------------------
mogp_meanfunc* mogp_meanfunc_zero(void) { auto* m = new mogp_meanfunc; m->mf.kind = 0; return m; }
mogp_meanfunc* mogp_meanfunc_fixed(double v) { auto* m = new mogp_meanfunc; m->mf.kind = 1; m->mf.value = v; return m; }
mogp_meanfunc* mogp_meanfunc_const(void) { auto* m = new mogp_meanfunc; m->mf.kind = 2; return m; }
mogp_meanfunc* mogp_meanfunc_poly(const int* dims, const int* powers, int nterms) {
  auto* m = new mogp_meanfunc;
  m->mf.kind = 3;
  m->mf.dims.assign(dims, dims + nterms);
  m->mf.powers.assign(powers, powers + nterms);
  return m;
}
void mogp_meanfunc_destroy(mogp_meanfunc* m) { delete m; }
int mogp_meanfunc_n_params(const mogp_meanfunc* m) { return m->mf.n_params(); }
int mogp_meanfunc_mean_f(const mogp_meanfunc* m, const double* xs, int mm, int D, const double* p, int np, double* out) {
  GUARD(m->mf.mean_f(xs, mm, D, p, np, out));
}
int mogp_meanfunc_mean_deriv(const mogp_meanfunc* m, const double* xs, int mm, int D, const double* p, int np, double* out) {
  GUARD(m->mf.mean_deriv(xs, mm, D, p, np, out));
}
int mogp_meanfunc_mean_inputderiv(const mogp_meanfunc* m, const double* xs, int mm, int D, const double* p, int np, double* out) {
  GUARD(m->mf.mean_inputderiv(xs, mm, D, p, np, out));
}

// ---- DenseGP_GPU --------------------------------------------------------------------------------
static mogp_densegp* densegp_create(const double* inputs, int n, int D, const double* targets, unsigned testing_size,
                                    const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size, bool analytic) {
  try {
    MeanFunc mf;
    if (mean) mf = mean->mf;
    std::unique_ptr<Engine> e(new Engine(inputs, n, D, targets, 1, testing_size, mf, kernel_type, nugget_type, nugget_size, analytic));
    return new mogp_densegp{e.release(), 0, true};
  } catch (const std::exception& e) {
    g_err = e.what();
    return nullptr;
  }
}
mogp_densegp* mogp_densegp_create(const double* inputs, int n, int D, const double* targets, unsigned testing_size,
                                  const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size) {
  return densegp_create(inputs, n, D, targets, testing_size, mean, kernel_type, nugget_type, nugget_size, false);
}
mogp_densegp* mogp_densegp_create_analytic_mean(const double* inputs, int n, int D, const double* targets, unsigned testing_size,
                                                const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size) {
  return densegp_create(inputs, n, D, targets, testing_size, mean, kernel_type, nugget_type, nugget_size, true);
}
int mogp_densegp_set_mean_priors(mogp_densegp* h, int q, const double* b, const double* Binv, const double* Binv_b, double logdetB) {
  DGUARD(h, h->eng->set_mean_priors(h->idx, q, b, Binv, Binv_b, logdetB));
}
int mogp_densegp_n_beta(const mogp_densegp* h) { return h->eng->q; }
int mogp_densegp_get_beta(const mogp_densegp* h, double* out) {
  const auto& b = h->eng->gp[h->idx].beta;
  for (size_t c = 0; c < b.size(); ++c) out[c] = b[c];
  return 0;
}
void mogp_densegp_destroy(mogp_densegp* h) {
  if (!h || !h->owns) return;
  try {
    DeviceGuard g(h->eng->device_id());
    delete h->eng;
  } catch (...) {
  }
  delete h;
}
int mogp_densegp_n(const mogp_densegp* h) { return h->eng->n; }
int mogp_densegp_D(const mogp_densegp* h) { return h->eng->D; }
int mogp_densegp_n_corr(const mogp_densegp* h) { return h->eng->NC; }
int mogp_densegp_n_params(const mogp_densegp* h) { return h->eng->n_data(h->idx); }
int mogp_densegp_n_mean(const mogp_densegp* h) { return h->eng->n_mean(); }
int mogp_densegp_n_data(const mogp_densegp* h) { return h->eng->n_data(h->idx); }
int mogp_densegp_inputs(const mogp_densegp* h, double* out) {
  std::memcpy(out, h->eng->hX.data(), h->eng->hX.size() * sizeof(double));
  return 0;
}
int mogp_densegp_targets(const mogp_densegp* h, double* out) {
  std::memcpy(out, h->eng->hT.data() + (size_t)h->idx * h->eng->n, h->eng->n * sizeof(double));
  return 0;
}
int mogp_densegp_theta_fit_status(const mogp_densegp* h) { return h->eng->gp[h->idx].has_data ? 1 : 0; }
int mogp_densegp_reset_theta_fit_status(mogp_densegp* h) {
  GPState& g = h->eng->gp[h->idx];
  g.unfit();
  std::fill(g.data.begin(), g.data.end(), 0.);
  std::fill(g.meanp.begin(), g.meanp.end(), 0.);
  return 0;
}
int mogp_densegp_get_theta(const mogp_densegp* h, double* data_out, double* mean_out) {
  const GPState& g = h->eng->gp[h->idx];
  if (data_out) std::memcpy(data_out, g.data.data(), g.data.size() * sizeof(double));
  if (mean_out && !g.meanp.empty()) std::memcpy(mean_out, g.meanp.data(), g.meanp.size() * sizeof(double));
  return 0;
}
int mogp_densegp_create_gppriors(mogp_densegp* h, int n_corr, const int* ct, const double* cp, int covt, const double* covp, int nugt,
                                 const double* nugp) {
  DGUARD(h, set_priors(h->eng, h->idx, n_corr, ct, cp, covt, covp, nugt, nugp));
}
int mogp_densegp_priors_logp(const mogp_densegp* h, const double* th, int len, double* out) {
  DGUARD(h, {
    if (len != h->eng->n_data(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    std::vector<double> v(th, th + len);
    *out = h->eng->gp[h->idx].pri.logp(v, h->eng->NC, h->eng->gp[h->idx].nug_type);
  });
}
int mogp_densegp_priors_dlogpdtheta(const mogp_densegp* h, const double* th, int len, double* out) {
  DGUARD(h, {
    if (len != h->eng->n_data(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    std::vector<double> v(th, th + len);
    h->eng->gp[h->idx].pri.dlogpdtheta(v, h->eng->NC, h->eng->gp[h->idx].nug_type, out);
  });
}
int mogp_densegp_priors_sample(mogp_densegp* h, double* out) {
  DGUARD(h, {
    static std::mt19937_64 r(std::random_device{}());
    const int nm = h->eng->n_mean();
    for (int k = 0; k < nm; ++k) out[k] = 0.;
    h->eng->gp[h->idx].pri.sample(r, h->eng->NC, h->eng->gp[h->idx].nug_type, out + nm);
  });
}
int mogp_densegp_fit(mogp_densegp* h, const double* theta, int len) { DGUARD(h, h->eng->fit_one(h->idx, theta, len)); }
int mogp_densegp_get_logpost(mogp_densegp* h, const double* theta, int len, double* out) {
  DGUARD(h, {
    Engine* e = h->eng;
    const int i = h->idx;
    if (len != e->n_theta(i)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    const GPState& g = e->gp[i];
    bool close = g.has_data && g.factored && !g.logpost_stale;
    if (close) {   // gpparams.hpp:204-210 test_close: ||theta - current|| < 1e-8
      double d2 = 0.;
      const int nm = e->n_mean();
      for (int k = 0; k < nm; ++k) d2 += (theta[k] - g.meanp[k]) * (theta[k] - g.meanp[k]);
      for (size_t k = 0; k < g.data.size(); ++k) d2 += (theta[nm + k] - g.data[k]) * (theta[nm + k] - g.data[k]);
      close = std::sqrt(d2) < 1e-8;
    }
    if (!close) e->fit_one(i, theta, len);
    *out = e->gp[i].logpost;
  });
}
int mogp_densegp_logpost_deriv(mogp_densegp* h, double* out, int len) {
  DGUARD(h, {
    Engine* e = h->eng;
    if (len < e->n_theta(h->idx)) throw std::runtime_error("logpost_deriv: the result buffer passed was too small");
    if (!e->gp[h->idx].factored) throw std::runtime_error("logpost_deriv: hyperparameters have not been fit");
    std::vector<int> ids{h->idx};
    e->grad_current(ids, out, len);
  });
}
static void check_batch(const mogp_densegp* h, int m, int D, int out_len, const char* small_msg) {
  if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
  if (out_len < m) throw std::runtime_error(small_msg);
  if ((unsigned)m > h->eng->testing_size)
    throw std::runtime_error("predict_variance_batch: More test points were passed than the maximum batch size");
}
int mogp_densegp_predict(mogp_densegp* h, const double* testing, int D, double* mean_out) {
  DGUARD(h, {
    if (D != h->eng->D) throw std::runtime_error("testing point must have D entries");
    std::vector<int> ids{h->idx};
    h->eng->predict(ids, testing, 1, false, mean_out, nullptr, 1, false, nullptr);
  });
}
int mogp_densegp_predict_variance(mogp_densegp* h, const double* testing, int D, double* mean_out, double* var_out) {
  DGUARD(h, {
    if (D != h->eng->D) throw std::runtime_error("testing point must have D entries");
    std::vector<int> ids{h->idx};
    h->eng->predict(ids, testing, 1, false, mean_out, var_out, 1, false, nullptr);
  });
}
int mogp_densegp_predict_batch(mogp_densegp* h, const double* testing, int m, int D, double* mean_out, int out_len) {
  DGUARD(h, {
    check_batch(h, m, D, out_len, "predict_batch: the result buffer passed was too small to hold the result");
    std::vector<int> ids{h->idx};
    h->eng->predict(ids, testing, m, false, mean_out, nullptr, m, false, nullptr);
  });
}
int mogp_densegp_predict_variance_batch(mogp_densegp* h, const double* testing, int m, int D, double* mean_out, double* var_out, int out_len) {
  DGUARD(h, {
    check_batch(h, m, D, out_len, "predict_variance_batch: The result buffer passed was too small to hold the variance");
    std::vector<int> ids{h->idx};
    h->eng->predict(ids, testing, m, false, mean_out, var_out, m, false, nullptr);
  });
}
int mogp_densegp_predict_deriv(mogp_densegp* h, const double* testing, int m, int D, double* out, int out_rows, int out_cols) {
  DGUARD(h, {
    if (out_rows < m || out_cols != h->eng->D)
      throw std::runtime_error("predict_deriv: the result buffer passed was the wrong shape to hold the result");
    check_batch(h, m, D, m, "");
    std::vector<int> ids{h->idx};
    h->eng->predict(ids, testing, m, false, nullptr, nullptr, m, false, out);        // derivatives only: no cross covariance
  });
}
int mogp_densegp_predict_full_cov(mogp_densegp* h, const double* testing, int m, int D, double* mean_out, double* cov_out) {
  DGUARD(h, {
    if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
    std::vector<int> ids{h->idx};
    h->eng->predict_full_cov(ids, testing, m, mean_out, cov_out);
  });
}
int mogp_densegp_implausibility(mogp_densegp* h, const double* testing, int m, int D, double obs, double obs_var, double discrepancy,
                                int include_nugget, double* out) {
  DGUARD(h, {
    if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
    std::vector<int> ids{h->idx};
    h->eng->implausibility(ids, testing, m, &obs, &obs_var, &discrepancy, include_nugget != 0, 0, out);
  });
}
int mogp_densegp_sobol(mogp_densegp* h, const double* A, const double* B, int N, int D, int unc, int include_nugget, double* S, double* ST,
                       double* mean_out, double* variance_out, double* emulator_variance_out) {
  DGUARD(h, {
    if (D != h->eng->D) throw std::runtime_error("sobol: the sample matrices must have D columns");
    if (!S || !ST || !mean_out || !variance_out) throw std::runtime_error("sobol: null result buffer");
    if (unc && !emulator_variance_out) throw std::runtime_error("sobol: unc needs a buffer for the emulator variance");
    std::vector<int> ids{h->idx};
    h->eng->sobol(ids, A, B, N, unc != 0, include_nugget != 0, S, ST, mean_out, variance_out, unc ? emulator_variance_out : nullptr);
  });
}
int mogp_densegp_logpost_hessian(mogp_densegp* h, const double* theta, int len, double* out) {
  DGUARD(h, {
    Engine* e = h->eng;
    if (len != e->n_theta(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    if (!theta || !out) throw std::runtime_error("logpost_hessian: null buffer");
    std::vector<int> ids{h->idx};
    std::vector<const double*> th{theta};
    int ok = 0;
    e->hessian(ids, th, out, len, &ok);
    if (!ok) throw std::runtime_error("logpost_hessian: the covariance matrix could not be factorised at theta");
  });
}
int mogp_densegp_predict_mixture(mogp_densegp* h, const double* thetas, int S, int len, const double* weights, const double* log_q,
                                 const double* testing, int m, int D, int include_nugget, int max_slots, int max_points, double* mean_out,
                                 double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out) {
  DGUARD(h, {
    Engine* e = h->eng;
    if (D != e->D) throw std::runtime_error("testing points must have D columns");
    if (S >= 1 && len != e->n_theta(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    const GPState& g = e->gp[h->idx];
    if (!(g.has_data && g.factored)) throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
    std::vector<int> ids{h->idx};
    e->predict_mixture(ids, thetas, S, len, weights, log_q, testing, m, include_nugget != 0, max_slots, max_points, mean_out, within_out,
                       between_out, weights_out, logpost_out, ok_out, nullptr);
  });
}
int mogp_densegp_loo_variance(mogp_densegp* h, double* out) { DGUARD(h, h->eng->loo_variance(h->idx, out)); }
int mogp_densegp_get_K(mogp_densegp* h, double* out) { DGUARD(h, h->eng->get_K(h->idx, out)); }
int mogp_densegp_get_invQ(mogp_densegp* h, double* out) { DGUARD(h, h->eng->get_invQ(h->idx, out)); }
int mogp_densegp_get_invQt(mogp_densegp* h, double* out) { DGUARD(h, h->eng->get_invQt(h->idx, out)); }
int mogp_densegp_get_cholesky_lower(mogp_densegp* h, double* out) { DGUARD(h, h->eng->get_chol(h->idx, out)); }
int mogp_densegp_get_pivot(mogp_densegp* h, int* P_out, int* rank_out) { DGUARD(h, h->eng->get_pivot(h->idx, P_out, rank_out)); }
int mogp_pivot_cholesky(const double* A, int n, double* L_out, int* P_out, int* rank_out) {
  GUARD(Engine::pivot_cholesky(A, n, L_out, P_out, rank_out));
}
double mogp_densegp_get_nugget_size(const mogp_densegp* h) { return h->eng->nugget_size(h->idx); }
int mogp_densegp_set_nugget_size(mogp_densegp* h, double v) {
  GPState& g = h->eng->gp[h->idx];
  // a fixed nugget is part of the factored matrix: a new value invalidates the factor, alpha and the log-posterior
  // (the reference keeps serving the stale ones, densegp_gpu.hpp:125-135); the emulator has to be fit again
  if (g.nug_type == NUG_FIXED && v != g.nug_size) g.unfit();
  g.nug_size = v;
  if (g.nug_type == NUG_FIT && !g.data.empty()) g.data[g.data.size() - 1] = v;   // gpparams.hpp:167-172
  return 0;
}
int mogp_densegp_get_nugget_type(const mogp_densegp* h) { return h->eng->gp[h->idx].nug_type; }
int mogp_densegp_set_nugget_type(mogp_densegp* h, int t) {
  DGUARD(h, {
    if (t < 0 || t > 3) throw std::runtime_error("Unrecognized nugget_type");
    GPState& g = h->eng->gp[h->idx];
    if (t != g.nug_type) {
      g.nug_type = t;
      g.data.assign(h->eng->NC + 1 + (t == NUG_FIT ? 1 : 0), 0.);
      g.unfit();
    }
  });
}
int mogp_densegp_get_kernel_type(const mogp_densegp* h) { return h->eng->kernel_type; }
int mogp_fit_single_GP_MAP(mogp_densegp* h, int n_tries, const double* theta0, int theta0_len) {
  DGUARD(h, {
    std::vector<int> ids{h->idx};
    h->eng->fit_map(ids, n_tries, theta0, theta0_len);
  });
}

// ---- MultiOutputGP_GPU ---------------------------------------------------------------------------
static mogp_mogp* mogp_create(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                              const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size, bool analytic,
                              const int* devices, int n_devices);
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

// ---- running the parts of a multi-part handle ------------------------------------------------------
// One mutex per device: the parts that share a device take it for the whole operation, so that two parts never have kernels in
// flight on one device at once (the one-launch Cholesky and the back-substitution chain spin-wait on the device and assume
// they are not co-resident with another such launch).  Never destroyed (threads of other handles may still hold one at exit).
static std::mutex& device_mutex(int device) {
  static std::mutex* reg = new std::mutex();
  static std::map<int, std::unique_ptr<std::mutex>>* mus = new std::map<int, std::unique_ptr<std::mutex>>();
  std::lock_guard<std::mutex> lk(*reg);
  std::unique_ptr<std::mutex>& m = (*mus)[device];
  if (!m) m.reset(new std::mutex());
  return *m;
}
static std::string part_tag(const mogp_part& p) {
  return " [part on device " + std::to_string(p.device) + ", emulators [" + std::to_string(p.lo) + ", " + std::to_string(p.hi) + ")]";
}
// f(part, k) for every part, one host thread per part, each under its device's mutex and a DeviceGuard.  The first failure in part order
// is rethrown on the calling thread once every part has finished, its message naming the part.  A handle with ONE part is the plain
// single-engine model: f runs on the calling thread under a DeviceGuard -- no thread, no mutex, the message as it was thrown.
static void for_parts(mogp_mogp* h, const std::function<void(mogp_part&, int)>& f) {
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
static mogp_part& part_of(mogp_mogp* h, int i) {
  for (auto& p : h->parts)
    if (i >= p.lo && i < p.hi) return p;
  throw std::runtime_error("Invalid emulator index");
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
  GUARD({
    if (index < 0 || index >= (int)h->views.size()) throw std::runtime_error("Invalid emulator index for setting priors");
    set_priors(h->views[index].eng, h->views[index].idx, n_corr, ct, cp, covt, covp, nugt, nugp);
  });
}
int mogp_mogp_eval(mogp_mogp* h, const double* thetas, int n_rows, int n_cols, double* logpost_out, double* grad_out, int* ok_out) {
  GUARD({
    if (n_rows != (int)h->views.size()) throw std::runtime_error("thetas must have one row per emulator");
    for (const auto& v : h->views)
      if (n_cols != v.eng->n_theta(v.idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    for_parts(h, [&](mogp_part& p, int) {
      const int nb = p.hi - p.lo;
      std::vector<int> ids(nb);
      std::vector<const double*> th(nb);
      for (int i = 0; i < nb; ++i) {
        ids[i] = i;
        th[i] = thetas + (size_t)(p.lo + i) * n_cols;
      }
      std::vector<double> f(nb);
      std::vector<int> ok(nb);
      p.eng->eval(ids, th, grad_out != nullptr, f.data(), grad_out ? grad_out + (size_t)p.lo * n_cols : nullptr, n_cols, ok.data());
      if (logpost_out) std::memcpy(logpost_out + p.lo, f.data(), sizeof(double) * nb);
      if (ok_out) std::memcpy(ok_out + p.lo, ok.data(), sizeof(int) * nb);
    });
  });
}
int mogp_mogp_fit(mogp_mogp* h, const double* thetas, int n_rows, int n_cols) {
  GUARD({
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
  GUARD({
    if (index < 0 || index >= (int)h->views.size()) throw std::runtime_error("Invalid emulator index");
    mogp_part& p = part_of(h, index);
    std::unique_lock<std::mutex> lk;      // (parts that share a device take turns; a single part has nobody to wait for)
    if (h->multi()) lk = std::unique_lock<std::mutex>(device_mutex(p.device));
    DeviceGuard g(p.device);
    p.eng->fit_one(index - p.lo, theta, len);
  });
}
static std::vector<int> fitted_ids(const Engine* e) {
  std::vector<int> ids;
  for (int i = 0; i < e->B; ++i)
    if (e->gp[i].has_data && e->gp[i].factored) ids.push_back(i);
  return ids;
}
// The fitted emulators of one engine, computed on compact scratch and scattered to their rows.  out[a] is the caller's array a with one
// row of row[a] doubles per emulator of the engine (null: not asked for); run(ids, buf) fills buf[a] -- (ids.size(), row[a]), null where
// out[a] is -- and row k of it goes to row ids[k] of out[a].  With every emulator fitted, run writes the caller's arrays themselves.
// Rows of unfitted emulators are left untouched, or become NaN with nan_unfitted.
using RowRun = std::function<void(const std::vector<int>&, const std::vector<double*>&)>;
static void with_fitted_rows(Engine* e, const std::vector<double*>& out, const std::vector<size_t>& row, bool nan_unfitted, const RowRun& run) {
  const std::vector<int> ids = fitted_ids(e);
  const size_t nf = ids.size(), na = out.size();
  if ((int)nf == e->B) {
    run(ids, out);
    return;
  }
  if (nan_unfitted)
    for (size_t a = 0; a < na; ++a)
      if (out[a]) std::fill(out[a], out[a] + (size_t)e->B * row[a], std::numeric_limits<double>::quiet_NaN());
  if (nf == 0) return;
  std::vector<std::vector<double>> tmp(na);
  std::vector<double*> buf(na, nullptr);
  for (size_t a = 0; a < na; ++a)
    if (out[a]) {
      tmp[a].resize(nf * row[a]);
      buf[a] = tmp[a].data();
    }
  run(ids, buf);
  for (size_t k = 0; k < nf; ++k)
    for (size_t a = 0; a < na; ++a)
      if (out[a]) std::memcpy(out[a] + (size_t)ids[k] * row[a], buf[a] + k * row[a], row[a] * sizeof(double));
}
// results of fitted emulators go to their own rows; rows of unfitted emulators are untouched (means == null: derivatives only)
static void engine_predict_common(Engine* e, const double* testing, int m, int D, double* means, double* vars, double* derivs) {
  if (D != e->D) throw std::runtime_error("testing points must have D columns");
  with_fitted_rows(e, {means, vars, derivs}, {(size_t)m, (size_t)m, (size_t)m * D}, false, [&](const std::vector<int>& ids, const std::vector<double*>& o) {
    e->predict(ids, testing, m, false, o[0], o[1], m, false, o[2]);
  });
}
// each part writes its own rows of the caller's (n_emulators, ...) arrays
static void mogp_predict_common(mogp_mogp* h, const double* testing, int m, int D, double* means, double* vars, double* derivs) {
  if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
  for_parts(h, [&](mogp_part& p, int) {
    const size_t lo = p.lo;
    engine_predict_common(p.eng.get(), testing, m, D, means ? means + lo * m : nullptr, vars ? vars + lo * m : nullptr,
                          derivs ? derivs + lo * m * D : nullptr);
  });
}
int mogp_mogp_predict_batch(mogp_mogp* h, const double* testing, int m, int D, double* means) {
  GUARD(mogp_predict_common(h, testing, m, D, means, nullptr, nullptr));
}
int mogp_mogp_predict_variance_batch(mogp_mogp* h, const double* testing, int m, int D, double* means, double* vars) {
  GUARD(mogp_predict_common(h, testing, m, D, means, vars, nullptr));
}
int mogp_mogp_predict_deriv(mogp_mogp* h, const double* testing, int m, int D, double* derivs) {
  GUARD(mogp_predict_common(h, testing, m, D, nullptr, nullptr, derivs));
}
static void engine_predict_full_cov(Engine* e, const double* testing, int m, int D, double* means, double* covs) {
  if (D != e->D) throw std::runtime_error("testing points must have D columns");
  with_fitted_rows(e, {means, covs}, {(size_t)m, (size_t)m * m}, false, [&](const std::vector<int>& ids, const std::vector<double*>& o) {
    e->predict_full_cov(ids, testing, m, o[0], o[1]);
  });
}
int mogp_mogp_predict_full_cov(mogp_mogp* h, const double* testing, int m, int D, double* means, double* covs) {
  GUARD({
    if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
    for_parts(h, [&](mogp_part& p, int) {
      const size_t lo = p.lo;
      engine_predict_full_cov(p.eng.get(), testing, m, D, means + lo * m, covs + lo * (size_t)m * m);
    });
  });
}
// Several parts: every part writes the (rank+1) largest implausibilities of its own emulators per query point into one block of a
// device buffer on part 0's device (implausibility_top); implausibility_merge_kernel reduces them there.  The query points go in outer
// chunks of at most 2^18, so that the lists of one chunk stay small next to the engines' own scratch.
static void mogp_implausibility_parts(mogp_mogp* h, const double* testing, int m, const double* obs, const double* obs_var,
                                      const double* discrepancy, bool include_nugget, int rank, double* out) {
  const int B = (int)h->views.size();
  if (B == 1) rank = 0;                                       // HistoryMatching.py:254-255
  if (rank < 0) throw std::runtime_error("rank must be a non-negative integer");
  if (rank >= B) throw std::runtime_error("rank must be less than the number of observations");
  if (rank > IMPLAUS_MAX_RANK) throw std::runtime_error("rank above " + std::to_string(IMPLAUS_MAX_RANK) + " is not supported on the device");
  if (m <= 0) return;
  const int np = (int)h->parts.size(), keep = rank + 1, dev0 = h->parts[0].device;
  const long OC = std::min<long>(m, 1L << 18);
  // the two buffers live on part 0's device: the calling thread stays on it for the whole function (the threads of for_parts set their own)
  DeviceGuard g(dev0);
  DevBuf<double> dLists((size_t)np * keep * OC), dOut((size_t)OC);
  for (long c0 = 0; c0 < m; c0 += OC) {
    const int mc = (int)std::min<long>(OC, m - c0);
    for_parts(h, [&](mogp_part& p, int k) {
      std::vector<int> ids(p.hi - p.lo);
      for (int i = 0; i < (int)ids.size(); ++i) ids[i] = i;
      p.eng->implausibility_top(ids, testing + (size_t)c0 * h->eng->D, mc, obs + p.lo, obs_var + p.lo, discrepancy + p.lo, include_nugget,
                                keep, dLists + (size_t)k * keep * OC, OC, dev0);
    });
    mogp_part& p0 = h->parts[0];
    std::lock_guard<std::mutex> lk(device_mutex(dev0));
    launch_implausibility_merge(np, dLists, OC, mc, rank, dOut, p0.eng->stream);
    hip_check(hipMemcpyAsync(out + c0, dOut, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, p0.eng->stream), "hipMemcpyAsync");
    hip_check(hipStreamSynchronize(p0.eng->stream), "hipStreamSynchronize");
  }
  hip_check(hipGetLastError(), "implausibility_merge_kernel");
}
int mogp_mogp_implausibility(mogp_mogp* h, const double* testing, int m, int D, const double* obs, const double* obs_var,
                             const double* discrepancy, int include_nugget, int rank, double* out) {
  GUARD({
    if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
    for (const auto& v : h->views)
      if (!(v.eng->gp[v.idx].has_data && v.eng->gp[v.idx].factored))
        throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
    if (!h->multi()) {
      Engine* e = h->eng;
      DeviceGuard g(e->device_id());
      std::vector<int> ids = fitted_ids(e);
      e->implausibility(ids, testing, m, obs, obs_var, discrepancy, include_nugget != 0, rank, out);
      return 0;
    }
    mogp_implausibility_parts(h, testing, m, obs, obs_var, discrepancy, include_nugget != 0, rank, out);
  });
}
// the fitted emulators of one engine into their own rows of the caller's arrays; rows of unfitted emulators become NaN
static void engine_sobol(Engine* e, const double* A, const double* B, int N, bool unc, bool include_nugget, double* S, double* ST,
                         double* mean_out, double* variance_out, double* emvar_out) {
  const size_t D = e->D;
  with_fitted_rows(e, {S, ST, mean_out, variance_out, emvar_out}, {D, D, 1, 1, 1}, true, [&](const std::vector<int>& ids, const std::vector<double*>& o) {
    e->sobol(ids, A, B, N, unc, include_nugget, o[0], o[1], o[2], o[3], o[4]);
  });
}
// Emulators are independent: every part runs its own block on its own engine and writes its own rows (no cross-device reduction)
int mogp_mogp_sobol(mogp_mogp* h, const double* A, const double* B, int N, int D, int unc, int include_nugget, double* S, double* ST,
                    double* mean_out, double* variance_out, double* emulator_variance_out) {
  GUARD({
    if (D != h->eng->D) throw std::runtime_error("sobol: the sample matrices must have D columns");
    if (!S || !ST || !mean_out || !variance_out) throw std::runtime_error("sobol: null result buffer");
    if (unc && !emulator_variance_out) throw std::runtime_error("sobol: unc needs a buffer for the emulator variance");
    double* ev = unc ? emulator_variance_out : nullptr;
    for_parts(h, [&](mogp_part& p, int) {
      const size_t lo = p.lo;
      engine_sobol(p.eng.get(), A, B, N, unc != 0, include_nugget != 0, S + lo * D, ST + lo * D, mean_out + lo, variance_out + lo,
                   ev ? ev + lo : nullptr);
    });
  });
}
// every part: its fitted emulators in one Engine::predict_mixture, the rows of the others NaN
int mogp_mogp_predict_mixture(mogp_mogp* h, const double* thetas, int S, int n_cols, const double* weights, const double* log_q,
                              const double* testing, int m, int D, int include_nugget, int max_slots, int max_points, double* mean_out,
                              double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out,
                              int* ok_all_out) {
  GUARD({
    if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
    if (S < 1) throw std::runtime_error("predict_mixture: at least one sample per emulator is needed (S = " + std::to_string(S) + ")");
    if (!thetas || !mean_out || !within_out || !between_out || !weights_out || !logpost_out || !ok_out)
      throw std::runtime_error("predict_mixture: null buffer");
    if ((weights != nullptr) == (log_q != nullptr)) throw std::runtime_error("predict_mixture: exactly one of weights and log_q must be given");
    int widest = 0;
    for (const auto& v : h->views) widest = std::max(widest, v.eng->n_theta(v.idx));
    if (n_cols != widest) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    const size_t mm = (size_t)std::max(m, 0);
    const size_t SS = (size_t)S;
    for_parts(h, [&](mogp_part& p, int) {
      Engine* e = p.eng.get();
      const std::vector<int> ids = fitted_ids(e);
      const size_t nf = ids.size(), lo = (size_t)p.lo;
      const double nan = std::numeric_limits<double>::quiet_NaN();
      if ((int)nf == e->B) {
        e->predict_mixture(ids, thetas + lo * SS * n_cols, S, n_cols, weights ? weights + lo * SS : nullptr, log_q ? log_q + lo * SS : nullptr,
                           testing, m, include_nugget != 0, max_slots, max_points, mean_out + lo * mm, within_out + lo * mm,
                           between_out + lo * mm, weights_out + lo * SS, logpost_out + lo * SS, ok_out + lo * SS,
                           ok_all_out ? ok_all_out + lo : nullptr);
        return;
      }
      for (int i = 0; i < e->B; ++i) {
        const size_t r = lo + i;
        std::fill(mean_out + r * mm, mean_out + (r + 1) * mm, nan);
        std::fill(within_out + r * mm, within_out + (r + 1) * mm, nan);
        std::fill(between_out + r * mm, between_out + (r + 1) * mm, nan);
        std::fill(weights_out + r * SS, weights_out + (r + 1) * SS, nan);
        std::fill(logpost_out + r * SS, logpost_out + (r + 1) * SS, nan);
        std::fill(ok_out + r * SS, ok_out + (r + 1) * SS, 0);
        if (ok_all_out) ok_all_out[r] = 0;
      }
      if (nf == 0) return;
      // the fitted emulators, compact
      std::vector<double> th(nf * SS * n_cols), wq(nf * SS), mu(nf * mm), wi(nf * mm), be(nf * mm), wo(nf * SS), lp(nf * SS);
      std::vector<int> ok(nf * SS), oka(nf);
      const double* src = weights ? weights : log_q;
      for (size_t k = 0; k < nf; ++k) {
        const size_t r = lo + ids[k];
        std::memcpy(th.data() + k * SS * n_cols, thetas + r * SS * n_cols, SS * n_cols * sizeof(double));
        std::memcpy(wq.data() + k * SS, src + r * SS, SS * sizeof(double));
      }
      e->predict_mixture(ids, th.data(), S, n_cols, weights ? wq.data() : nullptr, log_q ? wq.data() : nullptr, testing, m, include_nugget != 0,
                         max_slots, max_points, mu.data(), wi.data(), be.data(), wo.data(), lp.data(), ok.data(), oka.data());
      for (size_t k = 0; k < nf; ++k) {
        const size_t r = lo + ids[k];
        std::memcpy(mean_out + r * mm, mu.data() + k * mm, mm * sizeof(double));
        std::memcpy(within_out + r * mm, wi.data() + k * mm, mm * sizeof(double));
        std::memcpy(between_out + r * mm, be.data() + k * mm, mm * sizeof(double));
        std::memcpy(weights_out + r * SS, wo.data() + k * SS, SS * sizeof(double));
        std::memcpy(logpost_out + r * SS, lp.data() + k * SS, SS * sizeof(double));
        std::memcpy(ok_out + r * SS, ok.data() + k * SS, SS * sizeof(int));
        if (ok_all_out) ok_all_out[r] = oka[k];
      }
    });
  });
}
int mogp_mogp_hessian(mogp_mogp* h, const double* thetas, int n_rows, int n_cols, double* hess_out, int* ok_out) {
  GUARD({
    if (n_rows != (int)h->views.size()) throw std::runtime_error("thetas must have one row per emulator");
    if (!thetas || !hess_out) throw std::runtime_error("logpost_hessian: null buffer");
    int widest = 0;
    for (const auto& v : h->views) widest = std::max(widest, v.eng->n_theta(v.idx));
    if (n_cols != widest) throw std::runtime_error("Shape of new GPParams object does not match existing one");
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
// device-resident prediction: d_means / d_vars (n_emulators, m) and d_derivs (n_emulators, m, D) are device buffers (d_vars, d_derivs may be
// null); rows of emulators that are not fit are filled with NaN (MultiOutputGP_GPU.py:288-296)
#define HIPCK(x) hip_check((x), #x)
static void engine_predict_dev(Engine* e, const double* d_testing, int m, int D, double* d_means, double* d_vars, double* d_derivs) {
  std::vector<int> ids = fitted_ids(e);
  if ((int)ids.size() == e->B) {
    e->predict(ids, d_testing, m, true, d_means, d_vars, m, true, d_derivs);
    return;
  }
  // some emulators are not fit: the fitted ones are predicted into scratch rows and copied to their places, the others become NaN (the
  // all-ones bit pattern is a quiet NaN: a memset on the engine's stream instead of one blocking host copy per row and array)
  const size_t nf = ids.size(), row = (size_t)m, drow = (size_t)m * D;
  hipStream_t st = e->stream;
  std::vector<char> fitted(e->B, 0);
  for (int i : ids) fitted[i] = 1;
  for (int i = 0; i < e->B; ++i) {
    if (fitted[i]) continue;
    if (d_means) HIPCK(hipMemsetAsync(d_means + (size_t)i * row, 0xFF, row * sizeof(double), st));
    if (d_vars) HIPCK(hipMemsetAsync(d_vars + (size_t)i * row, 0xFF, row * sizeof(double), st));
    if (d_derivs) HIPCK(hipMemsetAsync(d_derivs + (size_t)i * drow, 0xFF, drow * sizeof(double), st));
  }
  if (nf == 0) {
    HIPCK(hipStreamSynchronize(st));
    return;
  }
  DevBuf<double> tm, tv, td;
  SyncOnUnwind drained{st};
  if (d_means) tm.reserve(nf * row);
  if (d_vars) tv.reserve(nf * row);
  if (d_derivs) td.reserve(nf * drow);
  e->predict(ids, d_testing, m, true, tm, tv, m, true, td);
  // runs of consecutive fitted emulators go in one copy each
  for (size_t k = 0; k < nf;) {
    size_t len = 1;
    while (k + len < nf && ids[k + len] == ids[k] + (int)len) ++len;
    if (d_means) HIPCK(hipMemcpyAsync(d_means + (size_t)ids[k] * row, tm + k * row, len * row * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (d_vars) HIPCK(hipMemcpyAsync(d_vars + (size_t)ids[k] * row, tv + k * row, len * row * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (d_derivs) HIPCK(hipMemcpyAsync(d_derivs + (size_t)ids[k] * drow, td + k * drow, len * drow * sizeof(double), hipMemcpyDeviceToDevice, st));
    k += len;
  }
  HIPCK(hipStreamSynchronize(st));
}
// Several parts: a part on the device of the caller's buffers predicts straight into its rows; a part on another device copies the test points
// to its own device, predicts into scratch there and copies its rows back with peer copies on its stream.
static void mogp_predict_dev_parts(mogp_mogp* h, const double* d_testing, int m, int D, double* d_means, double* d_vars, double* d_derivs) {
  int caller = -1;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, d_testing) == hipSuccess && attr.device >= 0) caller = attr.device;
  else HIPCK(hipGetDevice(&caller));
  for_parts(h, [&](mogp_part& p, int) {
    Engine* e = p.eng.get();
    const size_t rows = p.hi - p.lo, lo = p.lo, row = (size_t)m, drow = (size_t)m * D;
    double* om = d_means ? d_means + lo * row : nullptr;
    double* ov = d_vars ? d_vars + lo * row : nullptr;
    double* od = d_derivs ? d_derivs + lo * drow : nullptr;
    if (p.device == caller) {
      engine_predict_dev(e, d_testing, m, D, om, ov, od);
      return;
    }
    hipStream_t st = e->stream;
    DevBuf<double> xs(drow), tm, tv, td;
    SyncOnUnwind drained{st};
    if (om) tm.reserve(rows * row);
    if (ov) tv.reserve(rows * row);
    if (od) td.reserve(rows * drow);
    HIPCK(hipMemcpyPeerAsync(xs, p.device, d_testing, caller, drow * sizeof(double), st));
    engine_predict_dev(e, xs, m, D, tm, tv, td);
    if (om) HIPCK(hipMemcpyPeerAsync(om, caller, tm, p.device, rows * row * sizeof(double), st));
    if (ov) HIPCK(hipMemcpyPeerAsync(ov, caller, tv, p.device, rows * row * sizeof(double), st));
    if (od) HIPCK(hipMemcpyPeerAsync(od, caller, td, p.device, rows * drow * sizeof(double), st));
    HIPCK(hipStreamSynchronize(st));
  });
}
static void mogp_predict_dev_common(mogp_mogp* h, const double* d_testing, int m, int D, double* d_means, double* d_vars, double* d_derivs) {
  if (D != h->eng->D) throw std::runtime_error("testing points must have D columns");
  if (m <= 0) return;
  // the same contract whatever the fit status is: the test points are required, any of the three outputs may be null
  // (Engine::predict: means == nullptr = derivatives only), but not all of them
  if (!d_testing) throw std::runtime_error("device-resident predict: the test points pointer is null");
  if (!d_means && !d_vars && !d_derivs) throw std::runtime_error("device-resident predict: no output buffer given");
  if (!h->multi()) {
    DeviceGuard g(h->eng->device_id());
    engine_predict_dev(h->eng, d_testing, m, D, d_means, d_vars, d_derivs);
    return;
  }
  mogp_predict_dev_parts(h, d_testing, m, D, d_means, d_vars, d_derivs);
}
#undef HIPCK
int mogp_mogp_predict_variance_batch_dev(mogp_mogp* h, const double* d_testing, int m, int D, double* d_means, double* d_vars) {
  GUARD(mogp_predict_dev_common(h, d_testing, m, D, d_means, d_vars, nullptr));
}
int mogp_mogp_predict_dev(mogp_mogp* h, const double* d_testing, int m, int D, double* d_means, double* d_vars, double* d_derivs) {
  GUARD(mogp_predict_dev_common(h, d_testing, m, D, d_means, d_vars, d_derivs));
}
using EmuRef = std::pair<const Engine*, int>;      // (a comma inside GUARD's argument would split it)
int mogp_fit_GP_MAP(mogp_mogp* h, int n_tries, const double* theta0, int theta0_len) {
  GUARD({
    // every starting point is drawn here, in the order of the unsharded model (start-major), from part 0's rng -- seeded as a single
    // engine's is -- with each emulator's own priors; each part then runs its block.  The end point of a run does not depend on the
    // batch it ran in (Engine::run_pool), so the result is the single-engine one whatever the split.  With one part this is
    // Engine::fit_map: the same checks in the same order, the same draws from the same generator.
    if (n_tries < 1) throw std::runtime_error("number of attempts must be positive");
    std::vector<EmuRef> emus;
    for (const auto& v : h->views) {
      if (theta0_len > 0 && theta0_len != v.eng->n_theta(v.idx)) throw std::runtime_error("length of theta0 must equal n_params of GP.");
      emus.emplace_back(v.eng, v.idx);
    }
    const Engine::Starts x0 = Engine::draw_starts(h->eng->random(), emus, n_tries, theta0, theta0_len);
    for_parts(h, [&](mogp_part& p, int) {
      const int nb = p.hi - p.lo;
      std::vector<int> ids(nb);
      for (int i = 0; i < nb; ++i) ids[i] = i;
      Engine::Starts sub(n_tries, std::vector<std::vector<double>>(nb));
      for (int s = 0; s < n_tries; ++s)
        for (int i = 0; i < nb; ++i) sub[s][i] = x0[s][p.lo + i];
      p.eng->fit_map_from(ids, sub);
    });
  });
}
int mogp_set_fit_options(int max_iter, double ftol, double gtol, unsigned long long seed) {
  FitOptions& o = fit_options();
  if (max_iter > 0) o.max_iter = max_iter;
  if (ftol > 0) o.ftol = ftol;
  if (gtol > 0) o.gtol = gtol;
  o.seed = seed;
  return 0;
}

// ---- stand-alone kernel objects (bindings.cu:340-361, kernel.hpp:47-107) --------------------------------------
// kernel_type as in the enum (0 SqExp, 1 Matern52, 2 ProductMat52, 3 UniformSqExp, 4 UniformMat52); params = [corr_raw.., log sigma^2]
// (n_corr + 1 entries, n_corr = 1 for the uniform kernels); what = 0 kernel_f -> out (n1, n2), 1 kernel_deriv -> out
// (n_corr + 1, n1, n2), 2 kernel_inputderiv -> out (n2, n1, D) (the reference's flat order)
int mogp_kernel_eval(int kernel_type, int what, const double* x1, int n1, const double* x2, int n2, int D, const double* params, int n_params,
                     double* out) {
  GUARD(kernel_eval_impl(kernel_type, what, x1, n1, x2, n2, D, params, n_params, out));
}

int mogp_gkdr_R(const double* X, int n, int m, const double* y, int nx, const double* sgx2, int ny, const double* sgy2, double eps,
                int max_pairs_per_pass, double* R_out, int* info_out) {
  GUARD(gkdr_R(X, n, m, y, nx, sgx2, ny, sgy2, eps, max_pairs_per_pass, R_out, info_out));
}

int mogp_design_min_pdist(const double* designs, int T, int n, int D, double* out) {
  GUARD(design_min_pdist(designs, T, n, D, out));
}

// ---- measurement hooks ----------------------------------------------------------------------------
int mogp_profile_enable(int on) { prof_enable(on != 0); return 0; }
int mogp_profile_reset(void) { prof_reset(); return 0; }
int mogp_profile_schedule(int schedule, int single_stream) {
  schedule_override().schedule = schedule;
  schedule_override().single_stream = single_stream != 0;
  return 0;
}
static int task_table_out(int n_plus_rhs, bool ahead, int* out, int capacity) {
  // host-only: the per-emulator task order of the one-launch Cholesky for a matrix of NP = roundup(n_plus_rhs, 128) rows
  const int NP = (n_plus_rhs + TILE - 1) / TILE * TILE;
  const std::vector<int> tb = mchol_task_table(NP, ahead);
  if (out)
    for (int i = 0; i < (int)tb.size() && i < capacity; ++i) out[i] = tb[i];
  return (int)tb.size();
}
int mogp_mchol_task_table(int n_plus_rhs, int* out, int capacity) { return task_table_out(n_plus_rhs, false, out, capacity); }
int mogp_mchol_task_table_ahead(int n_plus_rhs, int* out, int capacity) { return task_table_out(n_plus_rhs, true, out, capacity); }
int mogp_profile_counter(const char* name, long long* out) {
  const long long v = prof_counter(name);
  if (v < 0 || !out) {
    g_err = std::string("unknown counter ") + (name ? name : "(null)");
    return 1;
  }
  *out = v;
  return 0;
}
int mogp_profile_get(const char* tag, double* total_ms, long long* launches, double* alg_flops, double* alg_bytes) {
  return prof_get(tag, total_ms, launches, alg_flops, alg_bytes) ? 0 : 1;
}
void* mogp_dev_malloc(unsigned long long bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { g_err = "hipMalloc failed"; return nullptr; }
  return p;
}
int mogp_dev_free(void* p) { GUARD(hip_check(hipFree(p), "hipFree")); }
int mogp_dev_upload(void* d, const void* s, unsigned long long bytes) { GUARD(hip_check(hipMemcpy(d, s, bytes, hipMemcpyHostToDevice), "upload")); }
int mogp_dev_download(void* d, const void* s, unsigned long long bytes) { GUARD(hip_check(hipMemcpy(d, s, bytes, hipMemcpyDeviceToHost), "download")); }
int mogp_dev_synchronize(void) { GUARD(hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize")); }

}  // extern "C"
