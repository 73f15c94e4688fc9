// DenseGP_GPU: one emulator, an engine of its own or a borrowed view into a MultiOutputGP_GPU's (capi_internal.h)
#include "analysis.h"
#include "capi_internal.h"

using namespace mogp;
using namespace mogp::capi;

void mogp::capi::set_priors(Engine* eng, int i, int n_corr, const int* ct, const double* cp, int covt, const double* covp, int nugt,
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
void mogp::capi::check_sobol_args(int D, const Engine* e, const double* S, const double* ST, const double* mean_out, const double* variance_out,
                                  int unc, const double* emulator_variance_out) {
  check_D(D, e, "sobol: the sample matrices must have D columns");
  if (!S || !ST || !mean_out || !variance_out) throw std::runtime_error("sobol: null result buffer");
  if (unc && !emulator_variance_out) throw std::runtime_error("sobol: unc needs a buffer for the emulator variance");
}

extern "C" {

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
  return on_engine_device(h, [&] { h->eng->set_mean_priors(h->idx, q, b, Binv, Binv_b, logdetB); });
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
  return on_engine_device(h, [&] { set_priors(h->eng, h->idx, n_corr, ct, cp, covt, covp, nugt, nugp); });
}
int mogp_densegp_priors_logp(const mogp_densegp* h, const double* th, int len, double* out) {
  return on_engine_device(h, [&] {
    if (len != h->eng->n_data(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    std::vector<double> v(th, th + len);
    *out = h->eng->gp[h->idx].pri.logp(v, h->eng->NC, h->eng->gp[h->idx].nug_type);
  });
}
int mogp_densegp_priors_dlogpdtheta(const mogp_densegp* h, const double* th, int len, double* out) {
  return on_engine_device(h, [&] {
    if (len != h->eng->n_data(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    std::vector<double> v(th, th + len);
    h->eng->gp[h->idx].pri.dlogpdtheta(v, h->eng->NC, h->eng->gp[h->idx].nug_type, out);
  });
}
int mogp_densegp_priors_sample(mogp_densegp* h, double* out) {
  return on_engine_device(h, [&] {
    static std::mt19937_64 r(std::random_device{}());
    const int nm = h->eng->n_mean();
    for (int k = 0; k < nm; ++k) out[k] = 0.;
    h->eng->gp[h->idx].pri.sample(r, h->eng->NC, h->eng->gp[h->idx].nug_type, out + nm);
  });
}
int mogp_densegp_fit(mogp_densegp* h, const double* theta, int len) { return on_engine_device(h, [&] { h->eng->fit_one(h->idx, theta, len); }); }
int mogp_densegp_get_logpost(mogp_densegp* h, const double* theta, int len, double* out) {
  return on_engine_device(h, [&] {
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
  return on_engine_device(h, [&] {
    Engine* e = h->eng;
    if (len < e->n_theta(h->idx)) throw std::runtime_error("logpost_deriv: the result buffer passed was too small");
    if (!e->gp[h->idx].factored) throw std::runtime_error("logpost_deriv: hyperparameters have not been fit");
    e->grad_current({h->idx}, out, len);
  });
}
static void check_batch(const mogp_densegp* h, int m, int D, int out_len, const char* small_msg) {
  check_D(D, h->eng);
  if (out_len < m) throw std::runtime_error(small_msg);
  if ((unsigned)m > h->eng->testing_size)
    throw std::runtime_error("predict_variance_batch: More test points were passed than the maximum batch size");
}
int mogp_densegp_predict(mogp_densegp* h, const double* testing, int D, double* mean_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng, "testing point must have D entries");
    h->eng->predict({h->idx}, testing, 1, false, mean_out, nullptr, 1, false, nullptr);
  });
}
int mogp_densegp_predict_variance(mogp_densegp* h, const double* testing, int D, double* mean_out, double* var_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng, "testing point must have D entries");
    h->eng->predict({h->idx}, testing, 1, false, mean_out, var_out, 1, false, nullptr);
  });
}
int mogp_densegp_predict_batch(mogp_densegp* h, const double* testing, int m, int D, double* mean_out, int out_len) {
  return on_engine_device(h, [&] {
    check_batch(h, m, D, out_len, "predict_batch: the result buffer passed was too small to hold the result");
    h->eng->predict({h->idx}, testing, m, false, mean_out, nullptr, m, false, nullptr);
  });
}
int mogp_densegp_predict_variance_batch(mogp_densegp* h, const double* testing, int m, int D, double* mean_out, double* var_out, int out_len) {
  return on_engine_device(h, [&] {
    check_batch(h, m, D, out_len, "predict_variance_batch: The result buffer passed was too small to hold the variance");
    h->eng->predict({h->idx}, testing, m, false, mean_out, var_out, m, false, nullptr);
  });
}
int mogp_densegp_predict_deriv(mogp_densegp* h, const double* testing, int m, int D, double* out, int out_rows, int out_cols) {
  return on_engine_device(h, [&] {
    if (out_rows < m || out_cols != h->eng->D)
      throw std::runtime_error("predict_deriv: the result buffer passed was the wrong shape to hold the result");
    check_batch(h, m, D, m, "");
    h->eng->predict({h->idx}, testing, m, false, nullptr, nullptr, m, false, out);        // derivatives only: no cross covariance
  });
}
int mogp_densegp_predict_full_cov(mogp_densegp* h, const double* testing, int m, int D, double* mean_out, double* cov_out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng);
    h->eng->predict_full_cov({h->idx}, testing, m, mean_out, cov_out);
  });
}
int mogp_densegp_implausibility(mogp_densegp* h, const double* testing, int m, int D, double obs, double obs_var, double discrepancy,
                                int include_nugget, double* out) {
  return on_engine_device(h, [&] {
    check_D(D, h->eng);
    h->eng->implausibility({h->idx}, testing, m, &obs, &obs_var, &discrepancy, include_nugget != 0, 0, out);
  });
}
int mogp_densegp_sobol(mogp_densegp* h, const double* A, const double* B, int N, int D, int unc, int include_nugget, double* S, double* ST,
                       double* mean_out, double* variance_out, double* emulator_variance_out) {
  return on_engine_device(h, [&] {
    check_sobol_args(D, h->eng, S, ST, mean_out, variance_out, unc, emulator_variance_out);
    h->eng->sobol({h->idx}, A, B, N, unc != 0, include_nugget != 0, S, ST, mean_out, variance_out, unc ? emulator_variance_out : nullptr);
  });
}
int mogp_densegp_logpost_hessian(mogp_densegp* h, const double* theta, int len, double* out) {
  return on_engine_device(h, [&] {
    Engine* e = h->eng;
    if (len != e->n_theta(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    if (!theta || !out) throw std::runtime_error("logpost_hessian: null buffer");
    std::vector<const double*> th{theta};
    int ok = 0;
    e->hessian({h->idx}, th, out, len, &ok);
    if (!ok) throw std::runtime_error("logpost_hessian: the covariance matrix could not be factorised at theta");
  });
}
int mogp_densegp_predict_mixture(mogp_densegp* h, const double* thetas, int S, int len, const double* weights, const double* log_q,
                                 const double* testing, int m, int D, int include_nugget, int max_slots, int max_points, double* mean_out,
                                 double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out) {
  return on_engine_device(h, [&] {
    Engine* e = h->eng;
    check_D(D, e);
    if (S >= 1 && len != e->n_theta(h->idx)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    const GPState& g = e->gp[h->idx];
    if (!(g.has_data && g.factored)) throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
    predict_mixture(*e, {h->idx}, thetas, S, len, weights, log_q, testing, m, include_nugget != 0, max_slots, max_points, mean_out, within_out,
                       between_out, weights_out, logpost_out, ok_out, nullptr);
  });
}
int mogp_densegp_cross_validate(mogp_densegp* h, const int* labels, int n_labels, int k, int include_nugget, int max_slots, double* mean_out,
                                double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  return on_engine_device(h, [&] {
    Engine* e = h->eng;
    const GPState& g = e->gp[h->idx];
    if (!(g.has_data && g.factored)) throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
    if (n_labels != e->n) throw std::runtime_error("cross_validate: one fold label per training point is needed");
    cross_validate(*e, {h->idx}, labels, k, include_nugget != 0, max_slots, mean_out, var_out, maha_out, log_score_out, ok_out);
  });
}
int mogp_densegp_sample_posterior(mogp_densegp* h, const double* testing, int m, int D, int S, unsigned long long seed, unsigned int stream0,
                                  const double* z_in, int z_in_per_emulator, int include_nugget, double jitter, int max_slots, int max_draws,
                                  double* samples_out, double* mean_out, double* z_out, double* jitter_used_out, int* ok_out) {
  return on_engine_device(h, [&] {
    Engine* e = h->eng;
    check_D(D, e);
    const GPState& g = e->gp[h->idx];
    if (!(g.has_data && g.factored)) throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
    (void)z_in_per_emulator;      // one emulator: (S, m) either way
    sample_posterior(*e, {h->idx}, &stream0, testing, m, S, seed, z_in, false, include_nugget != 0, jitter, max_slots, max_draws, samples_out,
                        mean_out, z_out, jitter_used_out, ok_out);
  });
}
int mogp_densegp_loo_variance(mogp_densegp* h, double* out) { return on_engine_device(h, [&] { h->eng->loo_variance(h->idx, out); }); }
int mogp_densegp_get_K(mogp_densegp* h, double* out) { return on_engine_device(h, [&] { h->eng->get_K(h->idx, out); }); }
int mogp_densegp_get_invQ(mogp_densegp* h, double* out) { return on_engine_device(h, [&] { h->eng->get_invQ(h->idx, out); }); }
int mogp_densegp_get_invQt(mogp_densegp* h, double* out) { return on_engine_device(h, [&] { h->eng->get_invQt(h->idx, out); }); }
int mogp_densegp_get_cholesky_lower(mogp_densegp* h, double* out) { return on_engine_device(h, [&] { h->eng->get_chol(h->idx, out); }); }
int mogp_densegp_get_pivot(mogp_densegp* h, int* P_out, int* rank_out) { return on_engine_device(h, [&] { h->eng->get_pivot(h->idx, P_out, rank_out); }); }
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
  return on_engine_device(h, [&] {
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
  return on_engine_device(h, [&] {
    h->eng->fit_map({h->idx}, n_tries, theta0, theta0_len);
  });
}

}  // extern "C"
