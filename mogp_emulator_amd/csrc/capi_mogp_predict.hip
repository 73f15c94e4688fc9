// MultiOutputGP_GPU: the prediction family -- host predict, full covariance, Sobol indices, the mixture over hyperparameter samples,
// implausibility with its cross-part merge, and the device-resident predict
#include "analysis.h"
#include "capi_internal.h"

using namespace mogp;
using namespace mogp::capi;

// The fitted emulators of one engine on compact rows, scattered to their rows of the caller's arrays (with_rows of fitted_rows.h):
// run(ids, a) computes the emulators ids into a.  With every emulator fitted, run writes the caller's arrays themselves.
using RowRun = std::function<void(const std::vector<int>&, const std::vector<Rows>&)>;
static void with_fitted_rows(Engine* e, const std::vector<Rows>& arrays, const RowRun& run) {
  const std::vector<int> ids = fitted_ids(e);
  with_rows(e->B, ids, arrays, [&](const std::vector<Rows>& a) { run(ids, a); });
}
// results of fitted emulators go to their own rows; rows of unfitted emulators are untouched (means == null: derivatives only)
static void engine_predict_common(Engine* e, const double* testing, int m, int D, double* means, double* vars, double* derivs) {
  check_D(D, e);
  const size_t mm = m;
  with_fitted_rows(e, {Rows::out(means, mm, false), Rows::out(vars, mm, false), Rows::out(derivs, mm * D, false)},
                   [&](const std::vector<int>& ids, const std::vector<Rows>& o) {
                     e->predict(ids, testing, m, false, o[0].d(), o[1].d(), m, false, o[2].d());
                   });
}
// each part writes its own rows of the caller's (n_emulators, ...) arrays
static void mogp_predict_common(mogp_mogp* h, const double* testing, int m, int D, double* means, double* vars, double* derivs) {
  check_D(D, h->eng);
  for_parts(h, [&](mogp_part& p, int) {
    const size_t lo = p.lo;
    engine_predict_common(p.eng.get(), testing, m, D, means ? means + lo * m : nullptr, vars ? vars + lo * m : nullptr,
                          derivs ? derivs + lo * m * D : nullptr);
  });
}
static void engine_predict_full_cov(Engine* e, const double* testing, int m, int D, double* means, double* covs) {
  check_D(D, e);
  with_fitted_rows(e, {Rows::out(means, (size_t)m, false), Rows::out(covs, (size_t)m * m, false)},
                   [&](const std::vector<int>& ids, const std::vector<Rows>& o) { e->predict_full_cov(ids, testing, m, o[0].d(), o[1].d()); });
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
      p.eng->implausibility_top(all_ids(p.hi - p.lo), testing + (size_t)c0 * h->eng->D, mc, obs + p.lo, obs_var + p.lo, discrepancy + p.lo, include_nugget,
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
// the fitted emulators of one engine into their own rows of the caller's arrays; rows of unfitted emulators become NaN
static void engine_sobol(Engine* e, const double* A, const double* B, int N, bool unc, bool include_nugget, double* S, double* ST,
                         double* mean_out, double* variance_out, double* emvar_out) {
  const size_t D = e->D;
  with_fitted_rows(e, {Rows::out(S, D, true), Rows::out(ST, D, true), Rows::out(mean_out, 1, true), Rows::out(variance_out, 1, true), Rows::out(emvar_out, 1, true)},
                   [&](const std::vector<int>& ids, const std::vector<Rows>& o) {
                     e->sobol(ids, A, B, N, unc, include_nugget, o[0].d(), o[1].d(), o[2].d(), o[3].d(), o[4].d());
                   });
}
// device-resident prediction: d_means / d_vars (n_emulators, m) and d_derivs (n_emulators, m, D) are device buffers (d_vars, d_derivs may be
// null); rows of emulators that are not fit are filled with NaN (MultiOutputGP_GPU.py:288-296)
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
  check_D(D, h->eng);
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

extern "C" {

int mogp_mogp_predict_batch(mogp_mogp* h, const double* testing, int m, int D, double* means) {
  return guarded([&] { mogp_predict_common(h, testing, m, D, means, nullptr, nullptr); });
}
int mogp_mogp_predict_variance_batch(mogp_mogp* h, const double* testing, int m, int D, double* means, double* vars) {
  return guarded([&] { mogp_predict_common(h, testing, m, D, means, vars, nullptr); });
}
int mogp_mogp_predict_deriv(mogp_mogp* h, const double* testing, int m, int D, double* derivs) {
  return guarded([&] { mogp_predict_common(h, testing, m, D, nullptr, nullptr, derivs); });
}
int mogp_mogp_predict_full_cov(mogp_mogp* h, const double* testing, int m, int D, double* means, double* covs) {
  return guarded([&] {
    check_D(D, h->eng);
    for_parts(h, [&](mogp_part& p, int) {
      const size_t lo = p.lo;
      engine_predict_full_cov(p.eng.get(), testing, m, D, means + lo * m, covs + lo * (size_t)m * m);
    });
  });
}
int mogp_mogp_implausibility(mogp_mogp* h, const double* testing, int m, int D, const double* obs, const double* obs_var,
                             const double* discrepancy, int include_nugget, int rank, double* out) {
  return guarded([&] {
    check_D(D, h->eng);
    for (const auto& v : h->views)
      if (!(v.eng->gp[v.idx].has_data && v.eng->gp[v.idx].factored))
        throw std::runtime_error("Hyperparameters have not been fit for this Gaussian Process");
    if (!h->multi()) {
      Engine* e = h->eng;
      DeviceGuard g(e->device_id());
      std::vector<int> ids = fitted_ids(e);
      e->implausibility(ids, testing, m, obs, obs_var, discrepancy, include_nugget != 0, rank, out);
      return;
    }
    mogp_implausibility_parts(h, testing, m, obs, obs_var, discrepancy, include_nugget != 0, rank, out);
  });
}
// Emulators are independent: every part runs its own block on its own engine and writes its own rows (no cross-device reduction)
int mogp_mogp_sobol(mogp_mogp* h, const double* A, const double* B, int N, int D, int unc, int include_nugget, double* S, double* ST,
                    double* mean_out, double* variance_out, double* emulator_variance_out) {
  return guarded([&] {
    check_sobol_args(D, h->eng, S, ST, mean_out, variance_out, unc, emulator_variance_out);
    double* ev = unc ? emulator_variance_out : nullptr;
    for_parts(h, [&](mogp_part& p, int) {
      const size_t lo = p.lo;
      engine_sobol(p.eng.get(), A, B, N, unc != 0, include_nugget != 0, S + lo * D, ST + lo * D, mean_out + lo, variance_out + lo,
                   ev ? ev + lo : nullptr);
    });
  });
}
// every part: its fitted emulators in one predict_mixture, the rows of the others NaN
int mogp_mogp_predict_mixture(mogp_mogp* h, const double* thetas, int S, int n_cols, const double* weights, const double* log_q,
                              const double* testing, int m, int D, int include_nugget, int max_slots, int max_points, double* mean_out,
                              double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out,
                              int* ok_all_out) {
  return guarded([&] {
    check_D(D, h->eng);
    if (S < 1) throw std::runtime_error("predict_mixture: at least one sample per emulator is needed (S = " + std::to_string(S) + ")");
    if (!thetas || !mean_out || !within_out || !between_out || !weights_out || !logpost_out || !ok_out)
      throw std::runtime_error("predict_mixture: null buffer");
    if ((weights != nullptr) == (log_q != nullptr)) throw std::runtime_error("predict_mixture: exactly one of weights and log_q must be given");
    if (n_cols != widest_n_theta(h)) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    const size_t mm = (size_t)std::max(m, 0), SS = (size_t)S;
    for_parts(h, [&](mogp_part& p, int) {
      Engine* e = p.eng.get();
      const size_t lo = (size_t)p.lo;
      with_fitted_rows(e,
                       {Rows::in(thetas + lo * SS * n_cols, SS * n_cols), Rows::in(weights ? weights + lo * SS : nullptr, SS),
                        Rows::in(log_q ? log_q + lo * SS : nullptr, SS), Rows::out(mean_out + lo * mm, mm, true),
                        Rows::out(within_out + lo * mm, mm, true), Rows::out(between_out + lo * mm, mm, true),
                        Rows::out(weights_out + lo * SS, SS, true), Rows::out(logpost_out + lo * SS, SS, true),
                        Rows::out(ok_out + lo * SS, SS, true), Rows::out(ok_all_out ? ok_all_out + lo : nullptr, 1, true)},
                       [&](const std::vector<int>& ids, const std::vector<Rows>& a) {
                         predict_mixture(*e, ids, a[0].d(), S, n_cols, a[1].d(), a[2].d(), testing, m, include_nugget != 0, max_slots, max_points,
                                            a[3].d(), a[4].d(), a[5].d(), a[6].d(), a[7].d(), a[8].i(), a[9].i());
                       });
    });
  });
}
// every part: its fitted emulators in one cross_validate, the rows of the others NaN and ok = 0
int mogp_mogp_cross_validate(mogp_mogp* h, const int* labels, int n_labels, int k, int include_nugget, int max_slots, double* mean_out,
                             double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  return guarded([&] {
    if (!labels || !mean_out || !var_out || !maha_out || !log_score_out || !ok_out) throw std::runtime_error("cross_validate: null buffer");
    if (n_labels != h->eng->n) throw std::runtime_error("cross_validate: one fold label per training point is needed");
    if (k < 2 || k > n_labels) throw std::runtime_error("cross_validate: the number of folds must be between 2 and the number of training points");
    const size_t nn = (size_t)n_labels, kk = (size_t)k;
    for_parts(h, [&](mogp_part& p, int) {
      Engine* e = p.eng.get();
      const size_t lo = (size_t)p.lo;
      with_fitted_rows(e,
                       {Rows::out(mean_out + lo * nn, nn, true), Rows::out(var_out + lo * nn, nn, true), Rows::out(maha_out + lo * kk, kk, true),
                        Rows::out(log_score_out + lo * kk, kk, true), Rows::out(ok_out + lo * kk, kk, true)},
                       [&](const std::vector<int>& ids, const std::vector<Rows>& a) {
                         cross_validate(*e, ids, labels, k, include_nugget != 0, max_slots, a[0].d(), a[1].d(), a[2].d(), a[3].d(), a[4].i());
                       });
    });
  });
}
// every part: its fitted emulators in one sample_posterior, each on stream stream0 + its index in the model; the rows of the
// others NaN and ok = 0
int mogp_mogp_sample_posterior(mogp_mogp* h, const double* testing, int m, int D, int S, unsigned long long seed, unsigned int stream0,
                               const double* z_in, int z_in_per_emulator, int include_nugget, double jitter, int max_slots, int max_draws,
                               double* samples_out, double* mean_out, double* z_out, double* jitter_used_out, int* ok_out) {
  return guarded([&] {
    check_D(D, h->eng);
    if (!testing || !samples_out || !mean_out || !jitter_used_out || !ok_out) throw std::runtime_error("sample_posterior: null buffer");
    if (m < 1) throw std::runtime_error("sample_posterior: at least one query point is needed");
    if (S < 1) throw std::runtime_error("sample_posterior: at least one draw is needed (n_draws = " + std::to_string(S) + ")");
    if (h->eng->analytic) throw std::runtime_error("sample_posterior: not available with analytic_mean=True (its covariance term is finished on the host)");
    if (h->nug_type0 == NUG_PIVOT) throw std::runtime_error("sample_posterior: not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
    const size_t mm = (size_t)m, sm = (size_t)S * mm;
    const bool per = z_in && z_in_per_emulator != 0;
    for_parts(h, [&](mogp_part& p, int) {
      Engine* e = p.eng.get();
      const size_t lo = (size_t)p.lo;
      with_fitted_rows(e,
                       {Rows::in(per ? z_in + lo * sm : nullptr, sm), Rows::out(samples_out + lo * sm, sm, true), Rows::out(mean_out + lo * mm, mm, true),
                        Rows::out(z_out ? z_out + lo * sm : nullptr, sm, true), Rows::out(jitter_used_out + lo, 1, true), Rows::out(ok_out + lo, 1, true)},
                       [&](const std::vector<int>& ids, const std::vector<Rows>& a) {
                         std::vector<unsigned> streams(ids.size());
                         for (size_t k = 0; k < ids.size(); ++k) streams[k] = stream0 + (unsigned)(p.lo + ids[k]);
                         sample_posterior(*e, ids, streams.data(), testing, m, S, seed, per ? a[0].d() : z_in, per, include_nugget != 0, jitter,
                                             max_slots, max_draws, a[1].d(), a[2].d(), a[3].d(), a[4].d(), a[5].i());
                       });
    });
  });
}
int mogp_mogp_predict_variance_batch_dev(mogp_mogp* h, const double* d_testing, int m, int D, double* d_means, double* d_vars) {
  return guarded([&] { mogp_predict_dev_common(h, d_testing, m, D, d_means, d_vars, nullptr); });
}
int mogp_mogp_predict_dev(mogp_mogp* h, const double* d_testing, int m, int D, double* d_means, double* d_vars, double* d_derivs) {
  return guarded([&] { mogp_predict_dev_common(h, d_testing, m, D, d_means, d_vars, d_derivs); });
}

}  // extern "C"
