// The prediction family of Engine: predict and what is fused behind it (full covariance, implausibility, Sobol indices, leave-one-out
// variance).  How each cuts its query points to a byte budget is plain arithmetic in predict_plan.h.
#include "engine_internal.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace mogp {

void Engine::require_factored(const std::vector<int>& ids) const {
  for (int i : ids)
    if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
}

void Engine::require_plain_fit(const char* who, const std::vector<int>& ids, const char* analytic_reason) const {
  const std::string p = std::string(who) + ": not available with ";
  require_factored(ids);
  if (analytic) throw std::runtime_error(p + "analytic_mean=True (" + analytic_reason + ")");
  for (int i : ids)
    if (gp[i].nug_type == NUG_PIVOT || gp[i].permuted) throw std::runtime_error(p + "nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
}

void Engine::ensure_predict_scratch(int nb, int MC) {
  dKs.reserve((size_t)nb * MC * LD);
  // partial sums per row tile
  const size_t nti = (n + 127) / 128;
  dVarPartial.reserve((size_t)nb * nti * MC);
}

// fm / fv / fd: where the finished means / variances / derivatives live on the device -- the caller's buffers (out_on_device) or the
// engine's, copied out at the end.  dots: R rows of dot products per emulator (row 0 = k*^T K^-1 (t - H beta), rows 1.. = k*^T K^-1 h_c);
// with R = 1 that row IS the mean (before the mean-function term) and lands in the result rows directly.
Engine::PredictPlace Engine::place_predict_outputs(int nb, int m, double* means, double* vars, double* derivs, long out_ld, bool out_on_device) {
  PredictPlace o{means, vars, derivs, nullptr, out_ld, 0};
  if (!means && vars) throw std::runtime_error("predict: variances without means");
  if (!out_on_device && means) {
    dMeanFin.reserve((size_t)nb * m);
    o.fm = dMeanFin;
    o.ld = m;
    if (vars) {
      dVar.reserve((size_t)nb * m);
      o.fv = dVar;
    }
  }
  if (!out_on_device && derivs) {
    dDeriv.reserve((size_t)nb * m * D);
    o.fd = dDeriv;
  }
  o.dots = o.fm;
  o.dots_ld = o.ld;
  if (R > 1 && means) {
    dMean.reserve((size_t)nb * R * m);
    o.dots = dMean;
    o.dots_ld = m;
  }
  return o;
}

// dot products (and variances where o.fv is set) of the m points at dXsrc, one chunk of cross covariances at a time
void Engine::predict_chunks(const BatchView& v, const double* dXsrc, int m, const PredictPlace& o) {
  // never more than half of what the device has free right now (several engines / ranks per GPU, smaller devices);
  // what is already allocated for the chunk counts as free
  double cap = ks_budget_bytes();
  if (o.fv) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) cap = std::min(cap, 0.5 * ((double)free_b + (double)dKs.size() * sizeof(double)));
  }
  const int MC = predict_chunk_points(cap, v.nb, LD, m);
  if (o.fv) ensure_predict_scratch(v.nb, MC);
  for (int c0 = 0; c0 < m; c0 += MC) {
    const int mc = std::min(MC, m - c0);
    const int MPc = roundup(mc, 128);
    launch_cross_cov_mean(v, dXsrc + (size_t)c0 * D, mc, MPc, o.fv ? dKs : nullptr, o.dots + c0, (int)o.dots_ld, stream);
    if (o.fv) launch_predict_var(v, dKs, mc, MPc, dVarPartial, o.fv + c0, (int)o.ld, n_cu, stream);
  }
}

// mean-function terms, on the device: the basis columns from the device-resident test points (mean_basis_kernel), then
// predict_mean_finish_kernel.  Coefficients, LA and the polynomial's dims / powers are staged through dMeanAux (MeanStage, predict_plan.h).
void Engine::add_mean_terms(const std::vector<int>& ids, const double* dXsrc, int m, const PredictPlace& o) {
  const int nb = (int)ids.size();
  const int nterm = (mean.kind == 3) ? (int)mean.dims.size() : 0;
  const int nbasis = 1 + nterm;
  const int qq = R - 1;
  if (R > 1 && qq != nbasis) throw std::runtime_error("predict: analytic mean with an unexpected number of columns");
  const MeanStage s(nb, m, nbasis, nterm, qq);
  std::vector<double> st(s.total - s.o_coef, 0.);
  for (int k = 0; k < nb; ++k) {
    const GPState& g = gp[ids[k]];
    double* c = st.data() + (size_t)k * nbasis;
    if (R > 1) {
      for (int t = 0; t < qq; ++t) c[t] = g.beta[t];
      for (int e = 0; e < qq * qq; ++e) st[(s.o_la - s.o_coef) + (size_t)k * qq * qq + e] = g.LA[e];
    } else if (mean.kind == 1) c[0] = mean.value;
    else
      for (int t = 0; t < nbasis; ++t) c[t] = g.meanp[t];
  }
  // (ints packed behind the doubles of the same staging block: copied in, not written through a punned pointer)
  std::vector<int> hi(2 * (size_t)nterm + 2, 0);
  for (int t = 0; t < nterm; ++t) {
    hi[t] = mean.dims[t];
    hi[nterm + t] = mean.powers[t];
  }
  std::memcpy(st.data() + (s.o_int - s.o_coef), hi.data(), 2 * (size_t)nterm * sizeof(int));
  dMeanAux.reserve(s.total);
  HIPCK(hipMemcpyAsync(dMeanAux + s.o_coef, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  const int* di = reinterpret_cast<const int*>(dMeanAux + s.o_int);
  launch_mean_basis(dXsrc, m, D, nterm, di, di + nterm, dMeanAux + s.o_basis, dMeanAux + s.o_dbasis, stream);
  launch_predict_mean_finish(nb, m, D, R, nbasis, dMeanAux + s.o_basis, dMeanAux + s.o_coef, R > 1 ? o.dots : nullptr, dMeanAux + s.o_la, o.fm,
                             R > 1 ? o.fv : nullptr, o.ld, o.fd ? nterm : 0, dMeanAux + s.o_dbasis, di, di + nterm, o.fd, stream);
  HIPCK(hipStreamSynchronize(stream));      // `st` is the source of an asynchronous copy
}

// the engine's result buffers into the caller's host arrays (rows of the means / variances out_ld apart)
void Engine::copy_out_predictions(const PredictPlace& o, int nb, int m, double* means, double* vars, long out_ld, double* derivs) {
  if (means && out_ld == m) {        // contiguous result arrays: one transfer each instead of one per emulator
    HIPCK(hipMemcpyAsync(means, o.fm, (size_t)nb * m * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (vars) HIPCK(hipMemcpyAsync(vars, o.fv, (size_t)nb * m * sizeof(double), hipMemcpyDeviceToHost, stream));
  } else if (means) {
    for (int k = 0; k < nb; ++k) {
      HIPCK(hipMemcpyAsync(means + (size_t)k * out_ld, o.fm + (size_t)k * m, m * sizeof(double), hipMemcpyDeviceToHost, stream));
      if (vars) HIPCK(hipMemcpyAsync(vars + (size_t)k * out_ld, o.fv + (size_t)k * m, m * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
  }
  if (derivs) HIPCK(hipMemcpyAsync(derivs, o.fd, (size_t)nb * m * D * sizeof(double), hipMemcpyDeviceToHost, stream));
}

// place the outputs -> dot products and variances per chunk -> derivatives -> mean-function terms -> copy out
void Engine::predict(const std::vector<int>& ids, const double* Xs, int m, bool xs_on_device, double* means, double* vars, long out_ld,
                     bool out_on_device, double* derivs) {
  const int nb = (int)ids.size();
  if (nb == 0 || m == 0) return;
  require_factored(ids);
  ensure_alpha(ids);
  if (vars) ensure_linv(ids);
  upload_idx(ids);
  const BatchView v = view(nb);
  const double* dXsrc = Xs;
  if (!xs_on_device) {
    dXs.reserve((size_t)m * D);
    HIPCK(hipMemcpyAsync(dXs, Xs, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, stream));
    dXsrc = dXs;
  }
  const PredictPlace o = place_predict_outputs(nb, m, means, vars, derivs, out_ld, out_on_device);
  if (means) predict_chunks(v, dXsrc, m, o);       // derivatives only (mogp_*_predict_deriv): no cross covariance, no mean
  if (derivs) launch_predict_deriv(v, dXsrc, m, o.fd, (long)m * D, stream);
  if (mean.kind != 0 || R > 1) add_mean_terms(ids, dXsrc, m, o);
  if (!out_on_device) copy_out_predictions(o, nb, m, means, vars, out_ld, derivs);
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
}

void Engine::predict_full_cov(const std::vector<int>& ids, const double* Xs, int m, double* means, double* covs) {
  const int nb = (int)ids.size();
  if (nb == 0 || m == 0) return;
  require_factored(ids);
  const int MP = roundup(m, 128);
  const double need = (double)nb * 8.0 * ((double)LD * MP * 2.0 + (double)m * m);
  if (need > 64.0e9)
    throw std::runtime_error("full_cov: " + std::to_string(nb) + " x " + std::to_string(m) +
                             " test points need more than 64 GB of device scratch; use fewer points per call");
  ensure_alpha(ids);
  ensure_linv(ids);
  upload_idx(ids);
  DevBuf<double> dXf((size_t)m * D), dKf((size_t)nb * MP * LD), dV((size_t)nb * NP * MP), dC((size_t)nb * m * m), dDots((size_t)nb * R * m);
  HIPCK(hipMemcpyAsync(dXf, Xs, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, stream));
  fullcov_launches(nb, dXf, m, MP, dKf, dV, dC, dDots);
  std::vector<double> dots((size_t)nb * R * m);
  HIPCK(hipMemcpyAsync(dots.data(), dDots, dots.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(covs, dC, (size_t)nb * m * m * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
  fullcov_host_means(ids, Xs, m, dots.data(), means, covs);
}

// the device part of predict_full_cov for the emulators in dIdx: cross covariance and dot products, K**, Sigma* = K** - V^T V
void Engine::fullcov_launches(int nb, const double* dXf, int m, int MP, double* dKf, double* dV, double* dC, double* dDots) {
  const BatchView v = view(nb);
  launch_cross_cov_mean(v, dXf, m, MP, dKf, dDots, m, stream);
  launch_cov_self_batch(v, dXf, m, dC, stream);
  launch_predict_fullcov(v, dKf, m, MP, dV, dC, stream);
}

// the host part: the means from the dot products, the mean-function terms added (and, with the analytic mean, its covariance term)
void Engine::fullcov_host_means(const std::vector<int>& ids, const double* Xs, int m, const double* dots, double* means, double* covs) {
  const int nb = (int)ids.size();
  std::vector<double> mv(m), Hs((size_t)q * m), rm((size_t)q * m), dummy(std::max(q, 1), 0.);
  if (R > 1) mean.mean_deriv(Xs, m, D, dummy.data(), q, Hs.data());
  for (int k = 0; k < nb; ++k) {
    const GPState& g = gp[ids[k]];
    const double* dk = dots + (size_t)k * R * m;
    double* mu = means + (size_t)k * m;
    for (int j = 0; j < m; ++j) mu[j] = dk[j];
    if (R > 1) {
      fullcov_mean_terms(q, m, g.beta.data(), g.LA.data(), Hs.data(), dk, mu, rm.data(), covs + (size_t)k * m * m);
    } else if (mean.kind != 0) {
      mean.mean_f(Xs, m, D, g.meanp.data(), n_mean(), mv.data());
      for (int j = 0; j < m; ++j) mu[j] += mv[j];
    }
  }
}

// what implausibility and implausibility_top share in front of their buffers: the refusals, and the query points per chunk that both
// the buffers and the chunk loop are sized by (0: nothing to do)
int Engine::implausibility_chunk_points(const std::vector<int>& ids, int m) const {
  if (ids.empty() || m == 0) return 0;
  require_factored(ids);
  if (R > 1 || n_mean() > 0)
    throw std::runtime_error("implausibility: the fused device path supports zero / fixed mean functions only");
  return predict_chunk_points(implausibility_cap_bytes, (int)ids.size(), LD, m);
}

void Engine::implausibility_chunks(const std::vector<int>& ids, const double* Xs, int m, int MC, const double* obs, const double* obs_var,
                                   const double* discrepancy, bool include_nugget, const std::function<void(const double*, int, int)>& tail) {
  const int nb = (int)ids.size();
  std::vector<double> prm((size_t)nb * 3);
  for (int k = 0; k < nb; ++k) {
    if (discrepancy[k] < 0.) throw std::runtime_error("Model discrepancy variance cannot be negative");
    if (obs_var[k] < 0.) throw std::runtime_error("observation variance cannot be negative");
    prm[3 * k] = obs[k];
    prm[3 * k + 1] = obs_var[k] + discrepancy[k] + (include_nugget ? nugget_size(ids[k]) : 0.);
    prm[3 * k + 2] = (mean.kind == 1) ? mean.value : 0.;
  }
  ensure_alpha(ids);
  ensure_linv(ids);
  upload_idx(ids);
  BatchView v = view(nb);
  ensure_predict_scratch(nb, MC);
  dXs.reserve((size_t)MC * D);
  dMean.reserve((size_t)nb * MC);
  dVar.reserve((size_t)nb * MC);
  DevBuf<double> dPrm(prm.size());
  SyncOnUnwind drained{stream};
  HIPCK(hipMemcpyAsync(dPrm, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  for (int c0 = 0; c0 < m; c0 += MC) {
    const int mc = std::min(MC, m - c0);
    const int MPc = roundup(mc, 128);
    HIPCK(hipMemcpyAsync(dXs, Xs + (size_t)c0 * D, (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, stream));
    launch_cross_cov_mean(v, dXs, mc, MPc, dKs, dMean, MC, stream);
    launch_predict_var(v, dKs, mc, MPc, dVarPartial, dVar, MC, n_cu, stream);
    tail(dPrm, c0, mc);
    HIPCK(hipStreamSynchronize(stream));      // dXs is re-used by the next chunk
  }
  HIPCK(hipGetLastError());
}

void Engine::implausibility(const std::vector<int>& ids, const double* Xs, int m, const double* obs, const double* obs_var,
                            const double* discrepancy, bool include_nugget, int rank, double* out) {
  const int nb = (int)ids.size(), MC = implausibility_chunk_points(ids, m);
  if (MC == 0) return;
  if (nb == 1) rank = 0;                                       // HistoryMatching.py:254-255
  if (rank < 0) throw std::runtime_error("rank must be a non-negative integer");
  if (rank >= nb) throw std::runtime_error("rank must be less than the number of observations");
  if (rank > IMPLAUS_MAX_RANK) throw std::runtime_error("rank above " + std::to_string(IMPLAUS_MAX_RANK) + " is not supported on the device");
  DevBuf<double> dOut((size_t)MC);
  implausibility_chunks(ids, Xs, m, MC, obs, obs_var, discrepancy, include_nugget, [&](const double* dPrm, int c0, int mc) {
    launch_implausibility(nb, dMean, dVar, MC, mc, dPrm, rank, dOut, stream);
    HIPCK(hipMemcpyAsync(out + c0, dOut, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, stream));
  });
}

void Engine::implausibility_top(const std::vector<int>& ids, const double* Xs, int m, const double* obs, const double* obs_var,
                                const double* discrepancy, bool include_nugget, int keep, double* out, long out_ld, int out_device) {
  const int nb = (int)ids.size(), MC = implausibility_chunk_points(ids, m);
  if (MC == 0) return;
  if (keep < 1 || keep > IMPLAUS_MAX_RANK + 1) throw std::runtime_error("implausibility: bad number of largest values to keep");
  // the lists go straight into `out` when it lives on this engine's device, else through a scratch block and a peer copy
  const bool local = out_device == device;
  DevBuf<double> dTop;
  if (!local) dTop.reserve((size_t)keep * MC);
  implausibility_chunks(ids, Xs, m, MC, obs, obs_var, discrepancy, include_nugget, [&](const double* dPrm, int c0, int mc) {
    if (local) {
      launch_implausibility_top(nb, dMean, dVar, MC, mc, dPrm, keep, out + c0, out_ld, stream);
      return;
    }
    launch_implausibility_top(nb, dMean, dVar, MC, mc, dPrm, keep, dTop, MC, stream);
    for (int r = 0; r < keep; ++r)
      HIPCK(hipMemcpyPeerAsync(out + (size_t)r * out_ld + c0, out_device, dTop + (size_t)r * MC, device, (size_t)mc * sizeof(double), stream));
  });
}

// First-order and total-effect Sobol indices of the predictive means (kernels_sobol.hip has the estimators).  Pass 1 predicts A and B
// (one resident (2N, D) block) through predict()'s device-to-device path and keeps the means; pass 2 goes over the inputs and chunks of
// base rows: pick-freeze into dPick, the same mean path, the two sums into per-workgroup slots.  Only SOBOL_STATS + 2 D numbers per
// emulator come back.  Everything runs on the main stream; predict() synchronises it at the end of every call.
void Engine::sobol(const std::vector<int>& ids, const double* A, const double* Bs, long N, bool unc, bool include_nugget, double* S,
                   double* ST, double* mean_out, double* var_out, double* emvar_out) {
  const int nb = (int)ids.size();
  if (nb == 0) return;
  if (!A || !Bs) throw std::runtime_error("sobol: null sample matrix");
  if (N < 2) throw std::runtime_error("sobol: at least two base samples are needed (N = " + std::to_string(N) + ")");
  if (N > (1L << 28)) throw std::runtime_error("sobol: at most 2^28 base samples are supported");
  require_factored(ids);
  for (size_t e = 0; e < (size_t)N * D; ++e)
    if (!std::isfinite(A[e]) || !std::isfinite(Bs[e])) throw std::runtime_error("sobol: the sample matrices must be finite");
  const long M2 = 2 * N;
  // resident for the whole call: the samples, fA | fB (and their variances); refused beyond half of the free memory
  const double resident = 8.0 * ((double)M2 * D + (double)nb * M2 * (unc ? 2.0 : 1.0));
  size_t free_b = 0, total_b = 0;
  const bool have_free = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  if (have_free && resident > 0.5 * (double)free_b)
    throw std::runtime_error("sobol: the means of " + std::to_string(N) + " base samples x " + std::to_string(nb) +
                             " emulators do not fit half of the free device memory; use fewer base samples");
  // rows per chunk of pass 2: the chunk of AB_i, its means and predict()'s dot-product rows within predict()'s own budget
  double cap = ks_budget_bytes();
  if (have_free) cap = std::min(cap, 0.5 * ((double)free_b - resident));
  const long CH = sobol_chunk_rows(cap, D, nb, R, mean.kind, (int)mean.dims.size(), N);
  const long nchunks = (N + CH - 1) / CH;
  const int groups = sobol_groups(CH);
  const long nslot = nchunks * groups;
  const size_t n_part = std::max<size_t>((size_t)nb * SOBOL_MAX_GROUPS, (size_t)nb * D * nslot * 2);
  DevBuf<double> dS((size_t)M2 * D), dF((size_t)nb * M2), dV, dPick((size_t)CH * D), dFab((size_t)nb * CH), dPart(n_part),
      dStats((size_t)nb * SOBOL_STATS), dSums((size_t)nb * D * 2);
  if (unc) dV.reserve((size_t)nb * M2);
  SyncOnUnwind drained{stream};
  std::vector<double> stats((size_t)nb * SOBOL_STATS, 0.);
  // the nugget predict() adds to the variances on the host (not with nugget="pivot", GaussianProcess.py:915)
  for (int k = 0; k < nb; ++k)
    stats[(size_t)k * SOBOL_STATS + 3] = (include_nugget && gp[ids[k]].nug_type != NUG_PIVOT) ? nugget_size(ids[k]) : 0.;
  HIPCK(hipMemcpyAsync(dStats, stats.data(), stats.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipMemcpyAsync(dS, A, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipMemcpyAsync(dS + (size_t)N * D, Bs, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice, stream));
  // pass 1: fA | fB, then f0 and V (two passes over the resident means), and the mean predictive variance
  predict(ids, dS, (int)M2, true, dF, dV, M2, true, nullptr);
  launch_sobol_row_mean(nb, 0, dF, M2, M2, nullptr, 0, dPart, dStats + 0, SOBOL_STATS, stream);
  launch_sobol_row_mean(nb, 1, dF, M2, M2, dStats + 0, SOBOL_STATS, dPart, dStats + 1, SOBOL_STATS, stream);
  if (unc) launch_sobol_row_mean(nb, 2, dV, M2, M2, dStats + 3, SOBOL_STATS, dPart, dStats + 2, SOBOL_STATS, stream);
  // pass 2
  for (int col = 0; col < D; ++col) {
    for (long c = 0; c < nchunks; ++c) {
      const long r0 = c * CH;
      const int rows = (int)std::min<long>(CH, N - r0);
      launch_sobol_pick_freeze(dS, dS + (size_t)N * D, r0, rows, D, col, dPick, stream);
      predict(ids, dPick, rows, true, dFab, nullptr, CH, true, nullptr);
      launch_sobol_pair_sum(nb, dF + r0, dF + N + r0, M2, dFab, CH, rows, dStats, SOBOL_STATS, dPart, D, col, nslot, c * groups, groups,
                            stream);
    }
  }
  launch_sobol_pair_final(nb * D, dPart, nslot, 1.0 / (double)N, dSums, stream);
  std::vector<double> sums((size_t)nb * D * 2);
  HIPCK(hipMemcpyAsync(stats.data(), dStats, stats.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(sums.data(), dSums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < nb; ++k) {
    const double* st = stats.data() + (size_t)k * SOBOL_STATS;
    const double V = st[1];
    mean_out[k] = st[0];
    var_out[k] = V;
    if (emvar_out) emvar_out[k] = unc ? st[2] : nan;
    for (int d = 0; d < D; ++d) {
      // a constant emulator (V == 0) has no indices: NaN, not an error
      S[(size_t)k * D + d] = V > 0. ? sums[((size_t)k * D + d) * 2] / V : nan;
      ST[(size_t)k * D + d] = V > 0. ? sums[((size_t)k * D + d) * 2 + 1] / (2. * V) : nan;
    }
  }
}

void Engine::loo_variance(int i, double* out) {
  std::vector<int> ids{i};
  require_factored(ids);
  ensure_linv(ids);
  upload_idx(ids);
  DevBuf<double> tmp((size_t)n);
  launch_loo_variance(view(1), tmp, n, stream);
  HIPCK(hipMemcpyAsync(out, tmp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  unpermute(i, out);
}

}  // namespace mogp
