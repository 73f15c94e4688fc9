// The prediction family of Engine: predict and what is fused behind it (full covariance, implausibility, Sobol indices, the mixture over
// hyperparameter samples, cross-validation, leave-one-out variance).  How each cuts its query points to a byte budget is plain arithmetic in predict_plan.h.
#include "engine_internal.h"

#include <cmath>
#include <cstring>
#include <limits>

namespace mogp {

void Engine::require_factored(const std::vector<int>& ids) const {
  for (int i : ids)
    if (!gp[i].factored) throw std::runtime_error("emulator has not been fit");
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
  ensure_linv(ids);
  upload_idx(ids);
  BatchView v = view(nb);
  DevBuf<double> dXf((size_t)m * D), dKf((size_t)nb * MP * LD), dV((size_t)nb * NP * MP), dC((size_t)nb * m * m), dDots((size_t)nb * R * m);
  HIPCK(hipMemcpyAsync(dXf, Xs, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, stream));
  launch_cross_cov_mean(v, dXf, m, MP, dKf, dDots, m, stream);
  launch_cov_self_batch(v, dXf, m, dC, stream);
  launch_predict_fullcov(v, dKf, m, MP, dV, dC, stream);
  std::vector<double> dots((size_t)nb * R * m);
  HIPCK(hipMemcpyAsync(dots.data(), dDots, dots.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(covs, dC, (size_t)nb * m * m * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
  std::vector<double> mv(m), Hs((size_t)q * m), rm((size_t)q * m), dummy(std::max(q, 1), 0.);
  if (R > 1) mean.mean_deriv(Xs, m, D, dummy.data(), q, Hs.data());
  for (int k = 0; k < nb; ++k) {
    const GPState& g = gp[ids[k]];
    const double* dk = dots.data() + (size_t)k * R * m;
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

// Prediction averaged over hyperparameter samples (engine.h has the contract, kernels_mixture.hip the reduction).
//   1. every (emulator, sample) pair is factored on a replica engine, `slots` pairs per pass: F, ok and the nugget used per pair;
//   2. the weights, on the host (mixture_weights);
//   3. per pass and chunk of points the batched mean + variance prediction of the pass's slots, then mixture_accumulate into the
//      (E, 3, m) sums; with more than one pass the slots were overwritten in step 1, so a pass is factored again first (the same bits);
//   4. mixture_finalise and ONE download.
void Engine::predict_mixture(const std::vector<int>& ids, const double* thetas, int S, int ld, const double* weights, const double* log_q,
                             const double* Xs, int m, bool include_nugget, int max_slots, int max_points, double* mean_out,
                             double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out, int* ok_all) {
  const long E = (long)ids.size();
  if (E == 0) return;
  if (S < 1) throw std::runtime_error("predict_mixture: at least one sample per emulator is needed (S = " + std::to_string(S) + ")");
  if (analytic) throw std::runtime_error("predict_mixture: not available with analytic_mean=True (the mean coefficients are integrated out of theta)");
  for (int i : ids)
    if (gp[i].nug_type == NUG_PIVOT)
      throw std::runtime_error("predict_mixture: not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
  if (!thetas || (m > 0 && !Xs)) throw std::runtime_error("predict_mixture: null input buffer");
  if ((weights != nullptr) == (log_q != nullptr)) throw std::runtime_error("predict_mixture: exactly one of weights and log_q must be given");
  if (!mean_out || !within_out || !between_out || !weights_out || !logpost_out || !ok_out) throw std::runtime_error("predict_mixture: null result buffer");
  if (m < 0 || max_slots < 0 || max_points < 0) throw std::runtime_error("predict_mixture: m, max_slots and max_points must not be negative");
  if (E * (long)S > (1L << 30)) throw std::runtime_error("predict_mixture: too many (emulator, sample) pairs");
  for (long e = 0; e < E; ++e) {
    const int P = n_theta(ids[e]);
    if (P > ld) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    for (int s = 0; s < S; ++s) {
      const double* th = thetas + ((size_t)e * S + s) * ld;
      for (int k = 0; k < P; ++k)
        if (!std::isfinite(th[k])) throw std::runtime_error("predict_mixture: the hyperparameter samples must be finite");
      const double x = weights ? weights[e * S + s] : log_q[e * S + s];
      if (!std::isfinite(x)) throw std::runtime_error(weights ? "predict_mixture: the weights must be finite" : "predict_mixture: log_q must be finite");
      if (weights && x < 0.) throw std::runtime_error("predict_mixture: the weights must not be negative");
    }
  }
  for (size_t k = 0; k < (size_t)m * D; ++k)
    if (!std::isfinite(Xs[k])) throw std::runtime_error("predict_mixture: the query points must be finite");

  // slots: what fits beside this engine (fit_map_from's estimate: A, L^-1, K^-1 per slot plus the small per-emulator buffers) and what pays
  const long pairs = E * S;
  long device_slots = pairs;
  double cap = ks_budget_bytes();
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const double per_emu = 3.0 * (double)MS * sizeof(double) + 16.0 * LD * sizeof(double);
      device_slots = (long)std::max(1.0, std::floor(0.5 * (double)free_b / per_emu));
      cap = std::min(cap, 0.25 * (double)free_b);
    }
    device_slots = std::min<long>(device_slots, std::max<long>(E, 4095 / std::max(1, NP / TILE) + 1));
  }
  const MixturePlan plan = mixture_plan(E, S, LD, device_slots, m, max_slots, max_points, cap);
  const long slots = plan.slots, ngroups = (pairs + slots - 1) / slots;
  const int MC = plan.points;
  if (slots > 65535) throw std::runtime_error("predict_mixture: more than 65535 slots per pass are not supported");

  std::vector<double> targets((size_t)slots * n);
  for (long k = 0; k < slots; ++k) {
    const int i = ids[(size_t)(k / S)];
    std::copy(hT.begin() + (size_t)i * n, hT.begin() + (size_t)(i + 1) * n, targets.begin() + (size_t)k * n);
  }
  ReplicaLease rep(*this, slots, targets, gp[ids[0]].nug_type, gp[ids[0]].nug_size);
  hipStream_t st = rep->stream;

  // 1. F, ok and the nugget of every pair
  std::vector<double> F(pairs), nug(pairs, 0.), w(pairs);
  std::vector<int> okv(pairs, 0), holds(slots, -1);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto factor_group = [&](long g) {
    const long p0 = g * slots, cnt = std::min(slots, pairs - p0);
    std::vector<int> sl(cnt);
    std::vector<const double*> th(cnt);
    for (long k = 0; k < cnt; ++k) {
      const int e = (int)((p0 + k) / S);
      if (holds[k] != e) {
        rep->retarget((int)k, *this, ids[e]);
        holds[k] = e;
      }
      sl[k] = (int)k;
      th[k] = thetas + (size_t)(p0 + k) * ld;
    }
    rep->eval(sl, th, false, F.data() + p0, nullptr, 0, okv.data() + p0);
    for (long k = 0; k < cnt; ++k) {
      nug[p0 + k] = okv[p0 + k] ? rep->nugget_size((int)k) : 0.;
      if (!okv[p0 + k]) F[p0 + k] = nan;
    }
  };
  for (long g = 0; g < ngroups; ++g) factor_group(g);

  // 2. weights; the pivot of an emulator is its first sample that factorised
  std::vector<int> alive(E, 0), pivot_pair(E, -1);
  for (long e = 0; e < E; ++e) {
    alive[e] = mixture_weights(S, F.data() + e * S, okv.data() + e * S, weights ? weights + e * S : nullptr, log_q ? log_q + e * S : nullptr,
                               w.data() + e * S) ? 1 : 0;
    for (int s = 0; s < S && pivot_pair[e] < 0; ++s)
      if (okv[e * S + s]) pivot_pair[e] = (int)(e * S + s);
    if (ok_all) ok_all[e] = alive[e];
  }
  std::copy(w.begin(), w.end(), weights_out);
  std::copy(F.begin(), F.end(), logpost_out);
  std::copy(okv.begin(), okv.end(), ok_out);
  if (m == 0) return;

  // 3. the passes
  const size_t mm = (size_t)m;
  DevBuf<double> dXq(mm * D), dAcc((size_t)E * 3 * mm), dPivot((size_t)E * mm), dMu((size_t)slots * MC), dVa((size_t)slots * MC), dPrm(2 * (size_t)slots);
  DevBuf<int> dTab(4 * (size_t)slots), dRows((size_t)slots), dAlive((size_t)E);
  SyncOnUnwind drained{st};
  HIPCK(hipMemcpyAsync(dXq, Xs, mm * D * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemsetAsync(dAcc, 0, (size_t)E * 3 * mm * sizeof(double), st));
  HIPCK(hipMemsetAsync(dPivot, 0, (size_t)E * mm * sizeof(double), st));
  HIPCK(hipMemcpyAsync(dAlive, alive.data(), (size_t)E * sizeof(int), hipMemcpyHostToDevice, st));
  for (long g = 0; g < ngroups; ++g) {
    const long p0 = g * slots, cnt = std::min(slots, pairs - p0);
    std::vector<int> okslots, rows(cnt, -1), etab;
    std::vector<double> prm(2 * (size_t)cnt, 0.);
    for (long k = 0; k < cnt; ++k) {
      if (!okv[p0 + k]) continue;
      rows[k] = (int)okslots.size();
      okslots.push_back((int)k);
      prm[2 * k] = w[p0 + k];
      prm[2 * k + 1] = include_nugget ? nug[p0 + k] : 0.;
    }
    if (okslots.empty()) continue;
    if (ngroups > 1) {
      // the slots hold the last pass of step 1: factor this pass again.  What step 2 was computed from must be what is predicted from.
      const std::vector<double> F1(F.begin() + p0, F.begin() + p0 + cnt);
      const std::vector<int> ok1(okv.begin() + p0, okv.begin() + p0 + cnt);
      factor_group(g);
      for (long k = 0; k < cnt; ++k)
        if (okv[p0 + k] != ok1[k] || (ok1[k] && F[p0 + k] != F1[k]))
          throw std::runtime_error("predict_mixture: a sample did not factorise to the same bits twice");
    }
    for (long e = p0 / S; e <= (p0 + cnt - 1) / S; ++e) {
      const long first = std::max(e * S, p0) - p0, last = std::min((e + 1) * S, p0 + cnt) - p0;
      bool any = false;
      for (long k = first; k < last; ++k) any = any || rows[k] >= 0;
      if (!any || !alive[e]) continue;
      const long pp = pivot_pair[e] - p0;
      etab.insert(etab.end(), {(int)e, (int)first, (int)(last - first), (pp >= 0 && pp < cnt) ? rows[pp] : -1});
    }
    if (etab.empty()) continue;
    HIPCK(hipMemcpyAsync(dTab, etab.data(), etab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dRows, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dPrm, prm.data(), prm.size() * sizeof(double), hipMemcpyHostToDevice, st));
    for (int c0 = 0; c0 < m; c0 += MC) {
      const int mc = std::min(MC, m - c0);
      rep->predict(okslots, dXq + (size_t)c0 * D, mc, true, dMu, dVa, MC, true, nullptr);
      launch_mixture_accumulate(dMu, dVa, MC, mc, (int)(etab.size() / 4), dTab, dRows, dPrm, dAcc, dPivot, m, c0, st);
    }
    HIPCK(hipStreamSynchronize(st));        // the tables are temporaries, and the next pass overwrites the slots
  }
  // 4. finalise, one download
  launch_mixture_finalise((int)E, m, dAlive, dPivot, dAcc, st);
  std::vector<double> res((size_t)E * 3 * mm);
  HIPCK(hipMemcpyAsync(res.data(), dAcc, res.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  HIPCK(hipGetLastError());
  for (long e = 0; e < E; ++e) {
    const double* r = res.data() + (size_t)e * 3 * mm;
    std::copy(r, r + mm, mean_out + (size_t)e * mm);
    std::copy(r + mm, r + 2 * mm, within_out + (size_t)e * mm);
    std::copy(r + 2 * mm, r + 3 * mm, between_out + (size_t)e * mm);
  }
}

// Cross-validation at the fitted hyperparameters (engine.h has the contract, kernels_cv.hip the formulas and the kernels).
//   every fold a single point: L^-1 and ONE launch of cv_loo_kernel;
//   otherwise K^-1, then the (emulator, fold) pairs in passes of `slots` (cv_plan) through a sub-engine of nsub = the largest fold size
//   rows, built as gkdr_R builds its own: per pass factor_prebuilt with cv_gather_kernel as the fill, the log-determinant and L^-T y
//   launchers on the slots that factorised, cv_finish_kernel; ONE download at the end.
// The sub-engine and every buffer here are scratch of the call.
void Engine::cross_validate(const std::vector<int>& ids, const int* labels, int k, bool include_nugget, int max_slots, double* mean_out,
                            double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  require_factored(ids);
  if (analytic) throw std::runtime_error("cross_validate: not available with analytic_mean=True (a held-out fold changes the mean coefficients)");
  for (int i : ids)
    if (gp[i].nug_type == NUG_PIVOT || gp[i].permuted)
      throw std::runtime_error("cross_validate: not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
  if (!labels || !mean_out || !var_out || !maha_out || !log_score_out || !ok_out) throw std::runtime_error("cross_validate: null buffer");
  if (k < 2 || k > n) throw std::runtime_error("cross_validate: the number of folds must be between 2 and the number of training points (k = " + std::to_string(k) + ", n = " + std::to_string(n) + ")");
  if (max_slots < 0) throw std::runtime_error("cross_validate: max_slots must not be negative");
  if (E * (long)k > (1L << 30)) throw std::runtime_error("cross_validate: too many (emulator, fold) pairs");
  std::vector<int> size(k, 0);
  for (int i = 0; i < n; ++i) {
    if (labels[i] < 0 || labels[i] >= k) throw std::runtime_error("cross_validate: fold label " + std::to_string(labels[i]) + " of point " + std::to_string(i) + " is outside [0, " + std::to_string(k) + ")");
    size[labels[i]] += 1;
  }
  int nsub = 0;
  for (int f = 0; f < k; ++f) {
    if (size[f] == 0) throw std::runtime_error("cross_validate: fold " + std::to_string(f) + " is empty");
    nsub = std::max(nsub, size[f]);
  }

  // what both paths share: the observations and nuggets of the rows, the result buffers
  const size_t nn = (size_t)n, kk = (size_t)k;
  std::vector<double> traw((size_t)E * nn), eta(E);
  for (long e = 0; e < E; ++e) {
    std::copy(hT.begin() + (size_t)ids[e] * nn, hT.begin() + (size_t)(ids[e] + 1) * nn, traw.begin() + (size_t)e * nn);
    eta[e] = gp[ids[e]].nugget_used;
  }
  DevBuf<double> dTraw(traw.size()), dEta(eta.size()), dMeanO((size_t)E * nn), dVarO((size_t)E * nn), dMaha((size_t)E * kk), dLs((size_t)E * kk);
  DevBuf<int> dOk((size_t)E * kk);
  auto stage = [&](hipStream_t st) {
    HIPCK(hipMemcpyAsync(dTraw, traw.data(), traw.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dEta, eta.data(), eta.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(dMeanO, 0xFF, (size_t)E * nn * sizeof(double), st));
    HIPCK(hipMemsetAsync(dVarO, 0xFF, (size_t)E * nn * sizeof(double), st));
    HIPCK(hipMemsetAsync(dMaha, 0xFF, (size_t)E * kk * sizeof(double), st));
    HIPCK(hipMemsetAsync(dLs, 0xFF, (size_t)E * kk * sizeof(double), st));
    HIPCK(hipMemsetAsync(dOk, 0, (size_t)E * kk * sizeof(int), st));
  };
  auto download = [&](hipStream_t st) {
    HIPCK(hipMemcpyAsync(mean_out, dMeanO, (size_t)E * nn * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(var_out, dVarO, (size_t)E * nn * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(maha_out, dMaha, (size_t)E * kk * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(log_score_out, dLs, (size_t)E * kk * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(ok_out, dOk, (size_t)E * kk * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
  };

  if (nsub == 1) {
    // leave-one-out: L^-1 only
    DevBuf<int> dLab(nn);
    SyncOnUnwind drained{stream};
    ensure_linv(ids);
    upload_idx(ids);
    stage(stream);
    HIPCK(hipMemcpyAsync(dLab, labels, nn * sizeof(int), hipMemcpyHostToDevice, stream));
    launch_cv_loo(view((int)E), dLab, dTraw, dEta, include_nugget, dMeanO, dVarO, dMaha, dLs, dOk, stream);
    download(stream);
    return;
  }

  // fold index lists (k, nsub), -1 behind the end of a short fold; the points of a fold in ascending order
  std::vector<int> folds((size_t)k * nsub, -1), fillp(k, 0);
  for (int i = 0; i < n; ++i) folds[(size_t)labels[i] * nsub + fillp[labels[i]]++] = i;
  const int NPsub = roundup(nsub + 1, TILE);
  const long pairs = E * k;
  long device_slots = pairs;
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
      device_slots = (long)std::max(1.0, std::floor(0.5 * (double)free_b / cv_slot_bytes(NPsub)));
  }
  const long slots = cv_plan(E, k, NPsub, device_slots, max_slots);

  ensure_kinv(ids, false);
  HIPCK(hipStreamSynchronize(stream));        // the sub-engine reads K^-1 and alpha on its own stream
  const BatchView src = view(0);
  const std::vector<double> zeros((size_t)slots * nsub, 0.0);
  Engine sub(zeros.data(), nsub, 1, zeros.data(), (int)slots, 0, MeanFunc(), 0, NUG_FIXED, 0.0);
  if (sub.NP != NPsub) throw std::runtime_error("cross_validate: unexpected layout of the sub-engine");
  hipStream_t st = sub.stream;
  DevBuf<int> dFolds(folds.size()), dTab(4 * (size_t)slots);
  SyncOnUnwind drained{st};
  stage(st);
  HIPCK(hipMemcpyAsync(dFolds, folds.data(), folds.size() * sizeof(int), hipMemcpyHostToDevice, st));
  std::vector<int> tab(4 * (size_t)slots), info, okslots;
  const std::function<void(const BatchView&)> fill = [&](const BatchView& sv) {
    if (sv.nb != (int)slots) throw std::runtime_error("cross_validate: the factorisation must cover every slot");
    launch_cv_gather(src, dFolds, dTab, (int)slots, sv.A, nsub, NPsub, st);
  };
  for (long p0 = 0; p0 < pairs; p0 += slots) {
    const long cnt = std::min(slots, pairs - p0);
    for (long s = 0; s < slots; ++s) {
      const long e = (p0 + s) / k, f = (p0 + s) % k;
      int* t = tab.data() + 4 * s;
      if (s < cnt) { t[0] = ids[(size_t)e]; t[1] = (int)e; t[2] = (int)f; t[3] = size[f]; }
      else { t[0] = -1; t[1] = t[2] = t[3] = 0; }     // not used: an identity, so that the batch factorises
    }
    HIPCK(hipMemcpyAsync(dTab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    sub.factor_prebuilt(fill, info);
    okslots.clear();
    for (long s = 0; s < cnt; ++s)
      if (info[s] == 0) okslots.push_back((int)s);
    if (!okslots.empty()) {
      sub.upload_idx(okslots);
      const BatchView sv = sub.view((int)okslots.size());
      launch_logdet(sv, sub.dInfo, sub.dRes, st);
      launch_alpha_from_linv(sv, st);
    }
    launch_cv_finish(dFolds, dTab, (int)cnt, sub.dLinv, sub.dAlpha, sub.dRes, sub.dInfo, nsub, NPsub, dTraw, dEta, include_nugget, n, k, dMeanO,
                     dVarO, dMaha, dLs, dOk, st);
    HIPCK(hipStreamSynchronize(st));          // `tab` is rewritten by the next pass
  }
  download(st);
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
