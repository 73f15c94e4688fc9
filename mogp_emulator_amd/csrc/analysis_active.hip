// Active learning (analysis.h has the contracts, kernels_alc.hip the kernels, alc_plan of predict_plan.h the sizing).
//   alc:  1. refusals   2. the factor and L^-1   3. alc_plan   4. per group of emulators: the candidates once -- K*, s^2 and V_c with
//         predict()'s own launches --, then per chunk of reference points K*, s^2, V_r and alc_cross into the per-tile partials, then
//         alc_finish   5. one download per group.
//   predict_cov: the same with the store epilogue and no reduction.
// Every device allocation is a DevBuf local of the call.
#include "analysis.h"
#include "engine_internal.h"

#include <cmath>

namespace mogp {

namespace {

// what alc and predict_cov share: the refusals; and, for the nb emulators in dIdx and the m points at dXq, K* (scratch), the predictive
// variance (dVar, rows var_ld apart; null: not wanted) and V = L^-1 K*^T, with predict()'s own launches
void check_cov_args(const Engine& eng, const char* who, const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_a,
                    int max_b) {
  const std::string p = std::string(who) + ": ";
  eng.require_plain_fit(who, ids, "the covariance gains a term of the mean coefficients");
  if (!X1 || !X2) throw std::runtime_error(p + "null buffer");
  if (m1 < 1 || m2 < 1) throw std::runtime_error(p + "at least one point is needed in each set");
  if (max_a < 0 || max_b < 0) throw std::runtime_error(p + "max_slots and max_points must not be negative");
  require_finite(X1, (size_t)m1 * eng.D, (p + "the points must be finite").c_str());
  if (X2 != X1) require_finite(X2, (size_t)m2 * eng.D, (p + "the points must be finite").c_str());
}

void points_v(Engine& eng, int nb, const double* dXq, int m, int MP, double* dK, double* dDots, double* dPartial, double* dVar, int var_ld,
              double* dV) {
  const BatchView v = eng.view(nb);
  // (the dot products of the fused mean are not used: alpha need not be there)
  launch_cross_cov_mean(v, dXq, m, MP, dK, dDots, MP, eng.stream);
  if (dVar) launch_predict_var(v, dK, m, MP, dPartial, dVar, var_ld, eng.compute_units(), eng.stream);
  launch_predict_v_store(v, dK, m, MP, dV, eng.stream);
}

// what alc and alc_batch refuse alike, as `who`: negative or non-finite weights, weights that sum to 0, negative or non-finite noise;
// tau (ids) receives the noise variances
void check_weights_and_noise(const Engine& eng, const std::string& who, const std::vector<int>& ids, int mr, const double* w,
                             const double* noise, std::vector<double>& tau) {
  double wsum = 0.;
  for (int j = 0; j < mr; ++j) {
    if (!std::isfinite(w[j])) throw std::runtime_error(who + ": the weights must be finite");
    if (w[j] < 0.) throw std::runtime_error(who + ": the weights must not be negative");
    wsum += w[j];
  }
  if (!(wsum > 0.)) throw std::runtime_error(who + ": the weights must not sum to 0");
  tau.resize(ids.size());
  for (size_t e = 0; e < ids.size(); ++e) {
    tau[e] = noise ? noise[e] : eng.nugget_size(ids[e]);
    if (!(tau[e] >= 0.) || !std::isfinite(tau[e])) throw std::runtime_error(who + ": noise must be a finite number that is not negative");
  }
}

}  // namespace

void predict_cov(Engine& eng, const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_slots, double* out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  hipStream_t stream = eng.stream;
  const int D = eng.D, NP = eng.NP, LD = eng.LD;
  const bool same = X2 == nullptr;
  if (same) { X2 = X1; m2 = m1; }
  check_cov_args(eng, "predict_cov", ids, X1, m1, X2, m2, max_slots, 0);
  if (!out) throw std::runtime_error("predict_cov: null buffer");
  eng.ensure_linv(ids);
  const double per = predict_cov_rule_bytes(m1, m2, LD, NP);
  if (per > 64.0e9)
    throw std::runtime_error("predict_cov: " + std::to_string(m1) + " x " + std::to_string(m2) +
                             " points need more than 64 GB of device scratch; use fewer points per call");
  const double free_b = eng.free_bytes_or_twice_budget();
  if (per > 0.5 * free_b)
    throw std::runtime_error("predict_cov: one emulator at " + std::to_string(m1) + " x " + std::to_string(m2) +
                             " points needs more than half of the free device memory; use fewer points per call");
  long slots = std::min<long>(E, std::min<long>(slots_in_half_of(free_b, per), (long)std::floor(64.0e9 / per)));
  slots = std::min<long>(slots, 65535);
  if (max_slots > 0) slots = std::min<long>(slots, max_slots);
  slots = std::max<long>(1, slots);

  const int MP1 = (int)alc_mp(m1), MP2 = (int)alc_mp(m2), MPmax = std::max(MP1, MP2);
  const size_t sl = (size_t)slots, mm = (size_t)m1 * m2;
  DevBuf<double> dX1((size_t)m1 * D), dX2, dK(sl * MPmax * LD), dDots(sl * MPmax), dV1(sl * NP * MP1), dV2, dC(sl * mm);
  if (!same) {
    dX2.reserve((size_t)m2 * D);
    dV2.reserve(sl * NP * MP2);
  }
  SyncOnUnwind drained{stream};
  HIPCK(hipMemcpyAsync(dX1, X1, (size_t)m1 * D * sizeof(double), hipMemcpyHostToDevice, stream));
  if (!same) HIPCK(hipMemcpyAsync(dX2, X2, (size_t)m2 * D * sizeof(double), hipMemcpyHostToDevice, stream));
  for (long e0 = 0; e0 < E; e0 += slots) {
    const int cnt = (int)std::min(slots, E - e0);
    const std::vector<int> grp(ids.begin() + e0, ids.begin() + e0 + cnt);
    eng.upload_idx(grp);
    points_v(eng, cnt, dX1, m1, MP1, dK, dDots, nullptr, nullptr, 0, dV1);
    if (!same) points_v(eng, cnt, dX2, m2, MP2, dK, dDots, nullptr, nullptr, 0, dV2);
    launch_alc_store(eng.view(cnt), dV1, MP1, m1, dX1, same ? dV1.get() : dV2.get(), MP2, m2, same ? dX1.get() : dX2.get(), dC, stream);
    HIPCK(hipMemcpyAsync(out + (size_t)e0 * mm, dC, (size_t)cnt * mm * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));        // the next group overwrites the buffers
    HIPCK(hipGetLastError());
  }
}

void alc(Engine& eng, const std::vector<int>& ids, const double* Xc, int mc, const double* Xr, int mr, const double* w, const double* noise,
         int max_slots, int max_points, double* reduction, double* cand_var, double* ref_var, int* degenerate) {
  const long E = (long)ids.size();
  if (E == 0) return;
  hipStream_t stream = eng.stream;
  const int n = eng.n, D = eng.D, NP = eng.NP, LD = eng.LD;
  // 1. refusals
  check_cov_args(eng, "alc_criterion", ids, Xc, mc, Xr, mr, max_slots, max_points);
  if (!w || !reduction || !cand_var || !ref_var || !degenerate) throw std::runtime_error("alc_criterion: null buffer");
  std::vector<double> tau;
  check_weights_and_noise(eng, "alc_criterion", ids, mr, w, noise, tau);
  // 2. the factor is there (check_cov_args); L^-1
  eng.ensure_linv(ids);
  // 3. plan
  const AlcPlan plan = alc_plan(E, mc, mr, LD, NP, eng.free_bytes_or_twice_budget(), max_slots, max_points);
  const long slots = plan.slots;
  const int CH = (int)plan.points, MPc = (int)alc_mp(mc), tiles_r = (int)(alc_mp(mr) / 128), MPmax = std::max(MPc, CH);
  const size_t sl = (size_t)slots, nti = (size_t)(n + 127) / 128;
  // 4. the groups
  DevBuf<double> dXc((size_t)mc * D), dXr((size_t)mr * D), dW((size_t)mr), dTau(sl), dK(sl * MPmax * LD), dDots(sl * MPmax),
      dPartial(sl * nti * MPmax), dVc(sl * NP * MPc), dVr(sl * NP * CH), dPart(sl * tiles_r * MPc), dVarC(sl * mc), dVarR(sl * mr), dRed(sl * mc);
  DevBuf<int> dDeg(sl * mc);
  SyncOnUnwind drained{stream};
  HIPCK(hipMemcpyAsync(dXc, Xc, (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipMemcpyAsync(dXr, Xr, (size_t)mr * D * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipMemcpyAsync(dW, w, (size_t)mr * sizeof(double), hipMemcpyHostToDevice, stream));
  for (long e0 = 0; e0 < E; e0 += slots) {
    const int cnt = (int)std::min(slots, E - e0);
    const std::vector<int> grp(ids.begin() + e0, ids.begin() + e0 + cnt);
    eng.upload_idx(grp);
    const BatchView v = eng.view(cnt);
    HIPCK(hipMemcpyAsync(dTau, tau.data() + e0, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, stream));
    points_v(eng, cnt, dXc, mc, MPc, dK, dDots, dPartial, dVarC, mc, dVc);
    for (int c0 = 0; c0 < mr; c0 += CH) {
      const int mrc = std::min(CH, mr - c0), MPr = (int)alc_mp(mrc);
      points_v(eng, cnt, dXr + (size_t)c0 * D, mrc, MPr, dK, dDots, dPartial, dVarR + c0, mr, dVr);
      launch_alc_cross(v, dVc, MPc, mc, dXc, dVr, MPr, mrc, dXr + (size_t)c0 * D, dW + c0, NP, alc_kend(n), c0 / 128, tiles_r, dPart, stream);
    }
    launch_alc_finish(v, n, mc, MPc, tiles_r, dPart, dVarC, mc, dTau, dRed, dDeg, stream);
    // 5. one download
    const size_t oc = (size_t)e0 * mc, orr = (size_t)e0 * mr;
    HIPCK(hipMemcpyAsync(reduction + oc, dRed, (size_t)cnt * mc * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(cand_var + oc, dVarC, (size_t)cnt * mc * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(degenerate + oc, dDeg, (size_t)cnt * mc * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCK(hipMemcpyAsync(ref_var + orr, dVarR, (size_t)cnt * mr * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));        // the next group overwrites the buffers
    HIPCK(hipGetLastError());
    for (size_t k = 0; k < (size_t)cnt * mr; ++k)      // s^2 of the reference points as predict() reports it
      if (ref_var[orr + k] < 0.) ref_var[orr + k] = 0.;
  }
}

// ---------------------------------------------------------------------------------------------
// Greedy ALC batches (analysis.h has the contract, alc_batch_plan of predict_plan.h the sizing).
//   AlcBatch():  V and s^2 of both sets with predict()'s own launches, V copied behind one another into buffers of n16 + ext rows per slot
//   scores(t):   alc_cross over the K range [0, n16 + roundup(t, 16)) -- rows not yet written are 0 --, alc_finish with the floor of n + t
//   apply(t, .): the pick on the device, then the row n16 + t of both sets and their s^2
//   finish():    the one download of a group
// ---------------------------------------------------------------------------------------------

void alc_batch_check(const Engine& eng, const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
                     const double* noise, int q, int max_slots, std::vector<double>& tau) {
  check_cov_args(eng, "alc_batch", ids, X, M, Xr, mr, max_slots, 0);
  if (!w) throw std::runtime_error("alc_batch: null buffer");
  if (forced < 0 || forced > M) throw std::runtime_error("alc_batch: the pending points are a prefix of the candidates");
  if (q < 1) throw std::runtime_error("alc_batch: n_points must be at least 1");
  if (q > M - forced) throw std::runtime_error("alc_batch: n_points must not exceed the number of candidates");
  check_weights_and_noise(eng, "alc_batch", ids, mr, w, noise, tau);
}

long alc_batch_slots(const Engine& eng, long E, int M, int mr, int T, int max_slots, bool total) {
  return alc_batch_plan(E, M, mr, T, eng.LD, eng.NP, eng.free_bytes_or_twice_budget(), max_slots, total);
}

AlcBatch::AlcBatch(Engine& eng, const std::vector<int>& grp, const double* tau, const double* X, int M_, int forced, const double* Xr, int mr_,
                   const double* w, int q, const AlcBatchOut& out)
    : e(eng), ids(grp), o(out), cnt((int)grp.size()), M(M_), mr(mr_), T(forced + q), MPc((int)alc_mp(M_)), MPr((int)alc_mp(mr_)),
      tiles_r((int)(alc_mp(mr_) / 128)), rows(alc_kend(eng.n) + (int)alc_ext_rows(forced + q)), n16(alc_kend(eng.n)), hw(w, w + mr_) {
  const int NP = e.NP, LD = e.LD, D = e.D, MPmax = std::max(MPc, MPr);
  const size_t sl = (size_t)cnt, nti = (size_t)(e.n + 127) / 128;
  hipStream_t st = e.stream;
  e.ensure_linv(ids);
  dXc.reserve((size_t)M * D), dXr.reserve((size_t)mr * D), dW.reserve((size_t)mr), dTau.reserve(sl);
  dVc.reserve(sl * rows * MPc), dVr.reserve(sl * rows * MPr), dPart.reserve(sl * tiles_r * MPc);
  dVarC.reserve(sl * M), dVarR.reserve(sl * mr), dRed.reserve(sl * M), dPickRed.reserve(sl * T), dPickD.reserve(sl * T);
  dDeg.reserve(sl * M), dMask.reserve(sl * M), dPicks.reserve(sl * T);
  // scratch of the build alone
  DevBuf<double> dK(sl * MPmax * LD), dDots(sl * MPmax), dPartial(sl * nti * MPmax), dV(sl * NP * MPmax);
  SyncOnUnwind drained{st};
  HIPCK(hipMemcpyAsync(dXc, X, (size_t)M * D * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dXr, Xr, (size_t)mr * D * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dW, w, (size_t)mr * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dTau, tau, sl * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemsetAsync(dVc, 0, sl * rows * MPc * sizeof(double), st));
  HIPCK(hipMemsetAsync(dVr, 0, sl * rows * MPr * sizeof(double), st));
  HIPCK(hipMemsetAsync(dMask, 0, sl * M * sizeof(int), st));
  HIPCK(hipMemsetAsync(dPicks, 0xff, sl * T * sizeof(int), st));
  HIPCK(hipMemsetAsync(dPickRed, 0, sl * T * sizeof(double), st));
  e.upload_idx(ids);
  // the n16 base rows of every slot, from slots NP rows apart to slots `rows` rows apart
  const auto widen = [&](double* dst, int MP) {
    for (size_t s = 0; s < sl; ++s)
      HIPCK(hipMemcpyAsync(dst + s * rows * MP, dV.get() + s * NP * MP, (size_t)n16 * MP * sizeof(double), hipMemcpyDeviceToDevice, st));
  };
  points_v(e, cnt, dXc, M, MPc, dK, dDots, dPartial, dVarC, M, dV);
  widen(dVc, MPc);
  points_v(e, cnt, dXr, mr, MPr, dK, dDots, dPartial, dVarR, mr, dV);
  widen(dVr, MPr);
  HIPCK(hipMemcpyAsync(o.cand_var, dVarC, sl * M * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(o.ref_var, dVarR, sl * mr * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));            // the scratch goes
  HIPCK(hipGetLastError());
  for (size_t k = 0; k < sl * M; ++k)         // s^2 as predict() reports it
    if (o.cand_var[k] < 0.) o.cand_var[k] = 0.;
  for (size_t k = 0; k < sl * mr; ++k)
    if (o.ref_var[k] < 0.) o.ref_var[k] = 0.;
}

void AlcBatch::scores(int t) {
  hipStream_t st = e.stream;
  e.upload_idx(ids);
  const BatchView v = e.view(cnt);
  launch_alc_cross(v, dVc, MPc, M, dXc, dVr, MPr, mr, dXr, dW, rows, n16 + (t + 15) / 16 * 16, 0, tiles_r, dPart, st);
  launch_alc_finish(v, e.n + t, M, MPc, tiles_r, dPart, dVarC, M, dTau, dRed, dDeg, st);
  for (int s = 0; s < cnt; ++s) {            // this step's rows of every slot, (T, M) apart on the host
    if (o.red) HIPCK(hipMemcpyAsync(o.red + ((size_t)s * T + t) * M, dRed.get() + (size_t)s * M, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (o.deg) HIPCK(hipMemcpyAsync(o.deg + ((size_t)s * T + t) * M, dDeg.get() + (size_t)s * M, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, st));
  }
}

void AlcBatch::scores_to_host(int t, double* row_red, int* row_deg) {
  scores(t);
  HIPCK(hipMemcpyAsync(row_red, dRed, (size_t)cnt * M * sizeof(double), hipMemcpyDeviceToHost, e.stream));
  HIPCK(hipMemcpyAsync(row_deg, dDeg, (size_t)cnt * M * sizeof(int), hipMemcpyDeviceToHost, e.stream));
  HIPCK(hipStreamSynchronize(e.stream));
  HIPCK(hipGetLastError());
}

void AlcBatch::apply(int t, int forced) {
  hipStream_t st = e.stream;
  e.upload_idx(ids);
  const BatchView v = e.view(cnt);
  launch_alc_argmax(v, t, T, forced, M, dRed, dVarC, M, dTau, dMask, dPicks, dPickRed, dPickD, st);
  launch_alc_condition(v, t, T, rows, dPicks, dPickD, dVc, MPc, dXc, dVc, MPc, M, dXc, dVarC, M, st);
  launch_alc_condition(v, t, T, rows, dPicks, dPickD, dVc, MPc, dXc, dVr, MPr, mr, dXr, dVarR, mr, st);
}

void AlcBatch::finish() {
  hipStream_t st = e.stream;
  const size_t sl = (size_t)cnt;
  HIPCK(hipMemcpyAsync(o.picks, dPicks, sl * T * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(o.pick_red, dPickRed, sl * T * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(o.ref_var_after, dVarR, sl * mr * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  HIPCK(hipGetLastError());
  for (size_t k = 0; k < sl * mr; ++k)
    if (o.ref_var_after[k] < 0.) o.ref_var_after[k] = 0.;
  for (size_t s = 0; s < sl; ++s) {
    double* iv = o.iv + s * (T + 1);
    double a = 0.;
    for (int j = 0; j < mr; ++j) a += hw[j] * o.ref_var[s * mr + j];
    iv[0] = a;
    for (int t = 0; t < T; ++t) iv[t + 1] = iv[t] - o.pick_red[s * T + t];
  }
}

void alc_batch(Engine& eng, const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
               const double* noise, int q, int max_slots, const AlcBatchOut& out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  std::vector<double> tau;
  alc_batch_check(eng, ids, X, M, forced, Xr, mr, w, noise, q, max_slots, tau);
  if (!out.picks || !out.pick_red || !out.cand_var || !out.ref_var || !out.ref_var_after || !out.iv) throw std::runtime_error("alc_batch: null buffer");
  const int T = forced + q;
  const long slots = alc_batch_slots(eng, E, M, mr, T, max_slots, false);
  for (long e0 = 0; e0 < E; e0 += slots) {
    const long cnt = std::min(slots, E - e0);
    const std::vector<int> grp(ids.begin() + e0, ids.begin() + e0 + cnt);
    AlcBatch run(eng, grp, tau.data() + e0, X, M, forced, Xr, mr, w, q, out.rows_from((size_t)e0, T, M, mr));
    SyncOnUnwind drained{eng.stream};
    for (int t = 0; t < T; ++t) {
      run.scores(t);
      run.apply(t, t < forced ? t : -1);
    }
    run.finish();
  }
}

}  // namespace mogp
