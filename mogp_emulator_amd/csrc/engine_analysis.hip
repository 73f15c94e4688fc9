// The analysis family of Engine: what is computed AROUND a fit rather than by it -- the Hessian of the log-posterior, the prediction
// averaged over hyperparameter samples, cross-validation, joint posterior draws and the active-learning criterion.  Each reads as its steps; the host algebra of the Hessian is
// hessian_assemble (hostmath.h), the sizing rules and the index tables of the passes are plain arithmetic in predict_plan.h.
#include "engine_internal.h"

#include <cmath>
#include <limits>

namespace mogp {

// ---------------------------------------------------------------------------------------------
// Hessian of the negative log-posterior at per-emulator thetas (kernels_hess.hip, DESIGN.md section 3 "Hessian"): H holds one ld x ld
// row-major block per entry of ids, its leading n_theta x n_theta block filled (both triangles, exactly symmetric) and the rest of it
// NaN (an emulator narrower than ld), all of it NaN where the factorisation fails (ok = 0).  An emulator already fit at exactly theta is not evaluated again; one that was fit elsewhere is put back
// at its own theta afterwards, so its cached state is what it was.  The planes M_p are scratch of this call, taken per group of
// emulators within the prediction's chunk budget and freed before it returns.
// ---------------------------------------------------------------------------------------------

// the device scratch of one group of m emulators; `drained` comes last, so that the stream is drained before the buffers go when the
// group is left through an exception
struct Engine::HessianScratch {
  DevBuf<double> dXs, dMp, dTp, dTo, dPp, dPo, dV, dU, dZv;
  SyncOnUnwind drained;
  HessianScratch(size_t m, int NPh, int D, int TG, int PGR, hipStream_t st)
      : dXs(m * NPh * D), dMp(m * D * ((size_t)NPh * NPh)), dTp(m * TG * ((D + 1) * (D + 2))), dTo(m * ((D + 1) * (D + 2))), dPp(m * PGR * D * D),
        dPo(m * D * D), dV(m * D * NPh), dU(m * D * NPh), dZv(m * NPh), drained{st} {}
};

// the host copies of a group's sums (kept from one group to the next)
struct Engine::HessianSums {
  std::vector<double> go, To, Po, V, U, Zv;
};

// Brings the emulators of ids to their thetas: fine[k] = 1 where emulator ids[k] holds a factor at thetas[k] afterwards -- it was there
// already, or it was evaluated there --, before[k] = the theta a fitted emulator was moved away from (empty: nothing to put back).
// Every block of H is set to NaN on the way.
void Engine::hessian_move_to(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, std::vector<int>& fine,
                             std::vector<std::vector<double>>& before) {
  const int nb = (int)ids.size();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int> ev_ids, ev_pos;
  std::vector<const double*> ev_th;
  for (int k = 0; k < nb; ++k) {
    const int i = ids[k];
    const GPState& g = gp[i];
    const int P = n_theta(i);
    if (P > ld) throw std::runtime_error("logpost_hessian: the result buffer passed was too small");
    std::fill(H + (size_t)k * ld * ld, H + (size_t)(k + 1) * ld * ld, nan);
    const bool fit = g.has_data && g.factored;
    if (fit && !g.logpost_stale && std::equal(g.data.begin(), g.data.end(), thetas[k])) {
      fine[k] = 1;
      continue;
    }
    if (fit) before[k] = g.data;
    ev_ids.push_back(i);
    ev_pos.push_back(k);
    ev_th.push_back(thetas[k]);
  }
  if (!ev_ids.empty()) {
    std::vector<double> f(ev_ids.size());
    std::vector<int> okv(ev_ids.size());
    eval(ev_ids, ev_th, false, f.data(), nullptr, 0, okv.data());
    for (size_t e = 0; e < ev_ids.size(); ++e) fine[ev_pos[e]] = okv[e];
  }
}

// back to where the emulators were
void Engine::hessian_put_back(const std::vector<int>& ids, const std::vector<std::vector<double>>& before) {
  std::vector<int> rb_ids;
  std::vector<const double*> rb_th;
  for (size_t k = 0; k < ids.size(); ++k)
    if (!before[k].empty()) {
      rb_ids.push_back(ids[k]);
      rb_th.push_back(before[k].data());
    }
  if (!rb_ids.empty()) {
    std::vector<double> f(rb_ids.size());
    std::vector<int> okv(rb_ids.size());
    eval(rb_ids, rb_th, false, f.data(), nullptr, 0, okv.data());
  }
}

// the device sums of the emulators of grp (K^-1 is there): the gradient's, then scale, planes, trace, pair and vectors; six downloads,
// ONE synchronisation
void Engine::hessian_group_sums(const std::vector<int>& grp, HessianScratch& d, HessianSums& h) {
  const size_t m = grp.size();
  const int NPh = hess_np(n), TS = (D + 1) * (D + 2);
  upload_idx(grp);
  BatchView v = view((int)m);
  launch_grad(v, dGradPartial, dGradOut, stream);
  launch_hess_scale(v, d.dXs, stream);
  launch_hess_planes(v, d.dXs, d.dMp, stream);
  launch_hess_trace(v, d.dMp, d.dTp, d.dTo, stream);
  launch_hess_pair(v, d.dXs, d.dPp, d.dPo, stream);
  launch_hess_vectors(v, d.dMp, d.dV, d.dU, d.dZv, stream);
  h.To.resize(m * TS); h.Po.resize(m * D * D); h.V.resize(m * D * NPh); h.U.resize(m * D * NPh); h.Zv.resize(m * NPh);
  HIPCK(hipMemcpyAsync(h.go.data(), dGradOut, h.go.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.To.data(), d.dTo, h.To.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.Po.data(), d.dPo, h.Po.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.V.data(), d.dV, h.V.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.U.data(), d.dU, h.U.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipMemcpyAsync(h.Zv.data(), d.dZv, h.Zv.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCK(hipStreamSynchronize(stream));
  HIPCK(hipGetLastError());
}

void Engine::hessian(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, int* ok) {
  const int nb = (int)ids.size();
  if (nb == 0) return;
  if (analytic) throw std::runtime_error("logpost_hessian: not available with analytic_mean=True (the mean coefficients are integrated out of theta)");
  if (n_mean() > 0) throw std::runtime_error("logpost_hessian: not available for a mean function with parameters in theta");
  if (kernel_type == 2) throw std::runtime_error("logpost_hessian: not available for the ProductMat52 kernel");
  for (int i : ids)
    if (gp[i].nug_type == NUG_PIVOT)
      throw std::runtime_error("logpost_hessian: not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
  std::vector<std::vector<double>> before(nb);      // theta of the emulators that have to be put back
  std::vector<int> fine(nb, 0);
  hessian_move_to(ids, thetas, H, ld, fine, before);
  std::vector<int> good, gpos;
  for (int k = 0; k < nb; ++k)
    if (fine[k]) {
      good.push_back(ids[k]);
      gpos.push_back(k);
    }
  if (!good.empty()) {
    ensure_alpha(good);
    ensure_kinv(good, true);
    const int NPh = hess_np(n), NQ = D + 3, TQ = D + 2, TS = (D + 1) * TQ, TG = hess_trace_groups(n), PGR = hess_pair_groups(n);
    const size_t gsz = hessian_group_size(ks_budget_bytes(), hessian_scratch_bytes(NPh, D, TG, PGR), good.size());
    HessianSums h;
    h.go.resize((size_t)B * NQ);
    std::vector<double> al(n), tt(n), dpr(NC + 2), Fd((size_t)TQ * TQ);
    for (size_t g0 = 0; g0 < good.size(); g0 += gsz) {
      const std::vector<int> grp(good.begin() + g0, good.begin() + std::min(good.size(), g0 + gsz));
      HessianScratch dev(grp.size(), NPh, D, TG, PGR, stream);      // (lives to the end of the iteration, as the planes always did)
      hessian_group_sums(grp, dev, h);
      for (size_t s = 0; s < grp.size(); ++s) {
        const int i = grp[s], k = gpos[g0 + s];
        const GPState& g = gp[i];
        HIPCK(hipMemcpy(al.data(), dAlpha + (size_t)i * RA * LD, n * sizeof(double), hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(tt.data(), dT + (size_t)i * n, n * sizeof(double), hipMemcpyDeviceToHost));
        const int P = n_theta(i);
        std::vector<double> Hm((size_t)P * P, 0.);
        g.pri.d2logpdtheta2(g.data, NC, g.nug_type, dpr.data());
        if (!hessian_assemble(n, D, NC, uniform(), g.nug_type == NUG_FIT, g.nugget_used, h.go.data() + (size_t)i * NQ, h.To.data() + s * TS,
                              h.Po.data() + s * D * D, h.V.data() + s * D * NPh, h.U.data() + s * D * NPh, NPh, h.Zv.data() + s * NPh, al.data(),
                              tt.data(), dpr.data(), Fd.data(), Hm.data())) {
          fine[k] = 0;
          continue;
        }
        for (int r = 0; r < P; ++r)
          for (int c = r; c < P; ++c) H[((size_t)k * ld + r) * ld + c] = H[((size_t)k * ld + c) * ld + r] = Hm[(size_t)r * P + c];
      }
    }
  }
  hessian_put_back(ids, before);
  if (ok)
    for (int k = 0; k < nb; ++k) ok[k] = fine[k];
}

// ---------------------------------------------------------------------------------------------
// Prediction averaged over hyperparameter samples (engine.h has the contract, kernels_mixture.hip the reduction).
//   1. every (emulator, sample) pair is factored on a replica engine, `slots` pairs per pass: F, ok and the nugget used per pair;
//   2. the weights, on the host (mixture_weights);
//   3. per pass and chunk of points the batched mean + variance prediction of the pass's slots, then mixture_accumulate into the
//      (E, 3, m) sums; with more than one pass the slots were overwritten in step 1, so a pass is factored again first (the same bits);
//   4. mixture_finalise and ONE download.
// ---------------------------------------------------------------------------------------------

namespace {

// the refusals of predict_mixture
void check_mixture_args(const Engine& eng, const std::vector<int>& ids, const double* thetas, int S, int ld, const double* weights, const double* log_q,
                        const double* Xs, int m, int max_slots, int max_points, const double* mean_out, const double* within_out,
                        const double* between_out, const double* weights_out, const double* logpost_out, const int* ok_out) {
  const long E = (long)ids.size();
  if (S < 1) throw std::runtime_error("predict_mixture: at least one sample per emulator is needed (S = " + std::to_string(S) + ")");
  if (eng.analytic) throw std::runtime_error("predict_mixture: not available with analytic_mean=True (the mean coefficients are integrated out of theta)");
  for (int i : ids)
    if (eng.gp[i].nug_type == NUG_PIVOT)
      throw std::runtime_error("predict_mixture: not available with nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
  if (!thetas || (m > 0 && !Xs)) throw std::runtime_error("predict_mixture: null input buffer");
  if ((weights != nullptr) == (log_q != nullptr)) throw std::runtime_error("predict_mixture: exactly one of weights and log_q must be given");
  if (!mean_out || !within_out || !between_out || !weights_out || !logpost_out || !ok_out) throw std::runtime_error("predict_mixture: null result buffer");
  if (m < 0 || max_slots < 0 || max_points < 0) throw std::runtime_error("predict_mixture: m, max_slots and max_points must not be negative");
  if (E * (long)S > (1L << 30)) throw std::runtime_error("predict_mixture: too many (emulator, sample) pairs");
  for (long e = 0; e < E; ++e) {
    const int P = eng.n_theta(ids[e]);
    if (P > ld) throw std::runtime_error("Shape of new GPParams object does not match existing one");
    for (int s = 0; s < S; ++s) {
      const double* th = thetas + ((size_t)e * S + s) * ld;
      require_finite(th, (size_t)P, "predict_mixture: the hyperparameter samples must be finite");
      const double x = weights ? weights[e * S + s] : log_q[e * S + s];
      if (!std::isfinite(x)) throw std::runtime_error(weights ? "predict_mixture: the weights must be finite" : "predict_mixture: log_q must be finite");
      if (weights && x < 0.) throw std::runtime_error("predict_mixture: the weights must not be negative");
    }
  }
  require_finite(Xs, (size_t)m * eng.D, "predict_mixture: the query points must be finite");
}

}  // namespace

void Engine::predict_mixture(const std::vector<int>& ids, const double* thetas, int S, int ld, const double* weights, const double* log_q,
                             const double* Xs, int m, bool include_nugget, int max_slots, int max_points, double* mean_out,
                             double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out, int* ok_all) {
  const long E = (long)ids.size();
  if (E == 0) return;
  check_mixture_args(*this, ids, thetas, S, ld, weights, log_q, Xs, m, max_slots, max_points, mean_out, within_out, between_out, weights_out,
                     logpost_out, ok_out);

  // plan.  slots: what fits beside this engine and what pays (fit_map_from's rule); points: predict()'s chunk rule on the smaller budget
  const long pairs = E * S;
  long device_slots = pairs;
  double cap = ks_budget_bytes(), free_b = 0.;
  if (free_device_bytes(free_b)) {
    device_slots = slots_in_half_of(free_b, replica_slot_bytes(MS, LD));
    cap = std::min(cap, 0.25 * free_b);
  }
  device_slots = std::min<long>(device_slots, std::max<long>(E, replica_slot_bound(NP, TILE)));
  const MixturePlan plan = mixture_plan(E, S, LD, device_slots, m, max_slots, max_points, cap);
  const long slots = plan.slots, ngroups = (pairs + slots - 1) / slots;
  const int MC = plan.points;
  if (slots > 65535) throw std::runtime_error("predict_mixture: more than 65535 slots per pass are not supported");

  // lease
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
    const MixturePassTables t = mixture_pass_tables(p0, cnt, S, okv.data(), w.data(), nug.data(), include_nugget, alive.data(), pivot_pair.data());
    if (t.okslots.empty()) continue;
    if (ngroups > 1) {
      // the slots hold the last pass of step 1: factor this pass again.  What step 2 was computed from must be what is predicted from.
      // (Also where the pass is then skipped for an empty etab: the tables depend on step 1 alone.)
      const std::vector<double> F1(F.begin() + p0, F.begin() + p0 + cnt);
      const std::vector<int> ok1(okv.begin() + p0, okv.begin() + p0 + cnt);
      factor_group(g);
      for (long k = 0; k < cnt; ++k)
        if (okv[p0 + k] != ok1[k] || (ok1[k] && F[p0 + k] != F1[k]))
          throw std::runtime_error("predict_mixture: a sample did not factorise to the same bits twice");
    }
    if (t.etab.empty()) continue;
    HIPCK(hipMemcpyAsync(dTab, t.etab.data(), t.etab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dRows, t.rows.data(), t.rows.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dPrm, t.prm.data(), t.prm.size() * sizeof(double), hipMemcpyHostToDevice, st));
    for (int c0 = 0; c0 < m; c0 += MC) {
      const int mc = std::min(MC, m - c0);
      rep->predict(t.okslots, dXq + (size_t)c0 * D, mc, true, dMu, dVa, MC, true, nullptr);
      launch_mixture_accumulate(dMu, dVa, MC, mc, (int)(t.etab.size() / 4), dTab, dRows, dPrm, dAcc, dPivot, m, c0, st);
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

void Engine::require_plain_fit(const char* who, const std::vector<int>& ids, const char* analytic_reason) const {
  const std::string p = std::string(who) + ": not available with ";
  require_factored(ids);
  if (analytic) throw std::runtime_error(p + "analytic_mean=True (" + analytic_reason + ")");
  for (int i : ids)
    if (gp[i].nug_type == NUG_PIVOT || gp[i].permuted) throw std::runtime_error(p + "nugget=\"pivot\" (a pivoted, possibly rank-deficient factor)");
}

// ---------------------------------------------------------------------------------------------
// Cross-validation at the fitted hyperparameters (engine.h has the contract, kernels_cv.hip the formulas and the kernels).
//   every fold a single point: L^-1 and ONE launch of cv_loo_kernel (cv_leave_one_out);
//   otherwise K^-1, then the (emulator, fold) pairs in passes of `slots` (cv_plan) through a ScratchFactor of nsub = the largest fold size
//   rows: per pass its factor with cv_gather_kernel as the fill, the log-determinant and L^-T y launchers on the slots that factorised
//   (logdet_and_solve), cv_finish_kernel; ONE download at the end (cv_kfold).
// The ScratchFactor and every buffer here are scratch of the call.
// ---------------------------------------------------------------------------------------------

// what both paths share: the observations and nuggets of the rows of E emulators and the result buffers (n points, k folds)
struct CvBuffers {
  std::vector<double> traw, eta;
  size_t En, Ek;
  DevBuf<double> dTraw, dEta, dMeanO, dVarO, dMaha, dLs;
  DevBuf<int> dOk;
  CvBuffers(size_t E, size_t n, size_t k)
      : traw(E * n), eta(E), En(E * n), Ek(E * k), dTraw(traw.size()), dEta(eta.size()), dMeanO(En), dVarO(En), dMaha(Ek), dLs(Ek), dOk(Ek) {}
  // inputs up, results preset to NaN / not ok
  void stage(hipStream_t st) {
    HIPCK(hipMemcpyAsync(dTraw, traw.data(), traw.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(dEta, eta.data(), eta.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(dMeanO, 0xFF, En * sizeof(double), st));
    HIPCK(hipMemsetAsync(dVarO, 0xFF, En * sizeof(double), st));
    HIPCK(hipMemsetAsync(dMaha, 0xFF, Ek * sizeof(double), st));
    HIPCK(hipMemsetAsync(dLs, 0xFF, Ek * sizeof(double), st));
    HIPCK(hipMemsetAsync(dOk, 0, Ek * sizeof(int), st));
  }
  void download(hipStream_t st, double* mean_out, double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
    HIPCK(hipMemcpyAsync(mean_out, dMeanO, En * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(var_out, dVarO, En * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(maha_out, dMaha, Ek * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(log_score_out, dLs, Ek * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(ok_out, dOk, Ek * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
  }
};

// leave-one-out: L^-1 only
void Engine::cv_leave_one_out(const std::vector<int>& ids, const int* labels, bool include_nugget, CvBuffers& b, double* mean_out, double* var_out,
                              double* maha_out, double* log_score_out, int* ok_out) {
  const size_t nn = (size_t)n;
  DevBuf<int> dLab(nn);
  SyncOnUnwind drained{stream};
  ensure_alpha(ids);
  ensure_linv(ids);
  upload_idx(ids);
  b.stage(stream);
  HIPCK(hipMemcpyAsync(dLab, labels, nn * sizeof(int), hipMemcpyHostToDevice, stream));
  launch_cv_loo(view((int)ids.size()), dLab, b.dTraw, b.dEta, include_nugget, b.dMeanO, b.dVarO, b.dMaha, b.dLs, b.dOk, stream);
  b.download(stream, mean_out, var_out, maha_out, log_score_out, ok_out);
}

// k folds: K^-1, then the (emulator, fold) pairs in passes through a ScratchFactor of the call
void Engine::cv_kfold(const std::vector<int>& ids, const CvFolds& cf, int k, bool include_nugget, int max_slots, CvBuffers& b, double* mean_out,
                      double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  const long E = (long)ids.size();
  const int nsub = cf.nsub, NPsub = (int)scratch_np(nsub);
  const long pairs = E * k;
  long device_slots = pairs;
  double free_b = 0.;
  if (free_device_bytes(free_b)) device_slots = slots_in_half_of(free_b, cv_slot_bytes(NPsub));
  const long slots = cv_plan(E, k, NPsub, device_slots, max_slots);

  ensure_alpha(ids);
  ensure_kinv(ids, false);
  HIPCK(hipStreamSynchronize(stream));        // the ScratchFactor reads K^-1 and alpha on its own stream
  const BatchView src = view(0);
  ScratchFactor sub(nsub, slots);
  hipStream_t st = sub.stream();
  DevBuf<int> dFolds(cf.folds.size()), dTab(4 * (size_t)slots);
  SyncOnUnwind drained{st};
  b.stage(st);
  HIPCK(hipMemcpyAsync(dFolds, cf.folds.data(), cf.folds.size() * sizeof(int), hipMemcpyHostToDevice, st));
  std::vector<int> tab(4 * (size_t)slots), info, okslots;
  const CovFill fill = [&](const BatchView& sv) {
    if (sv.nb != (int)slots) throw std::runtime_error("cross_validate: the factorisation must cover every slot");
    launch_cv_gather(src, dFolds, dTab, (int)slots, sv.A, nsub, NPsub, st);
  };
  for (long p0 = 0; p0 < pairs; p0 += slots) {
    const long cnt = std::min(slots, pairs - p0);
    cv_pass_table(p0, cnt, slots, k, ids.data(), cf.size.data(), tab.data());
    HIPCK(hipMemcpyAsync(dTab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    sub.factor(fill, info);
    okslots.clear();
    for (long s = 0; s < cnt; ++s)
      if (info[s] == 0) okslots.push_back((int)s);
    sub.logdet_and_solve(okslots);
    launch_cv_finish(dFolds, dTab, (int)cnt, sub.linv(), sub.solution(), sub.logdet_words(), sub.status(), nsub, NPsub, b.dTraw, b.dEta,
                     include_nugget, n, k, b.dMeanO, b.dVarO, b.dMaha, b.dLs, b.dOk, st);
    HIPCK(hipStreamSynchronize(st));          // `tab` is rewritten by the next pass
  }
  b.download(st, mean_out, var_out, maha_out, log_score_out, ok_out);
}

void Engine::cross_validate(const std::vector<int>& ids, const int* labels, int k, bool include_nugget, int max_slots, double* mean_out,
                            double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  require_plain_fit("cross_validate", ids, "a held-out fold changes the mean coefficients");
  if (!labels || !mean_out || !var_out || !maha_out || !log_score_out || !ok_out) throw std::runtime_error("cross_validate: null buffer");
  if (k < 2 || k > n) throw std::runtime_error("cross_validate: the number of folds must be between 2 and the number of training points (k = " + std::to_string(k) + ", n = " + std::to_string(n) + ")");
  if (max_slots < 0) throw std::runtime_error("cross_validate: max_slots must not be negative");
  if (E * (long)k > (1L << 30)) throw std::runtime_error("cross_validate: too many (emulator, fold) pairs");
  const CvFolds cf = cv_folds(labels, n, k);

  CvBuffers b((size_t)E, (size_t)n, (size_t)k);
  for (long e = 0; e < E; ++e) {
    std::copy(hT.begin() + (size_t)ids[e] * n, hT.begin() + (size_t)(ids[e] + 1) * n, b.traw.begin() + (size_t)e * n);
    b.eta[e] = gp[ids[e]].nugget_used;
  }
  if (cf.nsub == 1) cv_leave_one_out(ids, labels, include_nugget, b, mean_out, var_out, maha_out, log_score_out, ok_out);
  else cv_kfold(ids, cf, k, include_nugget, max_slots, b, mean_out, var_out, maha_out, log_score_out, ok_out);
}

// ---------------------------------------------------------------------------------------------
// Joint posterior draws (engine.h has the contract, kernels_sample.hip the kernels, sample_plan of predict_plan.h the sizing).  Per pass of
// `slots` emulators:
//   1. sample_build: Sigma* and mu* with predict_full_cov's own launches; Sigma* stays on the device, mu* gets its mean-function terms on
//      the host and goes up again;
//   2. sample_factor: Sigma~ gathered into the ScratchFactor (sample_gather_kernel as the fill of its factor, L^-1 not formed), then
//      the jitter ladder on the host over the slots that failed -- they alone are gathered again, from the resident Sigma* --, then
//      sample_polish_kernel: the factor's diagonal from its finished rows with the correctly rounded square root;
//   3. sample_draws: per chunk of draws z uploaded or generated, z_out and Y = mu + L z downloaded; NaN rows where Sigma~ never factorised.
// The ScratchFactor and every buffer are scratch of the call.
// ---------------------------------------------------------------------------------------------

// the buffers of a pass, sized for `slots` emulators and `draws` draws per chunk; the guards come last, so that both streams are drained
// before the buffers go when the call is left through an exception
struct Engine::SamplePass {
  int m, MP;
  long slots, zrows;
  DevBuf<double> dC, dDots, dMu, dShift, dZ, dY;
  DevBuf<int> dSrc;
  DevBuf<unsigned> dStreams;
  std::vector<int> good;             // per slot of the pass: Sigma~ factorised
  SyncOnUnwind drained_main, drained_sub;
  SamplePass(int m_, long slots_, long draws, int R, hipStream_t main_stream, hipStream_t sub_stream)
      : m(m_), MP((int)sample_mp(m_)), slots(slots_), zrows(sample_draw_rows(draws)), dC((size_t)slots_ * m_ * m_), dDots((size_t)slots_ * R * m_),
        dMu((size_t)slots_ * m_), dShift((size_t)slots_), dZ((size_t)slots_ * zrows * MP), dY((size_t)slots_ * zrows * m_), dSrc((size_t)slots_),
        dStreams((size_t)slots_), good((size_t)slots_, 0), drained_main{main_stream}, drained_sub{sub_stream} {}
};

// 1. Sigma* (p.dC) and mu* (mean_out, p.dMu) of the emulators of grp
void Engine::sample_build(const std::vector<int>& grp, const double* Xs, const double* dXq, int m, SamplePass& p, double* mean_out) {
  const int nb = (int)grp.size();
  ensure_alpha(grp);
  ensure_linv(grp);
  upload_idx(grp);
  std::vector<double> dots((size_t)nb * R * m);
  {
    DevBuf<double> dKf((size_t)nb * p.MP * LD), dV((size_t)nb * NP * p.MP);
    SyncOnUnwind drained{stream};
    fullcov_launches(nb, dXq, m, p.MP, dKf, dV, p.dC, p.dDots);
    HIPCK(hipMemcpyAsync(dots.data(), p.dDots, dots.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));
    HIPCK(hipGetLastError());
  }
  fullcov_host_means(grp, Xs, m, dots.data(), mean_out, nullptr);
  HIPCK(hipMemcpyAsync(p.dMu, mean_out, (size_t)nb * m * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipStreamSynchronize(stream));        // the ScratchFactor reads Sigma* and mu* on its own stream
}

// 2. Sigma~ = L L^T in the slots 0 .. grp.size() - 1 of the ScratchFactor, the ladder over those that fail
void Engine::sample_factor(ScratchFactor& sub, const std::vector<int>& grp, bool include_nugget, double jitter, SamplePass& p, double* jitter_used,
                           int* ok) {
  const long cnt = (long)grp.size();
  const int m = p.m;
  hipStream_t st = sub.stream();
  std::vector<int> src((size_t)p.slots, -1), list((size_t)cnt), info;
  std::vector<double> shift((size_t)p.slots, 0.), nug((size_t)cnt), diag((size_t)m);
  for (long k = 0; k < cnt; ++k) {
    src[k] = list[k] = (int)k;
    nug[k] = include_nugget ? nugget_size(grp[k]) : 0.;
    shift[k] = nug[k] + jitter;
    jitter_used[k] = jitter;
  }
  HIPCK(hipMemcpyAsync(p.dSrc, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, st));
  const CovFill fill = [&](const BatchView& sv) {
    HIPCK(hipMemcpyAsync(p.dShift, shift.data(), shift.size() * sizeof(double), hipMemcpyHostToDevice, st));
    launch_sample_gather(sv, p.dC, p.dSrc, p.dShift, m, st);
  };
  auto failed_of = [&](const std::vector<int>& tried) {
    std::vector<int> f;
    for (int k : tried)
      if (info[k] != 0) f.push_back(k);
    return f;
  };
  sub.factor(fill, info, &list, false);
  std::vector<int> failed = failed_of(list);
  std::vector<double> mean_diag((size_t)cnt, 0.);
  for (int t = 0; t < SAMPLE_LADDER_RUNGS && !failed.empty(); ++t) {
    for (int k : failed) {
      if (t == 0) {       // the mean diagonal of Sigma*, read when the ladder first needs it
        HIPCK(hipMemcpy2D(diag.data(), sizeof(double), p.dC + (size_t)k * m * m, ((size_t)m + 1) * sizeof(double), sizeof(double), (size_t)m,
                          hipMemcpyDeviceToHost));
        double s = 0.;
        for (int j = 0; j < m; ++j) s += diag[j];
        mean_diag[k] = s / m;
      }
      const double delta = sample_ladder_delta(t, mean_diag[k]);
      jitter_used[k] = jitter + delta;
      shift[k] = nug[k] + jitter_used[k];
    }
    sub.factor(fill, info, &failed, false);
    failed = failed_of(failed);
  }
  // (src and shift on the device are those of every slot's last gather; a slot that never factorised is left alone by the kernel's test)
  launch_sample_polish(sub.factor_buffer(), sub.NP, (int)cnt, p.dC, p.dSrc, p.dShift, m, st);
  for (long k = 0; k < cnt; ++k) p.good[k] = 1;
  for (int k : failed) p.good[k] = 0;
  for (long k = 0; k < cnt; ++k) ok[k] = p.good[k];
}

// 3. the draws of the emulators [e0, e0 + cnt) of the call (slots 0 .. cnt - 1), chunk by chunk
void Engine::sample_draws(ScratchFactor& sub, long e0, long cnt, int m, int S, int Sc, unsigned long long seed, const double* z_in, bool z_per_emulator,
                          SamplePass& p, double* samples, double* z_out) {
  hipStream_t st = sub.stream();
  const size_t row = (size_t)m * sizeof(double), zpitch = (size_t)p.MP * sizeof(double), mm = (size_t)m;
  for (int s0 = 0; s0 < S; s0 += Sc) {
    const int sc = std::min(Sc, S - s0);
    if (z_in) {
      for (long k = 0; k < cnt; ++k) {
        const double* zsrc = z_in + ((z_per_emulator ? (size_t)(e0 + k) * S : 0) + s0) * mm;
        HIPCK(hipMemcpy2DAsync(p.dZ + (size_t)k * p.zrows * p.MP, zpitch, zsrc, row, row, sc, hipMemcpyHostToDevice, st));
      }
    } else {
      launch_sample_normals(p.dZ, (int)cnt, p.zrows, p.MP, m, sc, s0, seed, p.dStreams, st);
    }
    launch_sample_apply(sub.factor_buffer(), sub.NP, p.dZ, p.zrows, p.MP, p.dMu, m, sc, (int)cnt, p.dY, p.zrows, st);
    for (long k = 0; k < cnt; ++k) {
      const size_t o = ((size_t)(e0 + k) * S + s0) * mm;
      if (z_out) HIPCK(hipMemcpy2DAsync(z_out + o, row, p.dZ + (size_t)k * p.zrows * p.MP, zpitch, row, sc, hipMemcpyDeviceToHost, st));
      HIPCK(hipMemcpyAsync(samples + o, p.dY + (size_t)k * p.zrows * mm, (size_t)sc * row, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipStreamSynchronize(st));          // the next chunk overwrites Z and Y
    HIPCK(hipGetLastError());
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (long k = 0; k < cnt; ++k)
    if (!p.good[k]) std::fill(samples + (size_t)(e0 + k) * S * mm, samples + (size_t)(e0 + k + 1) * S * mm, nan);
}

void Engine::sample_posterior(const std::vector<int>& ids, const unsigned* streams, const double* Xs, int m, int S, unsigned long long seed,
                              const double* z_in, bool z_per_emulator, bool include_nugget, double jitter, int max_slots, int max_draws,
                              double* samples, double* mean_out, double* z_out, double* jitter_used, int* ok) {
  const long E = (long)ids.size();
  if (E == 0) return;
  require_plain_fit("sample_posterior", ids, "its covariance term is finished on the host");
  if (!streams || !Xs || !samples || !mean_out || !jitter_used || !ok) throw std::runtime_error("sample_posterior: null buffer");
  if (m < 1) throw std::runtime_error("sample_posterior: at least one query point is needed");
  if (S < 1) throw std::runtime_error("sample_posterior: at least one draw is needed (n_draws = " + std::to_string(S) + ")");
  if (!(jitter >= 0.) || !std::isfinite(jitter)) throw std::runtime_error("sample_posterior: jitter must be a finite number that is not negative");
  if (max_slots < 0 || max_draws < 0) throw std::runtime_error("sample_posterior: max_slots and max_draws must not be negative");
  require_finite(Xs, (size_t)m * D, "sample_posterior: the query points must be finite");
  if (z_in) require_finite(z_in, (size_t)(z_per_emulator ? E : 1) * S * m, "sample_posterior: z must be finite");

  const SamplePlan plan = sample_plan(E, m, S, LD, NP, R, free_bytes_or_twice_budget(), max_slots, max_draws);
  const long slots = plan.slots;
  const int Sc = (int)plan.draws;

  ScratchFactor sub(m, slots);
  DevBuf<double> dXq((size_t)m * D);
  SamplePass p(m, slots, Sc, R, stream, sub.stream());
  HIPCK(hipMemcpyAsync(dXq, Xs, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCK(hipMemsetAsync(p.dZ, 0, (size_t)slots * p.zrows * p.MP * sizeof(double), sub.stream()));      // columns >= m and rows >= Sc: exact zeros
  for (long e0 = 0; e0 < E; e0 += slots) {
    const long cnt = std::min(slots, E - e0);
    const std::vector<int> grp(ids.begin() + e0, ids.begin() + e0 + cnt);
    sample_build(grp, Xs, dXq, m, p, mean_out + (size_t)e0 * m);
    HIPCK(hipMemcpyAsync(p.dStreams, streams + e0, (size_t)cnt * sizeof(unsigned), hipMemcpyHostToDevice, sub.stream()));
    sample_factor(sub, grp, include_nugget, jitter, p, jitter_used + e0, ok + e0);
    sample_draws(sub, e0, cnt, m, S, Sc, seed, z_in, z_per_emulator, p, samples, z_out);
  }
}

// ---------------------------------------------------------------------------------------------
// Active learning (engine.h has the contracts, kernels_alc.hip the kernels, alc_plan of predict_plan.h the sizing).
//   alc:  1. refusals   2. the factor and L^-1   3. alc_plan   4. per group of emulators: the candidates once -- K*, s^2 and V_c with
//         predict()'s own launches --, then per chunk of reference points K*, s^2, V_r and alc_cross into the per-tile partials, then
//         alc_finish   5. one download per group.
//   predict_cov: the same with the store epilogue and no reduction.
// Every device allocation is a DevBuf local of the call.
// ---------------------------------------------------------------------------------------------

void Engine::check_cov_args(const char* who, const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_a,
                            int max_b) const {
  const std::string p = std::string(who) + ": ";
  require_plain_fit(who, ids, "the covariance gains a term of the mean coefficients");
  if (!X1 || !X2) throw std::runtime_error(p + "null buffer");
  if (m1 < 1 || m2 < 1) throw std::runtime_error(p + "at least one point is needed in each set");
  if (max_a < 0 || max_b < 0) throw std::runtime_error(p + "max_slots and max_points must not be negative");
  require_finite(X1, (size_t)m1 * D, (p + "the points must be finite").c_str());
  if (X2 != X1) require_finite(X2, (size_t)m2 * D, (p + "the points must be finite").c_str());
}

void Engine::points_v(int nb, const double* dXq, int m, int MP, double* dK, double* dDots, double* dPartial, double* dVar, int var_ld, double* dV) {
  const BatchView v = view(nb);
  // (the dot products of the fused mean are not used: alpha need not be there)
  launch_cross_cov_mean(v, dXq, m, MP, dK, dDots, MP, stream);
  if (dVar) launch_predict_var(v, dK, m, MP, dPartial, dVar, var_ld, n_cu, stream);
  launch_predict_v_store(v, dK, m, MP, dV, stream);
}

void Engine::predict_cov(const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_slots, double* out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  const bool same = X2 == nullptr;
  if (same) { X2 = X1; m2 = m1; }
  check_cov_args("predict_cov", ids, X1, m1, X2, m2, max_slots, 0);
  if (!out) throw std::runtime_error("predict_cov: null buffer");
  ensure_linv(ids);
  const double per = predict_cov_rule_bytes(m1, m2, LD, NP);
  if (per > 64.0e9)
    throw std::runtime_error("predict_cov: " + std::to_string(m1) + " x " + std::to_string(m2) +
                             " points need more than 64 GB of device scratch; use fewer points per call");
  const double free_b = free_bytes_or_twice_budget();
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
    upload_idx(grp);
    points_v(cnt, dX1, m1, MP1, dK, dDots, nullptr, nullptr, 0, dV1);
    if (!same) points_v(cnt, dX2, m2, MP2, dK, dDots, nullptr, nullptr, 0, dV2);
    launch_alc_store(view(cnt), dV1, MP1, m1, dX1, same ? dV1.get() : dV2.get(), MP2, m2, same ? dX1.get() : dX2.get(), dC, stream);
    HIPCK(hipMemcpyAsync(out + (size_t)e0 * mm, dC, (size_t)cnt * mm * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCK(hipStreamSynchronize(stream));        // the next group overwrites the buffers
    HIPCK(hipGetLastError());
  }
}

void Engine::alc(const std::vector<int>& ids, const double* Xc, int mc, const double* Xr, int mr, const double* w, const double* noise,
                 int max_slots, int max_points, double* reduction, double* cand_var, double* ref_var, int* degenerate) {
  const long E = (long)ids.size();
  if (E == 0) return;
  // 1. refusals
  check_cov_args("alc_criterion", ids, Xc, mc, Xr, mr, max_slots, max_points);
  if (!w || !reduction || !cand_var || !ref_var || !degenerate) throw std::runtime_error("alc_criterion: null buffer");
  double wsum = 0.;
  for (int j = 0; j < mr; ++j) {
    if (!std::isfinite(w[j])) throw std::runtime_error("alc_criterion: the weights must be finite");
    if (w[j] < 0.) throw std::runtime_error("alc_criterion: the weights must not be negative");
    wsum += w[j];
  }
  if (!(wsum > 0.)) throw std::runtime_error("alc_criterion: the weights must not sum to 0");
  std::vector<double> tau((size_t)E);
  for (long e = 0; e < E; ++e) {
    tau[e] = noise ? noise[e] : nugget_size(ids[e]);
    if (!(tau[e] >= 0.) || !std::isfinite(tau[e])) throw std::runtime_error("alc_criterion: noise must be a finite number that is not negative");
  }
  // 2. the factor is there (check_cov_args); L^-1
  ensure_linv(ids);
  // 3. plan
  const AlcPlan plan = alc_plan(E, mc, mr, LD, NP, free_bytes_or_twice_budget(), max_slots, max_points);
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
    upload_idx(grp);
    const BatchView v = view(cnt);
    HIPCK(hipMemcpyAsync(dTau, tau.data() + e0, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, stream));
    points_v(cnt, dXc, mc, MPc, dK, dDots, dPartial, dVarC, mc, dVc);
    for (int c0 = 0; c0 < mr; c0 += CH) {
      const int mrc = std::min(CH, mr - c0), MPr = (int)alc_mp(mrc);
      points_v(cnt, dXr + (size_t)c0 * D, mrc, MPr, dK, dDots, dPartial, dVarR + c0, mr, dVr);
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
// Greedy ALC batches (engine.h has the contract, alc_batch_plan of predict_plan.h the sizing).
//   AlcBatch():  V and s^2 of both sets with predict()'s own launches, V copied behind one another into buffers of n16 + ext rows per slot
//   scores(t):   alc_cross over the K range [0, n16 + roundup(t, 16)) -- rows not yet written are 0 --, alc_finish with the floor of n + t
//   apply(t, .): the pick on the device, then the row n16 + t of both sets and their s^2
//   finish():    the one download of a group
// ---------------------------------------------------------------------------------------------

void Engine::alc_batch_check(const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
                             const double* noise, int q, int max_slots, std::vector<double>& tau) const {
  check_cov_args("alc_batch", ids, X, M, Xr, mr, max_slots, 0);
  if (!w) throw std::runtime_error("alc_batch: null buffer");
  if (forced < 0 || forced > M) throw std::runtime_error("alc_batch: the pending points are a prefix of the candidates");
  if (q < 1) throw std::runtime_error("alc_batch: n_points must be at least 1");
  if (q > M - forced) throw std::runtime_error("alc_batch: n_points must not exceed the number of candidates");
  double wsum = 0.;
  for (int j = 0; j < mr; ++j) {
    if (!std::isfinite(w[j])) throw std::runtime_error("alc_batch: the weights must be finite");
    if (w[j] < 0.) throw std::runtime_error("alc_batch: the weights must not be negative");
    wsum += w[j];
  }
  if (!(wsum > 0.)) throw std::runtime_error("alc_batch: the weights must not sum to 0");
  tau.resize(ids.size());
  for (size_t e = 0; e < ids.size(); ++e) {
    tau[e] = noise ? noise[e] : nugget_size(ids[e]);
    if (!(tau[e] >= 0.) || !std::isfinite(tau[e])) throw std::runtime_error("alc_batch: noise must be a finite number that is not negative");
  }
}

long Engine::alc_batch_slots(long E, int M, int mr, int T, int max_slots, bool total) const {
  return alc_batch_plan(E, M, mr, T, LD, NP, free_bytes_or_twice_budget(), max_slots, total);
}

Engine::AlcBatch::AlcBatch(Engine& eng, const std::vector<int>& grp, const double* tau, const double* X, int M_, int forced, const double* Xr,
                           int mr_, const double* w, int q, const AlcBatchOut& out)
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
  e.points_v(cnt, dXc, M, MPc, dK, dDots, dPartial, dVarC, M, dV);
  widen(dVc, MPc);
  e.points_v(cnt, dXr, mr, MPr, dK, dDots, dPartial, dVarR, mr, dV);
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

void Engine::AlcBatch::scores(int t) {
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

void Engine::AlcBatch::scores_to_host(int t, double* row_red, int* row_deg) {
  scores(t);
  HIPCK(hipMemcpyAsync(row_red, dRed, (size_t)cnt * M * sizeof(double), hipMemcpyDeviceToHost, e.stream));
  HIPCK(hipMemcpyAsync(row_deg, dDeg, (size_t)cnt * M * sizeof(int), hipMemcpyDeviceToHost, e.stream));
  HIPCK(hipStreamSynchronize(e.stream));
  HIPCK(hipGetLastError());
}

void Engine::AlcBatch::apply(int t, int forced) {
  hipStream_t st = e.stream;
  e.upload_idx(ids);
  const BatchView v = e.view(cnt);
  launch_alc_argmax(v, t, T, forced, M, dRed, dVarC, M, dTau, dMask, dPicks, dPickRed, dPickD, st);
  launch_alc_condition(v, t, T, rows, dPicks, dPickD, dVc, MPc, dXc, dVc, MPc, M, dXc, dVarC, M, st);
  launch_alc_condition(v, t, T, rows, dPicks, dPickD, dVc, MPc, dXc, dVr, MPr, mr, dXr, dVarR, mr, st);
}

void Engine::AlcBatch::finish() {
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

void Engine::alc_batch(const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
                       const double* noise, int q, int max_slots, const AlcBatchOut& out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  std::vector<double> tau;
  alc_batch_check(ids, X, M, forced, Xr, mr, w, noise, q, max_slots, tau);
  if (!out.picks || !out.pick_red || !out.cand_var || !out.ref_var || !out.ref_var_after || !out.iv) throw std::runtime_error("alc_batch: null buffer");
  const int T = forced + q;
  const long slots = alc_batch_slots(E, M, mr, T, max_slots, false);
  for (long e0 = 0; e0 < E; e0 += slots) {
    const long cnt = std::min(slots, E - e0);
    const std::vector<int> grp(ids.begin() + e0, ids.begin() + e0 + cnt);
    AlcBatch run(*this, grp, tau.data() + e0, X, M, forced, Xr, mr, w, q, out.rows_from((size_t)e0, T, M, mr));
    SyncOnUnwind drained{stream};
    for (int t = 0; t < T; ++t) {
      run.scores(t);
      run.apply(t, t < forced ? t : -1);
    }
    run.finish();
  }
}

}  // namespace mogp
