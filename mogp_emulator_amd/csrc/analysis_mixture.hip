// Prediction averaged over hyperparameter samples (analysis.h has the contract, kernels_mixture.hip the reduction).
//   1. every (emulator, sample) pair is factored on a replica engine, `slots` pairs per pass: F, ok and the nugget used per pair;
//   2. the weights, on the host (mixture_weights);
//   3. per pass and chunk of points the batched mean + variance prediction of the pass's slots, then mixture_accumulate into the
//      (E, 3, m) sums; with more than one pass the slots were overwritten in step 1, so a pass is factored again first (the same bits);
//   4. mixture_finalise and ONE download.
#include "analysis.h"
#include "engine_internal.h"

#include <cmath>
#include <limits>

namespace mogp {

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

void predict_mixture(Engine& eng, const std::vector<int>& ids, const double* thetas, int S, int ld, const double* weights, const double* log_q,
                     const double* Xs, int m, bool include_nugget, int max_slots, int max_points, double* mean_out, double* within_out,
                     double* between_out, double* weights_out, double* logpost_out, int* ok_out, int* ok_all) {
  const long E = (long)ids.size();
  if (E == 0) return;
  const int n = eng.n, D = eng.D, NP = eng.NP, LD = eng.LD;
  check_mixture_args(eng, ids, thetas, S, ld, weights, log_q, Xs, m, max_slots, max_points, mean_out, within_out, between_out, weights_out,
                     logpost_out, ok_out);

  // plan.  slots: what fits beside this engine and what pays (fit_map_from's rule); points: predict()'s chunk rule on the smaller budget
  const long pairs = E * S;
  long device_slots = pairs;
  double cap = ks_budget_bytes(), free_b = 0.;
  if (eng.free_device_bytes(free_b)) {
    device_slots = slots_in_half_of(free_b, replica_slot_bytes(eng.MS, LD));
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
    std::copy(eng.hT.begin() + (size_t)i * n, eng.hT.begin() + (size_t)(i + 1) * n, targets.begin() + (size_t)k * n);
  }
  ReplicaLease rep(eng, slots, targets, eng.gp[ids[0]].nug_type, eng.gp[ids[0]].nug_size);
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
        rep->retarget((int)k, eng, ids[e]);
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

}  // namespace mogp
