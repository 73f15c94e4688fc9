// Cross-validation at the fitted hyperparameters (analysis.h has the contract, kernels_cv.hip the formulas and the kernels).
//   every fold a single point: L^-1 and ONE launch of cv_loo_kernel (cv_leave_one_out);
//   otherwise K^-1, then the (emulator, fold) pairs in passes of `slots` (cv_plan) through a ScratchFactor of nsub = the largest fold size
//   rows: per pass its factor with cv_gather_kernel as the fill, the log-determinant and L^-T y launchers on the slots that factorised
//   (logdet_and_solve), cv_finish_kernel; ONE download at the end (cv_kfold).
// The ScratchFactor and every buffer here are scratch of the call.
#include "analysis.h"
#include "engine_internal.h"

namespace mogp {

namespace {

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
void cv_leave_one_out(Engine& eng, const std::vector<int>& ids, const int* labels, bool include_nugget, CvBuffers& b, double* mean_out,
                      double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  hipStream_t stream = eng.stream;
  const size_t nn = (size_t)eng.n;
  DevBuf<int> dLab(nn);
  SyncOnUnwind drained{stream};
  eng.ensure_alpha(ids);
  eng.ensure_linv(ids);
  eng.upload_idx(ids);
  b.stage(stream);
  HIPCK(hipMemcpyAsync(dLab, labels, nn * sizeof(int), hipMemcpyHostToDevice, stream));
  launch_cv_loo(eng.view((int)ids.size()), dLab, b.dTraw, b.dEta, include_nugget, b.dMeanO, b.dVarO, b.dMaha, b.dLs, b.dOk, stream);
  b.download(stream, mean_out, var_out, maha_out, log_score_out, ok_out);
}

// k folds: K^-1, then the (emulator, fold) pairs in passes through a ScratchFactor of the call
void cv_kfold(Engine& eng, const std::vector<int>& ids, const CvFolds& cf, int k, bool include_nugget, int max_slots, CvBuffers& b,
              double* mean_out, double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  const long E = (long)ids.size();
  const int nsub = cf.nsub, NPsub = (int)scratch_np(nsub);
  const long pairs = E * k;
  long device_slots = pairs;
  double free_b = 0.;
  if (eng.free_device_bytes(free_b)) device_slots = slots_in_half_of(free_b, cv_slot_bytes(NPsub));
  const long slots = cv_plan(E, k, NPsub, device_slots, max_slots);

  eng.ensure_alpha(ids);
  eng.ensure_kinv(ids, false);
  HIPCK(hipStreamSynchronize(eng.stream));        // the ScratchFactor reads K^-1 and alpha on its own stream
  const BatchView src = eng.view(0);
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
                     include_nugget, eng.n, k, b.dMeanO, b.dVarO, b.dMaha, b.dLs, b.dOk, st);
    HIPCK(hipStreamSynchronize(st));          // `tab` is rewritten by the next pass
  }
  b.download(st, mean_out, var_out, maha_out, log_score_out, ok_out);
}

}  // namespace

void cross_validate(Engine& eng, const std::vector<int>& ids, const int* labels, int k, bool include_nugget, int max_slots, double* mean_out,
                    double* var_out, double* maha_out, double* log_score_out, int* ok_out) {
  const long E = (long)ids.size();
  if (E == 0) return;
  const int n = eng.n;
  eng.require_plain_fit("cross_validate", ids, "a held-out fold changes the mean coefficients");
  if (!labels || !mean_out || !var_out || !maha_out || !log_score_out || !ok_out) throw std::runtime_error("cross_validate: null buffer");
  if (k < 2 || k > n) throw std::runtime_error("cross_validate: the number of folds must be between 2 and the number of training points (k = " + std::to_string(k) + ", n = " + std::to_string(n) + ")");
  if (max_slots < 0) throw std::runtime_error("cross_validate: max_slots must not be negative");
  if (E * (long)k > (1L << 30)) throw std::runtime_error("cross_validate: too many (emulator, fold) pairs");
  const CvFolds cf = cv_folds(labels, n, k);

  CvBuffers b((size_t)E, (size_t)n, (size_t)k);
  for (long e = 0; e < E; ++e) {
    std::copy(eng.hT.begin() + (size_t)ids[e] * n, eng.hT.begin() + (size_t)(ids[e] + 1) * n, b.traw.begin() + (size_t)e * n);
    b.eta[e] = eng.gp[ids[e]].nugget_used;
  }
  if (cf.nsub == 1) cv_leave_one_out(eng, ids, labels, include_nugget, b, mean_out, var_out, maha_out, log_score_out, ok_out);
  else cv_kfold(eng, ids, cf, k, include_nugget, max_slots, b, mean_out, var_out, maha_out, log_score_out, ok_out);
}

}  // namespace mogp
