// The exact log-likelihood of a large design on the LocalGP handle (engine.h; DESIGN.md section 3 "Iterative exact likelihood"): the pieces of
//   log p(y) = -1/2 y^T alpha - 1/2 log|A| - N/2 log 2 pi   and of   d/dtheta_q = 1/2 alpha^T dA_q alpha - 1/2 tr(A^-1 dA_q)
// from ONE run of engine_iter.hip's conjugate gradients on the panel [y | z_1 .. z_T], z_t ~ N(0, P) with P the solver's preconditioner:
// the step coefficients of column t are the Lanczos matrix whose quadrature estimates tr log(P^-1/2 A P^-1/2) (stochastic Lanczos quadrature
// in its CG form, Gardner et al. 2018), and u_t^T dA_q w_t with u_t = A^-1 z_t, w_t = P^-1 z_t estimates tr(A^-1 dA_q) because E[z z^T] = P.
// The host reads scalars and the coefficient log; the quadrature itself is the caller's (IterativeGP.py).  Steps: the refusals and the plan
// (predict_plan.h), the preconditioner, the probes, the solve, the dots, the sweep (kernels_iter.hip).
#include "engine_internal.h"

#include <algorithm>
#include <climits>

namespace mogp {

void LocalGP::loglik_exact(int e, int kt, const double* scale, double sigma2, double nugget, int rank, double rtol, int max_iter, const double* g1,
                           int g1_rows, const double* g2, int T, bool want_grad, double* scalars, int* stat_i, double* residual, double* rho,
                           double* uw, double* coef, double* forms, double* forms_each, double* z_out, double* x_out, double* w_out) {
  const char* who = "loglik_exact";
  if (!scale || !g2 || !scalars || !stat_i || !residual || !rho || !uw || !coef || (want_grad && !forms) || (g1_rows > 0 && !g1))
    throw std::runtime_error("loglik_exact: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("loglik_exact: emulator index out of range");
  local_check_kernel(who, kt);
  iter_check_hyper(who, D, scale, sigma2, nugget);
  iter_check_rank(who, N, rank);
  iter_check_solve(who, 1, rtol, max_iter);
  iter_lik_check_probes(who, T);
  if (forms_each && !want_grad) throw std::runtime_error("loglik_exact: the forms per probe need want_grad");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  IterKey k;
  k.kt = kt, k.rank = rank, k.sigma2 = sigma2, k.nugget = nugget;
  k.scale.assign(scale, scale + D);
  iter_reserve(who, rank);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  double held = 0.;
  for (const DevBuf<double>* b : {&lkW, &lkLog, &lkG1, &lkPart, &lkOut}) held += 8.0 * (double)b->size();
  iter_lik_check_memory(who, N, D, rank, max_iter, (double)free_b, held);
  const int C = 1 + T;
  const size_t n = (size_t)N, panel = n * ITER_COLS, nblk = (n + 63) / 64, nlog = (size_t)2 * ITER_COLS * max_iter;
  lkW.reserve(panel);
  lkLog.reserve(nlog);
  lkG1.reserve((size_t)ITER_COLS * std::max(rank, 1));
  lkPart.reserve(nblk * 2 * D);
  lkOut.reserve((size_t)ITER_COLS * 2 * D);
  SyncOnUnwind sync{st};
  iter_build(k, st);
  if (g1_rows != itRank)
    throw std::runtime_error("loglik_exact: g1 must have as many rows as the rank the preconditioner reaches, " + std::to_string(itRank));
  const size_t panel_bytes = panel * sizeof(double);
  // the panel [y | g2], then the probes in place
  std::vector<double> hb(panel, 0.0);
  for (size_t i = 0; i < n; ++i)
    for (int t = 0; t < T; ++t) hb[(size_t)(1 + t) * n + i] = g2[i * T + t];
  HIPCK(hipMemcpyAsync(itB, hb.data(), panel_bytes, hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(itB, dY.get() + (size_t)e * n, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (itRank > 0) {
    std::vector<double> hg((size_t)ITER_COLS * itRank, 0.0);
    for (int s = 0; s < itRank; ++s)
      for (int t = 0; t < T; ++t) hg[(size_t)s * ITER_COLS + 1 + t] = g1[(size_t)s * T + t];
    HIPCK(hipMemcpyAsync(lkG1, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  // (at rank 0 the solver's preconditioner is the identity: P = I and z = g2)
  launch_probes(itL, N, itRank, lkG1, itRank > 0 ? std::sqrt(nugget) : 1.0, 1, C, itB, st);
  HIPCK(hipMemsetAsync(lkLog, 0, nlog * sizeof(double), st));
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  iter_cg(C, rtol, max_iter, it, cv, rs, st, lkW, lkLog);
  // the dots: rho_t = z_t^T w_t; then alpha takes column 0 of W, so that u^T w holds alpha^T alpha there; y^T alpha
  double d_rho[ITER_COLS], d_uw[ITER_COLS], d_ya[ITER_COLS];
  auto dots = [&](const double* a, const double* b, double* out) {
    launch_cg_dot(a, b, N, itPart, st);
    launch_cg_scalars(5, itPart, N, itSc, itFl, 0, rtol, st);
    HIPCK(hipMemcpyAsync(out, itSc.get() + 4 * ITER_COLS, ITER_COLS * sizeof(double), hipMemcpyDeviceToHost, st));
  };
  dots(itB, lkW, d_rho);
  HIPCK(hipMemcpyAsync(lkW, itX, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  dots(itX, lkW, d_uw);
  dots(itB, itX, d_ya);
  HIPCK(hipGetLastError());
  std::vector<double> hlog(nlog);
  HIPCK(hipMemcpyAsync(hlog.data(), lkLog, nlog * sizeof(double), hipMemcpyDeviceToHost, st));
  // alpha of this emulator, kept as predict_exact keeps it: a column's bits do not depend on the columns it shares a panel with
  IterKey ak = k;
  ak.rtol = rtol, ak.max_iter = max_iter;
  if (itAlpha.size() != (size_t)E) itAlpha.assign(E, IterAlpha());
  IterAlpha& a = itAlpha[e];
  a.key = IterKey();
  a.alpha.resize(n);
  HIPCK(hipMemcpyAsync(a.alpha.data(), itX, n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  a.iterations = it[0], a.converged = cv[0], a.residual = rs[0];
  a.key = ak;
  scalars[0] = d_ya[0], scalars[1] = d_uw[0], scalars[2] = itLogdetG, scalars[3] = (double)itRank;
  for (int c = 0; c < C; ++c) stat_i[2 * c] = it[c], stat_i[2 * c + 1] = cv[c], residual[c] = rs[c];
  for (int t = 0; t < T; ++t) rho[t] = d_rho[1 + t], uw[t] = d_uw[1 + t];
  for (int j = 0; j < max_iter; ++j)
    for (int q = 0; q < 2; ++q)
      for (int c = 0; c < C; ++c) coef[((size_t)j * 2 + q) * C + c] = hlog[((size_t)2 * j + q) * ITER_COLS + c];
  if (want_grad) {
    launch_kgrad_forms(dXs, N, D, kt, sigma2, itX, lkW, 1, C, lkPart, lkOut, st);
    if (forms_each)
      for (int t = 0; t < T; ++t) launch_kgrad_forms(dXs, N, D, kt, sigma2, itX, lkW, 1 + t, 2 + t, lkPart, lkOut.get() + (size_t)(1 + t) * 2 * D, st);
    HIPCK(hipGetLastError());
    std::vector<double> ho((size_t)C * 2 * D);
    HIPCK(hipMemcpyAsync(ho.data(), lkOut, (forms_each ? ho.size() : (size_t)2 * D) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    std::copy(ho.begin(), ho.begin() + 2 * D, forms);
    if (forms_each)
      for (int t = 0; t < T; ++t) std::copy(ho.begin() + (size_t)(1 + t) * 2 * D + D, ho.begin() + (size_t)(2 + t) * 2 * D, forms_each + (size_t)t * D);
  }
  if (z_out) {
    HIPCK(hipMemcpy(hb.data(), itB, panel_bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      for (int t = 0; t < T; ++t) z_out[i * T + t] = hb[(size_t)(1 + t) * n + i];
  }
  if (x_out) {
    HIPCK(hipMemcpy(hb.data(), itX, panel_bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      for (int c = 0; c < C; ++c) x_out[i * C + c] = hb[(size_t)c * n + i];
  }
  if (w_out) {
    HIPCK(hipMemcpy(hb.data(), lkW, panel_bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
      for (int c = 0; c < C; ++c) w_out[i * C + c] = hb[(size_t)c * n + i];
  }
}

}  // namespace mogp
