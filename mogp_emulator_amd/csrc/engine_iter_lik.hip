// The exact log-likelihood of a large design on the LocalGP handle (engine.h; DESIGN.md section 3 "Iterative exact likelihood"): the pieces of
//   log p(y) = -1/2 y^T alpha - 1/2 log|A| - N/2 log 2 pi   and of   d/dtheta_q = 1/2 alpha^T dA_q alpha - 1/2 tr(A^-1 dA_q)
// from ONE run of the solver's (IterSolver, engine_iter.hip) conjugate gradients on the panel [y | z_1 .. z_T], z_t ~ N(0, P) with P the solver's preconditioner:
// the step coefficients of column t are the Lanczos matrix whose quadrature estimates tr log(P^-1/2 A P^-1/2) (stochastic Lanczos quadrature
// in its CG form, Gardner et al. 2018), and u_t^T dA_q w_t with u_t = A^-1 z_t, w_t = P^-1 z_t estimates tr(A^-1 dA_q) because E[z z^T] = P.
// The host reads scalars and the coefficient log; the quadrature itself is the caller's (IterativeGP.py).  Steps: the refusals and the plan
// (predict_plan.h), the preconditioner, the probes, the solve, the dots, the sweep (kernels_iter.hip).
#include "engine_internal.h"
#include "iter_panel.h"

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
  const IterKey k = make_key(kt, scale, D, sigma2, nugget, rank);
  iter.reserve(who, rank);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  IterSolver::LikScratch& lik = iter.lik;
  iter_lik_check_memory(who, N, D, rank, max_iter, (double)free_b, lik.bytes());
  const int C = 1 + T;
  const size_t n = (size_t)N, panel = n * ITER_COLS, nlog = (size_t)2 * ITER_COLS * max_iter;
  lik.reserve(N, D, rank, max_iter);
  SyncOnUnwind sync{st};
  precondition_for(k, st);
  const int reached = iter.pre.rank();
  if (g1_rows != reached)
    throw std::runtime_error("loglik_exact: g1 must have as many rows as the rank the preconditioner reaches, " + std::to_string(reached));
  IterSolver::CgPanels& cg = iter.cg;
  const size_t panel_bytes = panel * sizeof(double);
  // the panel [y | g2], then the probes in place
  std::vector<double> hb(panel, 0.0);
  rows_to_panel(g2, n, (size_t)T, 0, (size_t)T, hb.data(), n, 1);
  HIPCK(hipMemcpyAsync(cg.b, hb.data(), panel_bytes, hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(cg.b, dY.get() + (size_t)e * n, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (reached > 0) {
    std::vector<double> hg((size_t)ITER_COLS * reached, 0.0);
    for (int s = 0; s < reached; ++s)
      for (int t = 0; t < T; ++t) hg[(size_t)s * ITER_COLS + 1 + t] = g1[(size_t)s * T + t];
    HIPCK(hipMemcpyAsync(lik.g1, hg.data(), hg.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  // (at rank 0 the solver's preconditioner is the identity: P = I and z = g2)
  launch_probes(iter.pre.L, N, reached, lik.g1, reached > 0 ? std::sqrt(nugget) : 1.0, 1, C, cg.b, st);
  HIPCK(hipMemsetAsync(lik.log, 0, nlog * sizeof(double), st));
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  iter.solve(C, rtol, max_iter, it, cv, rs, st, lik.W, lik.log);
  // the dots: rho_t = z_t^T w_t; then alpha takes column 0 of W, so that u^T w holds alpha^T alpha there; y^T alpha
  double d_rho[ITER_COLS], d_uw[ITER_COLS], d_ya[ITER_COLS];
  iter.dots(cg.b, lik.W, d_rho, st);
  HIPCK(hipMemcpyAsync(lik.W, cg.x, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  iter.dots(cg.x, lik.W, d_uw, st);
  iter.dots(cg.b, cg.x, d_ya, st);
  std::vector<double> hlog(nlog);
  HIPCK(hipMemcpyAsync(hlog.data(), lik.log, nlog * sizeof(double), hipMemcpyDeviceToHost, st));
  // alpha of this emulator, kept as predict_exact keeps it: a column's bits do not depend on the columns it shares a panel with
  IterKey ak = k;
  ak.rtol = rtol, ak.max_iter = max_iter;
  iter.keep_alpha(e, ak, it[0], cv[0], rs[0], st);
  scalars[0] = d_ya[0], scalars[1] = d_uw[0], scalars[2] = iter.pre.logdetG(), scalars[3] = (double)reached;
  for (int c = 0; c < C; ++c) stat_i[2 * c] = it[c], stat_i[2 * c + 1] = cv[c], residual[c] = rs[c];
  for (int t = 0; t < T; ++t) rho[t] = d_rho[1 + t], uw[t] = d_uw[1 + t];
  for (int j = 0; j < max_iter; ++j)
    for (int q = 0; q < 2; ++q)
      for (int c = 0; c < C; ++c) coef[((size_t)j * 2 + q) * C + c] = hlog[((size_t)2 * j + q) * ITER_COLS + c];
  if (want_grad) {
    launch_kgrad_forms(dXs, N, D, kt, sigma2, cg.x, lik.W, 1, C, lik.part, lik.out, st);
    if (forms_each)
      for (int t = 0; t < T; ++t) launch_kgrad_forms(dXs, N, D, kt, sigma2, cg.x, lik.W, 1 + t, 2 + t, lik.part, lik.out.get() + (size_t)(1 + t) * 2 * D, st);
    HIPCK(hipGetLastError());
    std::vector<double> ho((size_t)C * 2 * D);
    HIPCK(hipMemcpyAsync(ho.data(), lik.out, (forms_each ? ho.size() : (size_t)2 * D) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    std::copy(ho.begin(), ho.begin() + 2 * D, forms);
    if (forms_each)
      for (int t = 0; t < T; ++t) std::copy(ho.begin() + (size_t)(1 + t) * 2 * D + D, ho.begin() + (size_t)(2 + t) * 2 * D, forms_each + (size_t)t * D);
  }
  // a panel back to the caller: the columns [pc0, pc0 + ncols) as a row-major (N, ncols) matrix
  auto download = [&](const double* dev, size_t pc0, size_t ncols, double* out) {
    HIPCK(hipMemcpy(hb.data(), dev, panel_bytes, hipMemcpyDeviceToHost));
    panel_to_rows(out, n, ncols, 0, ncols, hb.data(), n, pc0);
  };
  if (z_out) download(cg.b, 1, (size_t)T, z_out);
  if (x_out) download(cg.x, 0, (size_t)C, x_out);
  if (w_out) download(lik.W, 0, (size_t)C, w_out);
}

}  // namespace mogp
