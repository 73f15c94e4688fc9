// Pathwise posterior draws on the LocalGP handle (engine.h; DESIGN.md section 3 "Pathwise posterior draws"): a draw of the posterior is the
// function  f_s(.) = g_s(.) + sigma2 k(., X) v_s  with a random-Fourier-feature prior draw g_s = amp Phi(.) W_s and the update
// v_s = A^-1 (y - g_s(X) - sqrt(nugget) e_s)  (Matheron's rule; Wilson et al. 2020).  Three entry points, each as its steps: null pointers, the
// named refusals and the plan (predict_plan.h: plain arithmetic, checked on the host by tests/c/rff_plan_check.cpp and
// inputderiv_plan_check.cpp), the launches, the copies.
//   rff            the feature product at the design or at queries, in passes of points and of ITER_COLS draws
//   rff_inputderiv its derivative with respect to the raw coordinates of the queries, (draws, points, D), in the same passes
//   sample_paths   the weights' normals, g_s(X), the right-hand sides and the solves, ITER_COLS draws at a time through IterSolver::solve as it is
// Nothing of the design-sized work crosses the bus but v and, where the device generated them, the weights' normals.
#include "engine_internal.h"

#include <algorithm>
#include <climits>

namespace mogp {

namespace {

void rff_check_inputs(const std::string& who, int D, int F, const double* omega, const double* phase, double amp) {
  require_finite(omega, (size_t)F * D, (who + ": the frequencies must be finite").c_str());
  require_finite(phase, (size_t)F, (who + ": the phases must be finite").c_str());
  if (!std::isfinite(amp)) throw std::runtime_error(who + ": the amplitude must be finite");
}

}  // namespace

void LocalGP::rff(const double* scale, const double* queries, long m, const double* omega, const double* phase, int F, const double* W, int S,
                  double amp, int max_points, double* out) {
  const std::string who = "rff";
  if (!scale || !omega || !phase || !W || !out) throw std::runtime_error("rff: null pointer");
  local_check_scales(who, D, scale);
  rff_check_counts(who, F, S, 0);
  if (queries && (m < 1 || m > INT_MAX)) throw std::runtime_error("rff: at least one query is needed");
  rff_check_inputs(who, D, F, omega, phase, amp);
  require_finite(W, (size_t)S * F, "rff: the weights must be finite");
  const long M = queries ? m : N;
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const RffPlan plan = rff_plan(who, M, D, F, S, (double)free_b, max_points);
  const size_t P = (size_t)plan.points, f = (size_t)F;
  DevBuf<double> dOm(f * D), dPh(f), dW(f * ITER_COLS), dO(P * ITER_COLS);
  QueryPass pass(queries ? P : 0, D);
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  HIPCK(hipMemcpyAsync(dOm, omega, f * D * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dPh, phase, f * sizeof(double), hipMemcpyHostToDevice, st));
  for (long p0 = 0; p0 < M; p0 += plan.points) {
    const long mc = std::min<long>(plan.points, M - p0);
    const double* rows = queries ? pass.load(queries, p0, mc, dScale, st) : dXs.get() + (size_t)p0 * D;
    for (int c0 = 0; c0 < S; c0 += ITER_COLS) {
      const int cols = std::min(ITER_COLS, S - c0), nb = cols > 16 ? 2 : 1;
      // (S, F) row-major is a panel of S columns already; the columns behind `cols` of the last block are exact zeros
      HIPCK(hipMemsetAsync(dW, 0, f * 16 * nb * sizeof(double), st));
      HIPCK(hipMemcpyAsync(dW, W + (size_t)c0 * f, f * cols * sizeof(double), hipMemcpyHostToDevice, st));
      launch_rff(rows, mc, dOm, dPh, F, D, dW, F, nb, amp, dO, mc, st);
      HIPCK(hipGetLastError());
      for (int c = 0; c < cols; ++c)
        HIPCK(hipMemcpyAsync(out + (size_t)(c0 + c) * M + p0, dO.get() + (size_t)c * mc, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
    }
  }
}

void LocalGP::rff_inputderiv(const double* scale, const double* queries, long m, const double* omega, const double* phase, int F, const double* W,
                             int S, double amp, int max_points, double* out) {
  const std::string who = "rff_inputderiv";
  if (!scale || !queries || !omega || !phase || !W || !out) throw std::runtime_error("rff_inputderiv: null pointer");
  local_check_scales(who, D, scale);
  rff_check_counts(who, F, S, 0);
  if (m < 1 || m > INT_MAX) throw std::runtime_error("rff_inputderiv: at least one query is needed");
  rff_check_inputs(who, D, F, omega, phase, amp);
  require_finite(W, (size_t)S * F, "rff_inputderiv: the weights must be finite");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const InderivPlan plan = rff_inderiv_plan(who, m, D, F, S, (double)free_b, max_points);
  const size_t P = (size_t)plan.points, f = (size_t)F, wide = (size_t)D * ITER_COLS;
  DevBuf<double> dOm(f * D), dPh(f), dW(f * ITER_COLS), dO(P * wide);
  QueryPass pass(P, D);
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  HIPCK(hipMemcpyAsync(dOm, omega, f * D * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dPh, phase, f * sizeof(double), hipMemcpyHostToDevice, st));
  std::vector<double> ho(P * wide);
  for (long p0 = 0; p0 < m; p0 += plan.points) {
    const long mc = std::min<long>(plan.points, m - p0);
    const double* rows = pass.load(queries, p0, mc, dScale, st);
    for (int c0 = 0; c0 < S; c0 += ITER_COLS) {
      const int cols = std::min(ITER_COLS, S - c0), nb = cols > 16 ? 2 : 1;
      // (S, F) row-major is a panel of S columns already; the columns behind `cols` of the last block are exact zeros
      HIPCK(hipMemsetAsync(dW, 0, f * 16 * nb * sizeof(double), st));
      HIPCK(hipMemcpyAsync(dW, W + (size_t)c0 * f, f * cols * sizeof(double), hipMemcpyHostToDevice, st));
      launch_rff_inderiv(rows, mc, dOm, dPh, F, D, dW, F, nb, amp, dScale, dO, mc, st);
      HIPCK(hipGetLastError());
      HIPCK(hipMemcpyAsync(ho.data(), dO, (size_t)mc * D * 16 * nb * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      // out[c0 + c][p0 + i][d] = the panel's column 16 nb d + c
      for (int c = 0; c < cols; ++c)
        for (long i = 0; i < mc; ++i) {
          double* dst = out + ((size_t)(c0 + c) * m + (size_t)(p0 + i)) * D;
          for (int d = 0; d < D; ++d) dst[d] = ho[((size_t)d * 16 * nb + c) * mc + i];
        }
    }
  }
}

void LocalGP::sample_paths(int e, int kt, const double* scale, double sigma2, double nugget, int rank, double rtol, int max_iter,
                           const double* omega, const double* phase, int F, int S, double amp, unsigned long long seed, unsigned stream,
                           int first_draw, const double* W_in, const double* noise_in, double* W_out, double* v_out, int* stat_i, double* residual,
                           int* rank_out) {
  const std::string who = "sample_paths";
  if (!scale || !omega || !phase || !W_out || !v_out || !stat_i || !residual || !rank_out) throw std::runtime_error("sample_paths: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("sample_paths: emulator index out of range");
  local_check_kernel(who, kt);
  iter_check_hyper(who, D, scale, sigma2, nugget);
  iter_check_rank(who, N, rank);
  iter_check_solve(who, 1, rtol, max_iter);
  rff_check_counts(who, F, S, first_draw);
  rff_check_inputs(who, D, F, omega, phase, amp);
  if (W_in) require_finite(W_in, (size_t)S * F, "sample_paths: feature_normals must be finite");
  if (noise_in) require_finite(noise_in, (size_t)S * N, "sample_paths: noise_normals must be finite");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  const IterKey k = make_key(kt, scale, D, sigma2, nugget, rank);
  iter.reserve(who.c_str(), rank);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  (void)rff_plan(who, 1, D, F, S, (double)free_b, 0);        // the features' own buffers; the design's rows are on the device already
  const size_t f = (size_t)F, n = (size_t)N;
  DevBuf<double> dOm(f * D), dPh(f), dW(f * ITER_COLS);
  SyncOnUnwind sync{st};
  precondition_for(k, st);
  *rank_out = iter.pre.rank();
  IterSolver::CgPanels& cg = iter.cg;
  HIPCK(hipMemcpyAsync(dOm, omega, f * D * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCK(hipMemcpyAsync(dPh, phase, f * sizeof(double), hipMemcpyHostToDevice, st));
  const double root = std::sqrt(nugget);
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  for (int c0 = 0; c0 < S; c0 += ITER_COLS) {
    const int cols = std::min(ITER_COLS, S - c0), nb = cols > 16 ? 2 : 1;
    const unsigned draw0 = (unsigned)(first_draw + c0);
    HIPCK(hipMemsetAsync(dW, 0, f * 16 * nb * sizeof(double), st));
    if (W_in)
      HIPCK(hipMemcpyAsync(dW, W_in + (size_t)c0 * f, f * cols * sizeof(double), hipMemcpyHostToDevice, st));
    else
      launch_rff_normals(seed, stream + 3u, draw0, cols, F, dW, F, st);
    HIPCK(hipMemcpyAsync(W_out + (size_t)c0 * f, dW, f * cols * sizeof(double), hipMemcpyDeviceToHost, st));
    // g_s(X) into cg.q (the solve overwrites it afterwards), the caller's noise into cg.v, the right-hand sides into cg.b
    launch_rff(dXs, N, dOm, dPh, F, D, dW, F, nb, amp, cg.q, N, st);
    if (noise_in) HIPCK(hipMemcpyAsync(cg.v, noise_in + (size_t)c0 * n, n * cols * sizeof(double), hipMemcpyHostToDevice, st));
    launch_rff_rhs(dY.get() + (size_t)e * n, cg.q, noise_in ? cg.v.get() : nullptr, N, cols, root, seed, stream + 4u, draw0, cg.b, st);
    HIPCK(hipGetLastError());
    iter.solve(cols, rtol, max_iter, it, cv, rs, st);
    HIPCK(hipMemcpyAsync(v_out + (size_t)c0 * n, cg.x, n * cols * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int c = 0; c < cols; ++c) {
      stat_i[2 * (c0 + c)] = it[c];
      stat_i[2 * (c0 + c) + 1] = cv[c];
      residual[c0 + c] = rs[c];
    }
  }
}

}  // namespace mogp
