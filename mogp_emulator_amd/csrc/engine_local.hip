// The LocalGP handle (engine.h): local approximate GP prediction and the Vecchia likelihood on a design that stays on the device.  Each
// method reads as its steps -- null pointers, the named refusals and the plan (predict_plan.h: plain arithmetic, checked on the host by
// tests/c/local_args_check.cpp, local_plan_check.cpp and vecchia_plan_check.cpp), then the launches of kernels_local.hip and the copies.
#include "engine_internal.h"

#include <algorithm>
#include <climits>

namespace mogp {

LocalGP::LocalGP(const double* inputs, long N_, int D_, const double* resid, int E_) : N(N_), D(D_), E(E_) {
  if (!inputs || !resid) throw std::runtime_error("predict_local: null pointer");
  if (D < 1 || D > MAX_D) throw std::runtime_error("predict_local: number of input dimensions must be between 1 and " + std::to_string(MAX_D));
  if (N < 1 || N > LOCAL_MAX_N) throw std::runtime_error("predict_local: the design must have between 1 and " + std::to_string(LOCAL_MAX_N) + " points");
  if (E < 1) throw std::runtime_error("predict_local: at least one row of targets is needed");
  HIPCK(hipGetDevice(&device));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) n_cu = cus;
  const size_t nd = (size_t)N * D;
  dX.reserve(nd);
  dXs.reserve(nd);
  dY.reserve((size_t)E * N);
  dScale.reserve(D);
  HIPCK(hipMemcpy(dX, inputs, nd * sizeof(double), hipMemcpyHostToDevice));
  HIPCK(hipMemcpy(dY, resid, (size_t)E * N * sizeof(double), hipMemcpyHostToDevice));
  iter.design = IterDesign{dXs, dY, N, D, E};      // (dXs and dY are reserved once, above, and never again: the pointers stay)
}

void LocalGP::ensure_scaled(const double* scale, hipStream_t st) {
  if (hScale.size() == (size_t)D && std::equal(hScale.begin(), hScale.end(), scale)) return;
  hScale.clear();
  HIPCK(hipMemcpyAsync(dScale, scale, D * sizeof(double), hipMemcpyHostToDevice, st));
  launch_local_scale(dX, N, D, dScale, dXs, st);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(st));
  hScale.assign(scale, scale + D);
}

void LocalGP::vecchia_neighbours(const double* scale, int k, int* nbr_out) {
  const char* who = "vecchia_neighbours";
  if (!scale) throw std::runtime_error("vecchia_neighbours: null pointer");
  local_check_k(who, N, k, true, LOCAL_MAX_K);
  local_check_scales(who, D, scale);
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  SyncOnUnwind sync{st};
  vk = 0;
  dVnbr.reserve((size_t)N * k);
  ensure_scaled(scale, st);
  launch_vecchia_knn(dXs, N, D, k, dVnbr, st);
  HIPCK(hipGetLastError());
  if (nbr_out) HIPCK(hipMemcpyAsync(nbr_out, dVnbr, (size_t)N * k * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  vk = k;
}

void LocalGP::vecchia_loglik(int e, int kt, const double* scale, double sigma2, double nugget, double jitter, int k, bool want_grad, int max_points,
                             double* value_out, double* grad_out, double* terms_out, int* ok_out) {
  const char* who = "vecchia_loglik";
  if (!scale || !value_out || (want_grad && !grad_out)) throw std::runtime_error("vecchia_loglik: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("vecchia_loglik: emulator index out of range");
  local_check_kernel(who, kt);
  if (vk == 0) throw std::runtime_error("vecchia_loglik: the neighbour lists have not been built (vecchia_neighbours)");
  if (k != vk) throw std::runtime_error("vecchia_loglik: the neighbour lists were built for n_neighbours = " + std::to_string(vk));
  local_check_hyper(who, D, scale, sigma2, nugget, jitter);
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const size_t wg = want_grad ? VECCHIA_WG_DOUBLES : LOCAL_WG_DOUBLES;
  const int cols = want_grad ? D + 3 : 1;
  const double held = vecchia_held_bytes(dVout.size(), dVred.size(), dVscratch.size(), dVok.size());
  const VecchiaPlan plan = vecchia_plan(N, D, want_grad, n_cu, (double)free_b + held, max_points, (double)wg * sizeof(double));
  SyncOnUnwind sync{st};
  dVout.reserve((size_t)cols * N);
  dVok.reserve((size_t)N);
  dVred.reserve((size_t)2 * cols * plan.blocks);
  dVscratch.reserve((size_t)plan.grid * wg);
  ensure_scaled(scale, st);
  const double* dYe = dY.get() + (size_t)e * N;
  for (long c0 = 0; c0 < N; c0 += plan.points) {
    const int mc = (int)std::min<long>(plan.points, N - c0);
    launch_vecchia_ll(dXs, dYe, N, D, c0, mc, k, dVnbr, kt, sigma2, nugget + jitter, nugget, want_grad, dVscratch, std::min(plan.grid, mc), dVout,
                      dVok, st);
  }
  HIPCK(hipGetLastError());
  double* half = dVred.get() + (size_t)cols * plan.blocks;
  const double* sums = launch_vecchia_reduce(dVout, N, cols, dVred, half, st);
  HIPCK(hipGetLastError());
  std::vector<double> h(cols);
  HIPCK(hipMemcpyAsync(h.data(), sums, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, st));
  if (terms_out) HIPCK(hipMemcpyAsync(terms_out, dVout, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (ok_out) HIPCK(hipMemcpyAsync(ok_out, dVok, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  *value_out = h[0];
  if (want_grad) std::copy(h.begin() + 1, h.end(), grad_out);
}

void LocalGP::predict(int e, int kt, const double* scale, double sigma2, double nugget, double jitter, bool include_nugget, const double* testing,
                      long m, int k, int max_points, double* mean, double* var, int* ok, double* radius, int* nbr) {
  const char* who = "predict_local";
  if (!scale || !testing || !mean || !ok || !radius) throw std::runtime_error("predict_local: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("predict_local: emulator index out of range");
  local_check_kernel(who, kt);
  local_check_k(who, N, k, false, LOCAL_MAX_K);
  if (m < 1 || m > INT_MAX) throw std::runtime_error("predict_local: at least one testing point is needed");
  local_check_hyper(who, D, scale, sigma2, nugget, jitter);
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const LocalPlan plan = local_plan(m, D, k, n_cu, (double)free_b, max_points, (double)LOCAL_WG_DOUBLES * sizeof(double));
  const size_t P = (size_t)plan.points;
  QueryPass pass(P, D);
  DevBuf<double> dRad(P), dMean(P), dVar(P), dScratch((size_t)plan.grid * LOCAL_WG_DOUBLES);
  DevBuf<int> dNbr(P * k), dOk(P);
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  const double* dYe = dY.get() + (size_t)e * N;
  for (long c0 = 0; c0 < m; c0 += plan.points) {
    const int mc = (int)std::min<long>(plan.points, m - c0);
    const int grid = std::min(plan.grid, mc);
    const double* dQs = pass.load(testing, c0, mc, dScale, st);
    launch_local_knn(dXs, N, D, dQs, mc, k, dNbr, dRad, st);
    launch_local_gp(dXs, dYe, N, D, dQs, mc, k, dNbr, kt, sigma2, nugget + jitter, include_nugget ? nugget : 0., dScratch, grid, dMean, dVar, dOk, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(mean + c0, dMean, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (var) HIPCK(hipMemcpyAsync(var + c0, dVar, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(ok + c0, dOk, (size_t)mc * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(radius + c0, dRad, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nbr) HIPCK(hipMemcpyAsync(nbr + (size_t)c0 * k, dNbr, (size_t)mc * k * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
}

}  // namespace mogp
