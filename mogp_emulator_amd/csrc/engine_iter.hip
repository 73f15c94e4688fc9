// Iterative exact prediction on the LocalGP handle (engine.h): conjugate gradients on A = sigma2 k(X, X) + nugget I of the whole design,
// preconditioned by a partial pivoted Cholesky factor, with A never stored (kernels_iter.hip generates its entries as they are multiplied).
// Each method reads as its steps: null pointers, the named refusals and the plan (predict_plan.h: plain arithmetic, checked on the host by
// tests/c/iter_plan_check.cpp), then the launches and the copies.  The iteration is a host loop of plain launches bounded by max_iter; the
// step scalars and the frozen flags live on the device and the host looks at the flags every ITER_LOOK iterations.
#include "engine_internal.h"
#include "iter_var_host.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace mogp {

namespace {

static_assert(ITER_COLS == ITER_PLAN_COLS && ITER_SEG == ITER_PLAN_SEG && ITER_DOT_BLOCK == ITER_PLAN_DOT, "predict_plan.h counts the bytes of the panels and segments of launch.h");
constexpr int ITER_LOOK = 8;      // iterations between two looks of the host at the frozen flags (no result depends on it)

// Ginv = G^-1 of the symmetric positive definite G (p x p, row-major), in place and exactly symmetric: G = C C^T, U = C^-T (row j of U is
// column j of C^-1), Ginv = U U^T.  Plain loops over contiguous rows; p <= 1024.  Returns log|G| = 2 sum_i log C_ii.
double spd_inverse(std::vector<double>& G, int p) {
  std::vector<double> C((size_t)p * p, 0.0), U((size_t)p * p, 0.0);
  for (int i = 0; i < p; ++i) {
    const double* gi = &G[(size_t)i * p];
    double* ci = &C[(size_t)i * p];
    for (int j = 0; j <= i; ++j) {
      const double* cj = &C[(size_t)j * p];
      double s = gi[j];
      for (int k = 0; k < j; ++k) s -= ci[k] * cj[k];
      if (i == j) {
        if (!(s > 0.0) || !std::isfinite(s)) throw std::runtime_error("precondition: nugget I + L^T L is not positive definite");
        ci[j] = std::sqrt(s);
      } else {
        ci[j] = s / cj[j];
      }
    }
  }
  for (int j = 0; j < p; ++j) {
    double* u = &U[(size_t)j * p];
    for (int i = j; i < p; ++i) {
      const double* ci = &C[(size_t)i * p];
      double s = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= ci[k] * u[k];
      u[i] = s / ci[i];
    }
  }
  for (int a = 0; a < p; ++a)
    for (int b = 0; b <= a; ++b) {
      const double *ua = &U[(size_t)a * p], *ub = &U[(size_t)b * p];
      double s = 0.0;
      for (int k = a; k < p; ++k) s += ua[k] * ub[k];
      G[(size_t)a * p + b] = G[(size_t)b * p + a] = s;
    }
  double logdet = 0.0;
  for (int i = 0; i < p; ++i) logdet += std::log(C[(size_t)i * p + i]);
  return 2.0 * logdet;
}

}  // namespace

double LocalGP::iter_held() const {
  double held = 0.;
  for (const DevBuf<double>* b : {&itL, &itG, &itDiag, &itDmax, &itPval, &itB, &itX, &itXl, &itR, &itP, &itQ, &itZ, &itV, &itWpart, &itW, &itW2, &itPart, &itSc})
    held += 8.0 * (double)b->size();
  for (const DevBuf<int>* b : {&itPiv, &itState, &itPidx, &itFl}) held += 4.0 * (double)b->size();
  return held;
}

void LocalGP::iter_reserve(const char* who, int rank) {
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const double held = iter_held();                           // what the handle holds of it already is reused, hence counts as free
  iter_check_memory(who, N, rank, (double)free_b, held);
  const size_t n = (size_t)N, panel = n * ITER_COLS, p = (size_t)std::max(rank, 1);
  const size_t segs = (n + ITER_SEG - 1) / ITER_SEG, dots = (n + ITER_DOT_BLOCK - 1) / ITER_DOT_BLOCK, blk = (n + 1023) / 1024;
  if (itL.size() < n * p) itKey = IterKey();                 // (the factor is about to be freed)
  itL.reserve(n * p);
  itG.reserve(p * p);
  itDiag.reserve(n);
  itDmax.reserve(p);
  itPiv.reserve(p);
  itState.reserve(2);
  itPval.reserve(blk);
  itPidx.reserve(blk);
  for (DevBuf<double>* b : {&itB, &itX, &itXl, &itR, &itP, &itQ, &itZ, &itV}) b->reserve(panel);
  itWpart.reserve(segs * p * ITER_COLS);
  itW.reserve(p * ITER_COLS);
  itW2.reserve(p * ITER_COLS);
  itPart.reserve(dots * ITER_COLS);
  itSc.reserve(5 * ITER_COLS);
  itFl.reserve(3 * ITER_COLS);
}

void LocalGP::iter_build(const IterKey& k, hipStream_t st) {
  ensure_scaled(k.scale.data(), st);
  if (k == itKey) return;
  itKey = IterKey();
  int state[2] = {0, 0};
  if (k.rank > 0) {
    launch_pchol_init(itDiag, N, k.sigma2, itState, st);
    for (int t = 0; t < k.rank; ++t) launch_pchol_step(dXs, N, D, k.kt, k.sigma2, t, itL, itDiag, itPiv, itDmax, itState, itPval, itPidx, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(state, itState, sizeof(state), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
  const int p = state[0];
  itLogdetG = 0.;
  if (p > 0) {
    launch_pchol_gram(itL, N, p, k.nugget, itG, st);
    HIPCK(hipGetLastError());
    std::vector<double> G((size_t)p * p);
    HIPCK(hipMemcpyAsync(G.data(), itG, G.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    itLogdetG = spd_inverse(G, p);
    HIPCK(hipMemcpyAsync(itG, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  itRank = p;
  itKey = k;
}

void LocalGP::iter_cg(int cols, double rtol, int max_iter, int* it_out, int* cv_out, double* rs_out, hipStream_t st, double* first_z,
                      double* coef_log) {
  const size_t panel_bytes = (size_t)N * ITER_COLS * sizeof(double);
  const IterKey& k = itKey;
  const bool pre = itRank > 0;
  // Columns >= cols of itB are zero and freeze at iteration 0, so with at most 16 live columns the product serves one block of 16 alone.
  // A column's bits do not depend on that: the product keeps its columns apart.  (The columns it then skips hold zeros, not stale data.)
  const int nb = cols > 16 ? 2 : 1;
  if (nb == 1) HIPCK(hipMemsetAsync(itQ, 0, panel_bytes, st));
  double* z = pre ? itZ.get() : itR.get();                   // plain CG: z = r
  auto apply = [&] {
    if (pre) launch_precond_apply(itL, N, itRank, itG, k.nugget, itR, itZ, itWpart, itW, itW2, st);
  };
  auto dot = [&](int mode, const double* a, const double* b, int it) {
    launch_cg_dot(a, b, N, itPart, st);
    launch_cg_scalars(mode, itPart, N, itSc, itFl, it, rtol, st, coef_log);
  };
  HIPCK(hipMemsetAsync(itX, 0, panel_bytes, st));
  HIPCK(hipMemsetAsync(itXl, 0, panel_bytes, st));
  HIPCK(hipMemcpyAsync(itR, itB, panel_bytes, hipMemcpyDeviceToDevice, st));
  dot(0, itB, itB, 0);
  apply();
  if (first_z) HIPCK(hipMemcpyAsync(first_z, z, panel_bytes, hipMemcpyDeviceToDevice, st));
  dot(1, itR, z, 0);
  launch_cg_direction(itP, z, N, true, itSc, itFl, st);
  int fl[3 * ITER_COLS];
  for (int it = 0; it < max_iter; ++it) {
    launch_kmatvec(dXs, N, dXs, N, D, k.kt, k.sigma2, k.nugget, true, itP, N, nb, itQ, N, st);
    dot(2, itP, itQ, it);
    launch_cg_update(itX, itXl, itR, itP, itQ, N, itSc, itFl, st);
    dot(3, itR, itR, it);
    apply();
    dot(4, itR, z, it);
    launch_cg_direction(itP, z, N, false, itSc, itFl, st);
    HIPCK(hipGetLastError());
    if ((it + 1) % ITER_LOOK == 0 && it + 1 < max_iter) {
      HIPCK(hipMemcpyAsync(fl, itFl, ITER_COLS * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      if (std::all_of(fl, fl + ITER_COLS, [](int f) { return f != 0; })) break;
    }
  }
  launch_panel_add(itX, itXl, N, st);                          // the iterate is x + xl: rounded once, here
  // the true residual, from one further product
  launch_kmatvec(dXs, N, dXs, N, D, k.kt, k.sigma2, k.nugget, true, itX, N, nb, itQ, N, st);
  launch_panel_sub(itB, itQ, N, itR, st);
  dot(5, itR, itR, 0);
  HIPCK(hipGetLastError());
  double sc[5 * ITER_COLS];
  HIPCK(hipMemcpyAsync(fl, itFl, sizeof(fl), hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(sc, itSc, sizeof(sc), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  for (int c = 0; c < ITER_COLS; ++c) {
    const bool frozen = fl[c] != 0;
    it_out[c] = frozen ? fl[2 * ITER_COLS + c] : max_iter;
    cv_out[c] = frozen ? fl[ITER_COLS + c] : 0;
    const double bb = sc[c], rr = sc[4 * ITER_COLS + c];
    rs_out[c] = bb == 0.0 ? 0.0 : std::sqrt(rr) / std::sqrt(bb);
  }
}

void LocalGP::kmatvec(int kt, const double* scale, double sigma2, double nugget, const double* queries, long m, const double* V, int r, double* out) {
  const char* who = "kmatvec";
  if (!scale || !V || !out) throw std::runtime_error("kmatvec: null pointer");
  local_check_kernel(who, kt);
  local_check_hyper(who, D, scale, sigma2, nugget, 0.);
  if (r < 1) throw std::runtime_error("kmatvec: at least one column is needed");
  if (queries && (m < 1 || m > INT_MAX)) throw std::runtime_error("kmatvec: at least one query is needed");
  const long M = queries ? m : N;
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const int wide = r > 16 ? 32 : 16;
  const double need = 8.0 * ((double)wide * ((double)N + (double)M) + (queries ? 2.0 * (double)M * D : 0.0));
  if (need > 0.5 * (double)free_b)
    throw std::runtime_error("kmatvec: " + std::to_string((long long)need) + " bytes of device memory are more than half of the free device memory");
  DevBuf<double> dV((size_t)N * wide), dO((size_t)M * wide), dQ, dQs;
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  const double* rows = dXs;
  if (queries) {
    dQ.reserve((size_t)M * D);
    dQs.reserve((size_t)M * D);
    HIPCK(hipMemcpyAsync(dQ, queries, (size_t)M * D * sizeof(double), hipMemcpyHostToDevice, st));
    launch_local_scale(dQ, M, D, dScale, dQs, st);
    rows = dQs;
  }
  std::vector<double> hv((size_t)N * wide), ho((size_t)M * wide);
  for (int c0 = 0; c0 < r; c0 += ITER_COLS) {
    const int cols = std::min(ITER_COLS, r - c0), nb = cols > 16 ? 2 : 1;
    std::fill(hv.begin(), hv.end(), 0.0);
    for (long j = 0; j < N; ++j)
      for (int c = 0; c < cols; ++c) hv[(size_t)c * N + j] = V[(size_t)j * r + c0 + c];
    HIPCK(hipMemcpyAsync(dV, hv.data(), (size_t)N * 16 * nb * sizeof(double), hipMemcpyHostToDevice, st));
    launch_kmatvec(rows, M, dXs, N, D, kt, sigma2, nugget, !queries, dV, N, nb, dO, M, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(ho.data(), dO, (size_t)M * 16 * nb * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (long i = 0; i < M; ++i)
      for (int c = 0; c < cols; ++c) out[(size_t)i * r + c0 + c] = ho[(size_t)c * M + i];
  }
}

int LocalGP::precondition(int kt, const double* scale, double sigma2, double nugget, int rank, int* piv_out, double* L_out) {
  const char* who = "precondition";
  if (!scale) throw std::runtime_error("precondition: null pointer");
  local_check_kernel(who, kt);
  iter_check_hyper(who, D, scale, sigma2, nugget);
  iter_check_rank(who, N, rank);
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  SyncOnUnwind sync{st};
  IterKey k;
  k.kt = kt, k.rank = rank, k.sigma2 = sigma2, k.nugget = nugget;
  k.scale.assign(scale, scale + D);
  iter_reserve(who, rank);
  iter_build(k, st);
  if (piv_out) {
    std::fill(piv_out, piv_out + rank, 0);
    if (itRank > 0) HIPCK(hipMemcpy(piv_out, itPiv, (size_t)itRank * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (L_out) {
    std::fill(L_out, L_out + (size_t)N * rank, 0.0);
    std::vector<double> col((size_t)N);
    for (int t = 0; t < itRank; ++t) {
      HIPCK(hipMemcpy(col.data(), itL.get() + (size_t)t * N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
      for (long i = 0; i < N; ++i) L_out[(size_t)i * rank + t] = col[i];
    }
  }
  return itRank;
}

void LocalGP::solve(const double* B, int c, double rtol, int max_iter, double* x, int* iterations, int* converged, double* residual) {
  const char* who = "solve";
  if (!B || !x || !iterations || !converged || !residual) throw std::runtime_error("solve: null pointer");
  iter_check_solve(who, c, rtol, max_iter);
  if (itKey.kt < 0) throw std::runtime_error("solve: precondition has not been called");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  SyncOnUnwind sync{st};
  const IterKey k = itKey;
  iter_build(k, st);                                         // (the scaled design may have been formed for other scales since)
  std::vector<double> hb((size_t)N * ITER_COLS);
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  for (int c0 = 0; c0 < c; c0 += ITER_COLS) {
    const int cols = std::min(ITER_COLS, c - c0);
    std::fill(hb.begin(), hb.end(), 0.0);
    for (long j = 0; j < N; ++j)
      for (int q = 0; q < cols; ++q) hb[(size_t)q * N + j] = B[(size_t)j * c + c0 + q];
    HIPCK(hipMemcpyAsync(itB, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice, st));
    iter_cg(cols, rtol, max_iter, it, cv, rs, st);
    HIPCK(hipMemcpy(hb.data(), itX, hb.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (long j = 0; j < N; ++j)
      for (int q = 0; q < cols; ++q) x[(size_t)j * c + c0 + q] = hb[(size_t)q * N + j];
    std::copy(it, it + cols, iterations + c0);
    std::copy(cv, cv + cols, converged + c0);
    std::copy(rs, rs + cols, residual + c0);
  }
}

void LocalGP::predict_exact(int e, int kt, const double* scale, double sigma2, double nugget, int rank, double rtol, int max_iter,
                            bool include_nugget, const double* testing, long m, int max_points, double* mean, double* var, int* stat_i,
                            double* stat_r, int* var_stat_i, double* var_stat_r, double* alpha_out) {
  const char* who = "predict_exact";
  if (!scale || !stat_i || !stat_r || (m > 0 && (!testing || !mean)) || (var && (!var_stat_i || !var_stat_r)))
    throw std::runtime_error("predict_exact: null pointer");
  if (e < 0 || e >= E) throw std::runtime_error("predict_exact: emulator index out of range");
  local_check_kernel(who, kt);
  iter_check_hyper(who, D, scale, sigma2, nugget);
  iter_check_rank(who, N, rank);
  iter_check_solve(who, 1, rtol, max_iter);
  if (m < 0 || m > INT_MAX) throw std::runtime_error("predict_exact: the number of testing points must not be negative");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  IterKey k;
  k.kt = kt, k.rank = rank, k.sigma2 = sigma2, k.nugget = nugget;
  k.scale.assign(scale, scale + D);
  iter_reserve(who, rank);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const IterPlan plan = iter_plan(who, std::max<long>(m, 1), D, (double)free_b, max_points);
  const size_t P = (size_t)plan.points;
  DevBuf<double> dQ(P * D), dQs(P * D), dOut(P * 16), dEye((size_t)ITER_COLS * ITER_COLS);
  SyncOnUnwind sync{st};
  iter_build(k, st);
  const size_t panel_bytes = (size_t)N * ITER_COLS * sizeof(double);
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  // alpha of this emulator: kept while everything it depends on stays
  IterKey ak = k;
  ak.rtol = rtol, ak.max_iter = max_iter;
  if (itAlpha.size() != (size_t)E) itAlpha.assign(E, IterAlpha());
  IterAlpha& a = itAlpha[e];
  if (!(a.key == ak)) {
    a.key = IterKey();
    HIPCK(hipMemsetAsync(itB, 0, panel_bytes, st));
    HIPCK(hipMemcpyAsync(itB, dY.get() + (size_t)e * N, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
    iter_cg(1, rtol, max_iter, it, cv, rs, st);
    a.alpha.resize((size_t)N);
    HIPCK(hipMemcpy(a.alpha.data(), itX, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    a.iterations = it[0], a.converged = cv[0], a.residual = rs[0];
    a.key = ak;
  }
  stat_i[0] = a.iterations, stat_i[1] = a.converged, stat_r[0] = a.residual;
  if (alpha_out) std::copy(a.alpha.begin(), a.alpha.end(), alpha_out);
  if (m == 0) return;
  // alpha as column 0 of a panel of 16 (the others zero): the rectangular product's V
  HIPCK(hipMemsetAsync(itV, 0, (size_t)N * 16 * sizeof(double), st));
  HIPCK(hipMemcpyAsync(itV, a.alpha.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
  if (var) {
    std::vector<double> eye((size_t)ITER_COLS * ITER_COLS, 0.0);
    for (int c = 0; c < ITER_COLS; ++c) eye[(size_t)c * ITER_COLS + c] = 1.0;
    HIPCK(hipMemcpyAsync(dEye, eye.data(), eye.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  const double var_add = include_nugget ? nugget : 0.;
  for (long c0 = 0; c0 < m; c0 += plan.points) {
    const long mc = std::min<long>(plan.points, m - c0);
    HIPCK(hipMemcpyAsync(dQ, testing + (size_t)c0 * D, (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, st));
    launch_local_scale(dQ, mc, D, dScale, dQs, st);
    launch_kmatvec(dQs, mc, dXs, N, D, kt, sigma2, 0., false, itV, N, 1, dOut, mc, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(mean + c0, dOut, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (!var) continue;
    for (long b0 = 0; b0 < mc; b0 += ITER_COLS) {
      const int nq = (int)std::min<long>(ITER_COLS, mc - b0);
      // the cross columns sigma2 k(X, q): the rectangular product with the design as rows, the queries as columns and V = I; columns
      // >= nq of the panel are exact zeros and freeze at iteration 0
      launch_kmatvec(dXs, N, dQs.get() + (size_t)b0 * D, nq, D, kt, sigma2, 0., false, dEye, ITER_COLS, 2, itB, N, st);
      iter_cg(nq, rtol, max_iter, it, cv, rs, st);
      launch_cg_dot(itB, itX, N, itPart, st);
      launch_cg_scalars(5, itPart, N, itSc, itFl, 0, rtol, st);
      HIPCK(hipGetLastError());
      double kz[ITER_COLS];
      HIPCK(hipMemcpyAsync(kz, itSc.get() + 4 * ITER_COLS, sizeof(kz), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      for (int q = 0; q < nq; ++q) {
        const double v = (sigma2 - kz[q]) + var_add;
        var[c0 + b0 + q] = v < 0.0 ? 0.0 : v;                // the floor of predict(): clipped at zero, NaN stays
        var_stat_i[2 * (c0 + b0 + q)] = it[q];
        var_stat_i[2 * (c0 + b0 + q) + 1] = cv[q];
        var_stat_r[c0 + b0 + q] = rs[q];
      }
    }
  }
}

// The cache of the variance bound: R (N, r) with span R = span L and R^T A R = I, in two orthonormalisations so that no matrix worse
// conditioned than A is factorised (chol(L^T A L) directly would meet cond(A) cond(L)^2):
//   G0 = L^T L,  G0[:r0, :r0] = C0 C0^T (a prefix, stopped where L's columns become dependent),  Q = L[:, :r0] C0^-T   (Q^T Q = I)
//   H = Q^T (A Q) one panel of 32 columns at a time,  H = C C^T (a prefix, stopped at a pivot <= 0),  R = Q[:, :r] C^-T
// Both triangular factors are prefixes, so R[:, :r'] is the cache of every smaller rank r'.
void LocalGP::iter_var_build(const IterKey& k, hipStream_t st) {
  if (k == itVarKey) return;
  itVarKey = IterKey();
  itVarRank = 0;
  const int p = itRank;
  const int pad = (int)iter_var_pad(std::max(p, 1));
  int r = 0;
  if (p > 0) {
    HIPCK(hipMemsetAsync(itVR, 0, (size_t)N * pad * sizeof(double), st));       // (the product with A reads whole panels of 32 columns)
    launch_pchol_gram(itL, N, p, 0., itVT, st);
    HIPCK(hipGetLastError());
    std::vector<double> G((size_t)p * p), C, T;
    HIPCK(hipMemcpyAsync(G.data(), itVT, G.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    const int r0 = prefix_cholesky(G.data(), p, ITER_VAR_TAU * G[0], C);
    if (r0 > 0) {
      upper_inverse(C.data(), p, r0, T, pad);
      HIPCK(hipMemcpyAsync(itVT, T.data(), (size_t)r0 * pad * sizeof(double), hipMemcpyHostToDevice, st));
      for (int c0 = 0; c0 < r0; c0 += ITER_COLS) launch_tri_right(itL, N, r0, itVT, pad, c0, itVR, st);
      HIPCK(hipGetLastError());
      std::vector<double> H((size_t)r0 * r0), w((size_t)r0 * ITER_COLS);
      for (int b0 = 0; b0 < r0; b0 += ITER_COLS) {
        launch_kmatvec(dXs, N, dXs, N, D, k.kt, k.sigma2, k.nugget, true, itVR.get() + (size_t)b0 * N, N, 2, itQ, N, st);
        launch_ltv(itVR, N, r0, itQ, itWpart, itW, st);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(w.data(), itW, w.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int a = 0; a < r0; ++a)
          for (int c = 0; c < ITER_COLS && b0 + c < r0; ++c) H[(size_t)a * r0 + b0 + c] = w[(size_t)a * ITER_COLS + c];
      }
      for (int a = 0; a < r0; ++a)
        for (int b = 0; b < a; ++b) H[(size_t)a * r0 + b] = H[(size_t)b * r0 + a] = 0.5 * (H[(size_t)a * r0 + b] + H[(size_t)b * r0 + a]);
      r = prefix_cholesky(H.data(), r0, 0., C);
      if (r > 0) {
        upper_inverse(C.data(), r0, r, T, pad);
        HIPCK(hipMemcpyAsync(itVT, T.data(), (size_t)r * pad * sizeof(double), hipMemcpyHostToDevice, st));
        for (int c0 = ((r - 1) / ITER_COLS) * ITER_COLS; c0 >= 0; c0 -= ITER_COLS) launch_tri_right(itVR, N, r, itVT, pad, c0, itVR, st);   // in place: descending
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(st));                     // (T is a local)
      }
    }
  }
  itVarRank = r;
  itVarReached = p;
  itVarKey = k;
}

void LocalGP::variance_bound(int kt, const double* scale, double sigma2, double nugget, int rank, int var_rank_request, bool include_nugget,
                             const double* testing, long m, int max_points, double* var, int* var_rank_out, double* R_out) {
  const char* who = "variance_bound";
  if (!scale || !var_rank_out || (m > 0 && (!testing || !var))) throw std::runtime_error("variance_bound: null pointer");
  local_check_kernel(who, kt);
  iter_check_hyper(who, D, scale, sigma2, nugget);
  iter_check_rank(who, N, rank);
  iter_var_check_precond(who, rank);
  iter_var_check_rank(who, var_rank_request, rank);
  if (m < 0 || m > INT_MAX) throw std::runtime_error("variance_bound: the number of testing points must not be negative");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  IterKey k;
  k.kt = kt, k.rank = rank, k.sigma2 = sigma2, k.nugget = nugget;
  k.scale.assign(scale, scale + D);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  iter_var_check_memory(who, N, rank, (double)free_b, iter_held() + 8.0 * ((double)itVR.size() + (double)itVT.size()));
  iter_reserve(who, rank);
  const size_t pad = (size_t)iter_var_pad(rank);
  if (itVR.size() < (size_t)N * pad || itVT.size() < pad * pad) itVarKey = IterKey();      // (the cache is about to be freed)
  itVR.reserve((size_t)N * pad);
  itVT.reserve(pad * pad);
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const IterPlan plan = iter_plan(who, std::max<long>(m, 1), D, (double)free_b, max_points);
  const size_t P = (size_t)plan.points;
  DevBuf<double> dQ(P * D), dQs(P * D), dPart(P * 16);
  SyncOnUnwind sync{st};
  if (k == itVarKey) {
    ensure_scaled(k.scale.data(), st);                       // the cache stands for itself: the preconditioner held may be another's
  } else {
    iter_build(k, st);
    iter_var_build(k, st);
  }
  iter_var_check_rank(who, var_rank_request, itVarReached);
  const int r = var_rank_request > 0 ? std::min(var_rank_request, itVarRank) : itVarRank;
  *var_rank_out = r;
  if (R_out) {
    std::fill(R_out, R_out + (size_t)N * rank, 0.0);
    std::vector<double> col((size_t)N);
    for (int t = 0; t < itVarRank; ++t) {
      HIPCK(hipMemcpy(col.data(), itVR.get() + (size_t)t * N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
      for (long i = 0; i < N; ++i) R_out[(size_t)i * rank + t] = col[i];
    }
  }
  const double base = include_nugget ? sigma2 + nugget : sigma2;
  for (long c0 = 0; c0 < m; c0 += plan.points) {
    const long mc = std::min<long>(plan.points, m - c0);
    if (r < 1) {                                             // an empty cache: the prior variance
      std::fill(var + c0, var + c0 + mc, base);
      continue;
    }
    HIPCK(hipMemcpyAsync(dQ, testing + (size_t)c0 * D, (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, st));
    launch_local_scale(dQ, mc, D, dScale, dQs, st);
    launch_kvar(dQs, mc, dXs, N, D, kt, sigma2, itVR, N, r, base, dPart, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(var + c0, dPart, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
}

}  // namespace mogp
