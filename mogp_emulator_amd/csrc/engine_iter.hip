// Iterative exact prediction on the LocalGP handle (engine.h): conjugate gradients on A = sigma2 k(X, X) + nugget I of the whole design,
// preconditioned by a partial pivoted Cholesky factor, with A never stored (kernels_iter.hip generates its entries as they are multiplied).
// First IterSolver (iter_solver.h): the groups' reserve -- the one place that frees their buffers and drops their keys --, the builds, the
// iteration, the dots and the kept alpha.  Then LocalGP's entry points, each as its steps: null pointers, the named refusals and the plan
// (predict_plan.h: plain arithmetic, checked on the host by tests/c/iter_plan_check.cpp), the calls on the solver, the copies.  The
// iteration is a host loop of plain launches bounded by max_iter; the step scalars and the frozen flags live on the device and the host
// looks at the flags every ITER_LOOK iterations.
#include "engine_internal.h"
#include "iter_panel.h"
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

// out (N, out_cols) row-major, zero-filled = the first `held` columns of the tall device factor F (ld N)
void download_columns(const double* F, long N, int held, int out_cols, double* out) {
  std::fill(out, out + (size_t)N * out_cols, 0.0);
  std::vector<double> col((size_t)N);
  for (int t = 0; t < held; ++t) {
    HIPCK(hipMemcpy(col.data(), F + (size_t)t * N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    panel_to_rows(out, (size_t)N, (size_t)out_cols, (size_t)t, 1, col.data(), (size_t)N, 0);
  }
}

}  // namespace

// ---- the groups: reserve is the one function that frees, and it drops the key of what it freed ------------------------------------------------
// (The key goes when ANY buffer grows.  N is fixed for a handle, so every buffer sized by the rank grows exactly when L does: the same
// rule as "when the factor grows", written so that it cannot miss a buffer.)
void IterSolver::Precond::reserve(long N, int rank) {
  const size_t n = (size_t)N, p = (size_t)std::max(rank, 1), segs = (n + ITER_SEG - 1) / ITER_SEG, blk = (n + 1023) / 1024;
  bool freed = grow(L, n * p);
  freed |= grow(G, p * p);
  freed |= grow(diag, n);
  freed |= grow(dmax, p);
  freed |= grow(piv, p);
  freed |= grow(state, 2);
  freed |= grow(pval, blk);
  freed |= grow(pidx, blk);
  freed |= grow(wpart, segs * p * ITER_COLS);
  freed |= grow(w, p * ITER_COLS);
  freed |= grow(w2, p * ITER_COLS);
  if (freed) drop();
}

void IterSolver::CgPanels::reserve(long N) {
  const size_t n = (size_t)N, dots = (n + ITER_DOT_BLOCK - 1) / ITER_DOT_BLOCK;
  for (DevBuf<double>* panel : {&b, &x, &xl, &r, &p, &q, &z, &v}) grow(*panel, n * ITER_COLS);
  grow(part, dots * ITER_COLS);
  grow(sc, 5 * ITER_COLS);
  grow(fl, 3 * ITER_COLS);
}

void IterSolver::VarCache::reserve(long N, int rank) {
  const size_t pad = (size_t)iter_var_pad(rank);
  bool freed = grow(R, (size_t)N * pad);
  freed |= grow(T, pad * pad);
  if (freed) drop();
}

void IterSolver::LikScratch::reserve(long N, int D, int rank, int max_iter) {
  const size_t n = (size_t)N;
  grow(W, n * ITER_COLS);
  grow(log, (size_t)2 * ITER_COLS * max_iter);
  grow(g1, (size_t)ITER_COLS * std::max(rank, 1));
  grow(part, (n + 63) / 64 * 2 * D);
  grow(out, (size_t)ITER_COLS * 2 * D);
}

void IterSolver::reserve(const char* who, int rank) {
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  iter_check_memory(who, design.N, rank, (double)free_b, held());   // what the handle holds of it already is reused, hence counts as free
  pre.reserve(design.N, rank);
  cg.reserve(design.N);
}

void IterSolver::build(const IterKey& k, hipStream_t st) {
  if (pre.holds(k)) return;
  pre.drop();
  const long N = design.N;
  int state[2] = {0, 0};
  if (k.rank > 0) {
    launch_pchol_init(pre.diag, N, k.sigma2, pre.state, st);
    for (int t = 0; t < k.rank; ++t)
      launch_pchol_step(design.Xs, N, design.D, k.kt, k.sigma2, t, pre.L, pre.diag, pre.piv, pre.dmax, pre.state, pre.pval, pre.pidx, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(state, pre.state, sizeof(state), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
  const int p = state[0];
  double logdet = 0.;
  if (p > 0) {
    launch_pchol_gram(pre.L, N, p, k.nugget, pre.G, st);
    HIPCK(hipGetLastError());
    std::vector<double> G((size_t)p * p);
    HIPCK(hipMemcpyAsync(G.data(), pre.G, G.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    logdet = spd_inverse(G, p);
    HIPCK(hipMemcpyAsync(pre.G, G.data(), G.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  pre.built(k, p, logdet);
}

void IterSolver::solve(int cols, double rtol, int max_iter, int* it_out, int* cv_out, double* rs_out, hipStream_t st, double* first_z,
                       double* coef_log) {
  const long N = design.N;
  const int D = design.D;
  const size_t panel_bytes = (size_t)N * ITER_COLS * sizeof(double);
  const IterKey& k = pre.key();
  const bool pc = pre.rank() > 0;
  // Columns >= cols of cg.b are zero and freeze at iteration 0, so with at most 16 live columns the product serves one block of 16 alone.
  // A column's bits do not depend on that: the product keeps its columns apart.  (The columns it then skips hold zeros, not stale data.)
  const int nb = cols > 16 ? 2 : 1;
  if (nb == 1) HIPCK(hipMemsetAsync(cg.q, 0, panel_bytes, st));
  double* z = pc ? cg.z.get() : cg.r.get();                  // plain CG: z = r
  auto apply = [&] {
    if (pc) launch_precond_apply(pre.L, N, pre.rank(), pre.G, k.nugget, cg.r, cg.z, pre.wpart, pre.w, pre.w2, st);
  };
  auto dot = [&](CgStep step, const double* a, const double* b, int it) {
    launch_cg_dot(a, b, N, cg.part, st);
    launch_cg_scalars(step, cg.part, N, cg.sc, cg.fl, it, rtol, st, coef_log);
  };
  HIPCK(hipMemsetAsync(cg.x, 0, panel_bytes, st));
  HIPCK(hipMemsetAsync(cg.xl, 0, panel_bytes, st));
  HIPCK(hipMemcpyAsync(cg.r, cg.b, panel_bytes, hipMemcpyDeviceToDevice, st));
  dot(CG_BB, cg.b, cg.b, 0);
  apply();
  if (first_z) HIPCK(hipMemcpyAsync(first_z, z, panel_bytes, hipMemcpyDeviceToDevice, st));
  dot(CG_RZ, cg.r, z, 0);
  launch_cg_direction(cg.p, z, N, true, cg.sc, cg.fl, st);
  int fl[3 * ITER_COLS];
  for (int it = 0; it < max_iter; ++it) {
    launch_kmatvec(design.Xs, N, design.Xs, N, D, k.kt, k.sigma2, k.nugget, true, cg.p, N, nb, cg.q, N, st);
    dot(CG_ALPHA, cg.p, cg.q, it);
    launch_cg_update(cg.x, cg.xl, cg.r, cg.p, cg.q, N, cg.sc, cg.fl, st);
    dot(CG_TEST, cg.r, cg.r, it);
    apply();
    dot(CG_BETA, cg.r, z, it);
    launch_cg_direction(cg.p, z, N, false, cg.sc, cg.fl, st);
    HIPCK(hipGetLastError());
    if ((it + 1) % ITER_LOOK == 0 && it + 1 < max_iter) {
      HIPCK(hipMemcpyAsync(fl, cg.fl, ITER_COLS * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      if (std::all_of(fl, fl + ITER_COLS, [](int f) { return f != 0; })) break;
    }
  }
  launch_panel_add(cg.x, cg.xl, N, st);                        // the iterate is x + xl: rounded once, here
  // the true residual, from one further product
  launch_kmatvec(design.Xs, N, design.Xs, N, D, k.kt, k.sigma2, k.nugget, true, cg.x, N, nb, cg.q, N, st);
  launch_panel_sub(cg.b, cg.q, N, cg.r, st);
  dot(CG_OUT, cg.r, cg.r, 0);
  HIPCK(hipGetLastError());
  double sc[5 * ITER_COLS];
  HIPCK(hipMemcpyAsync(fl, cg.fl, sizeof(fl), hipMemcpyDeviceToHost, st));
  HIPCK(hipMemcpyAsync(sc, cg.sc, sizeof(sc), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  for (int c = 0; c < ITER_COLS; ++c) {
    const bool frozen = fl[c] != 0;
    it_out[c] = frozen ? fl[2 * ITER_COLS + c] : max_iter;
    cv_out[c] = frozen ? fl[ITER_COLS + c] : 0;
    const double bb = sc[c], rr = sc[4 * ITER_COLS + c];
    rs_out[c] = bb == 0.0 ? 0.0 : std::sqrt(rr) / std::sqrt(bb);
  }
}

void IterSolver::dots(const double* a, const double* b, double* out, hipStream_t st) {
  launch_cg_dot(a, b, design.N, cg.part, st);
  launch_cg_scalars(CG_OUT, cg.part, design.N, cg.sc, cg.fl, 0, 0., st);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(out, cg.sc.get() + 4 * ITER_COLS, ITER_COLS * sizeof(double), hipMemcpyDeviceToHost, st));
}

IterSolver::KeptAlpha& IterSolver::alpha_of(int e) {
  if (alpha.size() != (size_t)design.E) alpha.assign(design.E, KeptAlpha());
  return alpha[e];
}

void IterSolver::keep_alpha(int e, const IterKey& k, int iterations, int converged, double residual, hipStream_t st) {
  KeptAlpha& a = alpha_of(e);
  a.key = IterKey();
  a.alpha.resize((size_t)design.N);
  HIPCK(hipMemcpyAsync(a.alpha.data(), cg.x, (size_t)design.N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCK(hipStreamSynchronize(st));
  a.iterations = iterations, a.converged = converged, a.residual = residual;
  a.key = k;
}

// The cache of the variance bound: R (N, r) with span R = span L and R^T A R = I, in two orthonormalisations so that no matrix worse
// conditioned than A is factorised (chol(L^T A L) directly would meet cond(A) cond(L)^2):
//   G0 = L^T L,  G0[:r0, :r0] = C0 C0^T (a prefix, stopped where L's columns become dependent),  Q = L[:, :r0] C0^-T   (Q^T Q = I)
//   H = Q^T (A Q) one panel of 32 columns at a time,  H = C C^T (a prefix, stopped at a pivot <= 0),  R = Q[:, :r] C^-T
// Both triangular factors are prefixes, so R[:, :r'] is the cache of every smaller rank r'.
void IterSolver::var_build(const IterKey& k, hipStream_t st) {
  if (var.holds(k)) return;
  var.drop();
  const long N = design.N;
  const int p = pre.rank();
  const int pad = (int)iter_var_pad(std::max(p, 1));
  int r = 0;
  if (p > 0) {
    HIPCK(hipMemsetAsync(var.R, 0, (size_t)N * pad * sizeof(double), st));       // (the product with A reads whole panels of 32 columns)
    launch_pchol_gram(pre.L, N, p, 0., var.T, st);
    HIPCK(hipGetLastError());
    std::vector<double> G((size_t)p * p), C, T;
    HIPCK(hipMemcpyAsync(G.data(), var.T, G.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    const int r0 = prefix_cholesky(G.data(), p, ITER_VAR_TAU * G[0], C);
    if (r0 > 0) {
      upper_inverse(C.data(), p, r0, T, pad);
      HIPCK(hipMemcpyAsync(var.T, T.data(), (size_t)r0 * pad * sizeof(double), hipMemcpyHostToDevice, st));
      for (int c0 = 0; c0 < r0; c0 += ITER_COLS) launch_tri_right(pre.L, N, r0, var.T, pad, c0, var.R, st);
      HIPCK(hipGetLastError());
      std::vector<double> H((size_t)r0 * r0), w((size_t)r0 * ITER_COLS);
      for (int b0 = 0; b0 < r0; b0 += ITER_COLS) {
        launch_kmatvec(design.Xs, N, design.Xs, N, design.D, k.kt, k.sigma2, k.nugget, true, var.R.get() + (size_t)b0 * N, N, 2, cg.q, N, st);
        launch_ltv(var.R, N, r0, cg.q, pre.wpart, pre.w, st);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(w.data(), pre.w, w.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (int a = 0; a < r0; ++a)
          for (int c = 0; c < ITER_COLS && b0 + c < r0; ++c) H[(size_t)a * r0 + b0 + c] = w[(size_t)a * ITER_COLS + c];
      }
      for (int a = 0; a < r0; ++a)
        for (int b = 0; b < a; ++b) H[(size_t)a * r0 + b] = H[(size_t)b * r0 + a] = 0.5 * (H[(size_t)a * r0 + b] + H[(size_t)b * r0 + a]);
      r = prefix_cholesky(H.data(), r0, 0., C);
      if (r > 0) {
        upper_inverse(C.data(), r0, r, T, pad);
        HIPCK(hipMemcpyAsync(var.T, T.data(), (size_t)r * pad * sizeof(double), hipMemcpyHostToDevice, st));
        for (int c0 = ((r - 1) / ITER_COLS) * ITER_COLS; c0 >= 0; c0 -= ITER_COLS) launch_tri_right(var.R, N, r, var.T, pad, c0, var.R, st);   // in place: descending
        HIPCK(hipGetLastError());
        HIPCK(hipStreamSynchronize(st));                     // (T is a local)
      }
    }
  }
  var.built(k, r, p);
}

// ---- the handle's entry points ----------------------------------------------------------------------------------------------------------------
void LocalGP::precondition_for(const IterKey& k, hipStream_t st) {
  ensure_scaled(k.scale.data(), st);
  iter.build(k, st);
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
  DevBuf<double> dV((size_t)N * wide), dO((size_t)M * wide);
  QueryPass pass(queries ? (size_t)M : 0, D);
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  const double* rows = queries ? pass.load(queries, 0, M, dScale, st) : dXs.get();
  std::vector<double> hv((size_t)N * wide), ho((size_t)M * wide);
  for (int c0 = 0; c0 < r; c0 += ITER_COLS) {
    const int cols = std::min(ITER_COLS, r - c0), nb = cols > 16 ? 2 : 1;
    std::fill(hv.begin(), hv.end(), 0.0);
    rows_to_panel(V, (size_t)N, (size_t)r, (size_t)c0, (size_t)cols, hv.data(), (size_t)N, 0);
    HIPCK(hipMemcpyAsync(dV, hv.data(), (size_t)N * 16 * nb * sizeof(double), hipMemcpyHostToDevice, st));
    launch_kmatvec(rows, M, dXs, N, D, kt, sigma2, nugget, !queries, dV, N, nb, dO, M, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(ho.data(), dO, (size_t)M * 16 * nb * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    panel_to_rows(out, (size_t)M, (size_t)r, (size_t)c0, (size_t)cols, ho.data(), (size_t)M, 0);
  }
}

void LocalGP::kmatvec_inputderiv(int kt, const double* scale, double sigma2, const double* queries, long m, const double* V, int r, int max_points,
                                 double* out) {
  const std::string who = "kmatvec_inputderiv";
  if (!scale || !queries || !V || !out) throw std::runtime_error("kmatvec_inputderiv: null pointer");
  local_check_kernel(who, kt);
  local_check_hyper(who, D, scale, sigma2, 0., 0.);
  if (r < 1) throw std::runtime_error("kmatvec_inputderiv: at least one column is needed");
  if (m < 1 || m > INT_MAX) throw std::runtime_error("kmatvec_inputderiv: at least one query is needed");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const InderivPlan plan = kinderiv_plan(who, m, D, N, r, (double)free_b, max_points);
  const size_t P = (size_t)plan.points, n = (size_t)N, wide = (size_t)D * ITER_COLS;
  DevBuf<double> dV(n * ITER_COLS), dO(P * wide);
  QueryPass pass(P, D);
  SyncOnUnwind sync{st};
  ensure_scaled(scale, st);
  std::vector<double> hv(n * ITER_COLS), ho(P * wide);
  for (int c0 = 0; c0 < r; c0 += ITER_COLS) {
    const int cols = std::min(ITER_COLS, r - c0), nb = cols > 16 ? 2 : 1;
    std::fill(hv.begin(), hv.end(), 0.0);                    // the columns behind `cols` of the last block are exact zeros
    rows_to_panel(V, n, (size_t)r, (size_t)c0, (size_t)cols, hv.data(), n, 0);
    HIPCK(hipMemcpyAsync(dV, hv.data(), n * 16 * nb * sizeof(double), hipMemcpyHostToDevice, st));
    for (long p0 = 0; p0 < m; p0 += plan.points) {
      const long mc = std::min<long>(plan.points, m - p0);
      const double* rows = pass.load(queries, p0, mc, dScale, st);
      launch_kinderiv(rows, mc, dXs, N, D, kt, sigma2, dScale, dV, N, nb, dO, mc, st);
      HIPCK(hipGetLastError());
      HIPCK(hipMemcpyAsync(ho.data(), dO, (size_t)mc * D * 16 * nb * sizeof(double), hipMemcpyDeviceToHost, st));
      HIPCK(hipStreamSynchronize(st));
      // dimension d is the panel of the columns [16 nb d, 16 nb d + cols) and the window [c0, c0 + cols) of the rows out[p0 + i][d][.]
      for (int d = 0; d < D; ++d)
        panel_to_rows(out + ((size_t)p0 * D + d) * r, (size_t)mc, (size_t)D * r, (size_t)c0, (size_t)cols, ho.data(), (size_t)mc, (size_t)d * 16 * nb);
    }
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
  iter.reserve(who, rank);
  precondition_for(make_key(kt, scale, D, sigma2, nugget, rank), st);
  const int reached = iter.pre.rank();
  if (piv_out) {
    std::fill(piv_out, piv_out + rank, 0);
    if (reached > 0) HIPCK(hipMemcpy(piv_out, iter.pre.piv, (size_t)reached * sizeof(int), hipMemcpyDeviceToHost));
  }
  if (L_out) download_columns(iter.pre.L, N, reached, rank, L_out);
  return reached;
}

void LocalGP::solve(const double* B, int c, double rtol, int max_iter, double* x, int* iterations, int* converged, double* residual) {
  const char* who = "solve";
  if (!B || !x || !iterations || !converged || !residual) throw std::runtime_error("solve: null pointer");
  iter_check_solve(who, c, rtol, max_iter);
  if (!iter.pre.any()) throw std::runtime_error("solve: precondition has not been called");
  DeviceGuard guard(device);
  hipStream_t st = nullptr;
  SyncOnUnwind sync{st};
  const IterKey k = iter.pre.key();
  precondition_for(k, st);                                   // (the scaled design may have been formed for other scales since)
  std::vector<double> hb((size_t)N * ITER_COLS);
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  for (int c0 = 0; c0 < c; c0 += ITER_COLS) {
    const int cols = std::min(ITER_COLS, c - c0);
    std::fill(hb.begin(), hb.end(), 0.0);
    rows_to_panel(B, (size_t)N, (size_t)c, (size_t)c0, (size_t)cols, hb.data(), (size_t)N, 0);
    HIPCK(hipMemcpyAsync(iter.cg.b, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice, st));
    iter.solve(cols, rtol, max_iter, it, cv, rs, st);
    HIPCK(hipMemcpy(hb.data(), iter.cg.x, hb.size() * sizeof(double), hipMemcpyDeviceToHost));
    panel_to_rows(x, (size_t)N, (size_t)c, (size_t)c0, (size_t)cols, hb.data(), (size_t)N, 0);
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
  const IterKey k = make_key(kt, scale, D, sigma2, nugget, rank);
  iter.reserve(who, rank);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const IterPlan plan = iter_plan(who, std::max<long>(m, 1), D, (double)free_b, max_points);
  const size_t P = (size_t)plan.points;
  QueryPass pass(P, D);
  DevBuf<double> dOut(P * 16), dEye((size_t)ITER_COLS * ITER_COLS);
  SyncOnUnwind sync{st};
  precondition_for(k, st);
  IterSolver::CgPanels& cg = iter.cg;
  int it[ITER_COLS], cv[ITER_COLS];
  double rs[ITER_COLS];
  // alpha of this emulator: kept while everything it depends on stays
  IterKey ak = k;
  ak.rtol = rtol, ak.max_iter = max_iter;
  if (!(iter.alpha_of(e).key == ak)) {
    HIPCK(hipMemsetAsync(cg.b, 0, (size_t)N * ITER_COLS * sizeof(double), st));
    HIPCK(hipMemcpyAsync(cg.b, dY.get() + (size_t)e * N, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, st));
    iter.solve(1, rtol, max_iter, it, cv, rs, st);
    iter.keep_alpha(e, ak, it[0], cv[0], rs[0], st);
  }
  const IterSolver::KeptAlpha& a = iter.alpha_of(e);
  stat_i[0] = a.iterations, stat_i[1] = a.converged, stat_r[0] = a.residual;
  if (alpha_out) std::copy(a.alpha.begin(), a.alpha.end(), alpha_out);
  if (m == 0) return;
  // alpha as column 0 of a panel of 16 (the others zero): the rectangular product's V
  HIPCK(hipMemsetAsync(cg.v, 0, (size_t)N * 16 * sizeof(double), st));
  HIPCK(hipMemcpyAsync(cg.v, a.alpha.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, st));
  if (var) {
    std::vector<double> eye((size_t)ITER_COLS * ITER_COLS, 0.0);
    for (int c = 0; c < ITER_COLS; ++c) eye[(size_t)c * ITER_COLS + c] = 1.0;
    HIPCK(hipMemcpyAsync(dEye, eye.data(), eye.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));
  }
  const double var_add = include_nugget ? nugget : 0.;
  for (long c0 = 0; c0 < m; c0 += plan.points) {
    const long mc = std::min<long>(plan.points, m - c0);
    const double* dQs = pass.load(testing, c0, mc, dScale, st);
    launch_kmatvec(dQs, mc, dXs, N, D, kt, sigma2, 0., false, cg.v, N, 1, dOut, mc, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(mean + c0, dOut, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (!var) continue;
    for (long b0 = 0; b0 < mc; b0 += ITER_COLS) {
      const int nq = (int)std::min<long>(ITER_COLS, mc - b0);
      // the cross columns sigma2 k(X, q): the rectangular product with the design as rows, the queries as columns and V = I; columns
      // >= nq of the panel are exact zeros and freeze at iteration 0
      launch_kmatvec(dXs, N, dQs + (size_t)b0 * D, nq, D, kt, sigma2, 0., false, dEye, ITER_COLS, 2, cg.b, N, st);
      iter.solve(nq, rtol, max_iter, it, cv, rs, st);
      double kz[ITER_COLS];
      iter.dots(cg.b, cg.x, kz, st);
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
  const IterKey k = make_key(kt, scale, D, sigma2, nugget, rank);
  size_t free_b = 0, total_b = 0;
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  iter_var_check_memory(who, N, rank, (double)free_b, iter.held() + iter.var.bytes());
  iter.reserve(who, rank);
  iter.var.reserve(N, rank);
  HIPCK(hipMemGetInfo(&free_b, &total_b));
  const IterPlan plan = iter_plan(who, std::max<long>(m, 1), D, (double)free_b, max_points);
  const size_t P = (size_t)plan.points;
  QueryPass pass(P, D);
  DevBuf<double> dPart(P * 16);
  SyncOnUnwind sync{st};
  if (iter.var.holds(k)) {
    ensure_scaled(k.scale.data(), st);                       // the cache stands for itself: the preconditioner held may be another's
  } else {
    precondition_for(k, st);
    iter.var_build(k, st);
  }
  iter_var_check_rank(who, var_rank_request, iter.var.reached());
  const int r = var_rank_request > 0 ? std::min(var_rank_request, iter.var.rank()) : iter.var.rank();
  *var_rank_out = r;
  if (R_out) download_columns(iter.var.R, N, iter.var.rank(), rank, R_out);
  const double base = include_nugget ? sigma2 + nugget : sigma2;
  for (long c0 = 0; c0 < m; c0 += plan.points) {
    const long mc = std::min<long>(plan.points, m - c0);
    if (r < 1) {                                             // an empty cache: the prior variance
      std::fill(var + c0, var + c0 + mc, base);
      continue;
    }
    launch_kvar(pass.load(testing, c0, mc, dScale, st), mc, dXs, N, D, kt, sigma2, iter.var.R, N, r, base, dPart, st);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(var + c0, dPart, (size_t)mc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
  }
}

}  // namespace mogp
