// The local-approximate-GP entries of the C ABI: a handle that keeps a large design on the device and predicts every query from its nearest
// design points alone (LocalGP, engine_local.hip).  No Engine is involved.
#include "capi_internal.h"

using namespace mogp;
using namespace mogp::capi;

struct mogp_local { std::unique_ptr<mogp::LocalGP> gp; };

extern "C" {

mogp_local* mogp_local_create(const double* inputs, long long N, int D, const double* residuals, int E, int device) {
  mogp_local* h = nullptr;
  const int status = guarded([&] {
    std::unique_ptr<mogp_local> p(new mogp_local);
    if (device < 0) hip_check(hipGetDevice(&device), "hipGetDevice");
    DeviceGuard g(device);
    p->gp.reset(new LocalGP(inputs, (long)N, D, residuals, E));
    h = p.release();
  });
  return status == 0 ? h : nullptr;
}

int mogp_local_predict(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, double jitter,
                       int include_nugget, const double* testing, int m, int D, int k, int max_points, double* mean_out, double* var_out,
                       int* ok_out, double* radius_out, int* neighbours_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("predict_local: null handle");
    if (D != h->gp->D) throw std::runtime_error("predict_local: testing points must have D columns");
    h->gp->predict(emulator, kernel_type, scale, sigma2, nugget, jitter, include_nugget != 0, testing, m, k, max_points, mean_out, var_out, ok_out,
                   radius_out, neighbours_out);
  });
}

int mogp_local_vecchia_neighbours(mogp_local* h, const double* scale, int k, int* neighbours_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("vecchia_neighbours: null handle");
    h->gp->vecchia_neighbours(scale, k, neighbours_out);
  });
}

int mogp_local_vecchia_loglik(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, double jitter, int k,
                              int want_grad, int max_points, double* value_out, double* grad_out, double* terms_out, int* ok_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("vecchia_loglik: null handle");
    h->gp->vecchia_loglik(emulator, kernel_type, scale, sigma2, nugget, jitter, k, want_grad != 0, max_points, value_out, grad_out, terms_out, ok_out);
  });
}

int mogp_local_kmatvec(mogp_local* h, int kernel_type, const double* scale, double sigma2, double nugget, const double* queries, int m, int D,
                       const double* V, int r, double* out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("kmatvec: null handle");
    if (queries && D != h->gp->D) throw std::runtime_error("kmatvec: queries must have D columns");
    h->gp->kmatvec(kernel_type, scale, sigma2, nugget, queries, m, V, r, out);
  });
}

int mogp_local_precondition(mogp_local* h, int kernel_type, const double* scale, double sigma2, double nugget, int rank, int* rank_out,
                            int* pivots_out, double* L_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("precondition: null handle");
    if (!rank_out) throw std::runtime_error("precondition: null pointer");
    *rank_out = h->gp->precondition(kernel_type, scale, sigma2, nugget, rank, pivots_out, L_out);
  });
}

int mogp_local_solve(mogp_local* h, const double* B, int c, double rtol, int max_iter, double* x_out, int* iterations_out, int* converged_out,
                     double* residual_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("solve: null handle");
    h->gp->solve(B, c, rtol, max_iter, x_out, iterations_out, converged_out, residual_out);
  });
}

int mogp_local_predict_exact(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, int rank, double rtol,
                             int max_iter, int include_nugget, const double* testing, int m, int D, int max_points, double* mean_out,
                             double* var_out, int* stat_out, double* residual_out, int* var_stat_out, double* var_residual_out,
                             double* alpha_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("predict_exact: null handle");
    if (m > 0 && D != h->gp->D) throw std::runtime_error("predict_exact: testing points must have D columns");
    h->gp->predict_exact(emulator, kernel_type, scale, sigma2, nugget, rank, rtol, max_iter, include_nugget != 0, testing, m, max_points, mean_out,
                         var_out, stat_out, residual_out, var_stat_out, var_residual_out, alpha_out);
  });
}

int mogp_local_loglik_exact(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, int rank, double rtol,
                            int max_iter, const double* g1, int g1_rows, const double* g2, int n_probes, int want_grad, double* scalars_out,
                            int* stat_out, double* residual_out, double* rho_out, double* uw_out, double* coef_out, double* forms_out,
                            double* forms_each_out, double* z_out, double* x_out, double* w_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("loglik_exact: null handle");
    h->gp->loglik_exact(emulator, kernel_type, scale, sigma2, nugget, rank, rtol, max_iter, g1, g1_rows, g2, n_probes, want_grad != 0, scalars_out,
                        stat_out, residual_out, rho_out, uw_out, coef_out, forms_out, forms_each_out, z_out, x_out, w_out);
  });
}

int mogp_local_variance_bound(mogp_local* h, int kernel_type, const double* scale, double sigma2, double nugget, int precond_rank,
                              int var_rank_request, int include_nugget, const double* testing, int m, int D, int max_points, double* var_out,
                              int* var_rank_out, double* R_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("variance_bound: null handle");
    if (m > 0 && D != h->gp->D) throw std::runtime_error("variance_bound: testing points must have D columns");
    h->gp->variance_bound(kernel_type, scale, sigma2, nugget, precond_rank, var_rank_request, include_nugget != 0, testing, m, max_points, var_out,
                          var_rank_out, R_out);
  });
}

int mogp_local_rff(mogp_local* h, const double* scale, const double* queries, int m, int D, const double* omega, const double* phase, int n_features,
                   const double* W, int n_draws, double amp, int max_points, double* out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("rff: null handle");
    if (D != h->gp->D) throw std::runtime_error("rff: queries and frequencies must have D columns");
    h->gp->rff(scale, queries, m, omega, phase, n_features, W, n_draws, amp, max_points, out);
  });
}

int mogp_local_sample_paths(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, int precond_rank,
                            double rtol, int max_iter, const double* omega, const double* phase, int n_features, int n_draws, double amp,
                            unsigned long long seed, unsigned stream, int first_draw, const double* W_in, const double* noise_in, double* W_out,
                            double* v_out, int* stat_out, double* residual_out, int* rank_out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("sample_paths: null handle");
    h->gp->sample_paths(emulator, kernel_type, scale, sigma2, nugget, precond_rank, rtol, max_iter, omega, phase, n_features, n_draws, amp, seed,
                        stream, first_draw, W_in, noise_in, W_out, v_out, stat_out, residual_out, rank_out);
  });
}

int mogp_local_kmatvec_inputderiv(mogp_local* h, int kernel_type, const double* scale, double sigma2, const double* queries, int m, int D,
                                  const double* V, int r, int max_points, double* out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("kmatvec_inputderiv: null handle");
    if (D != h->gp->D) throw std::runtime_error("kmatvec_inputderiv: queries must have D columns");
    h->gp->kmatvec_inputderiv(kernel_type, scale, sigma2, queries, m, V, r, max_points, out);
  });
}

int mogp_local_rff_inputderiv(mogp_local* h, const double* scale, const double* queries, int m, int D, const double* omega, const double* phase,
                              int n_features, const double* W, int n_draws, double amp, int max_points, double* out) {
  return guarded([&] {
    if (!h || !h->gp) throw std::runtime_error("rff_inputderiv: null handle");
    if (D != h->gp->D) throw std::runtime_error("rff_inputderiv: queries and frequencies must have D columns");
    h->gp->rff_inputderiv(scale, queries, m, omega, phase, n_features, W, n_draws, amp, max_points, out);
  });
}

void mogp_local_destroy(mogp_local* h) {
  if (!h) return;
  (void)guarded([&] {
    if (h->gp) {
      DeviceGuard g(h->gp->device_id());
      h->gp.reset();
    }
  });
  delete h;
}

}  // extern "C"
