// extern "C" surface of libmogp_hip.so (include/mogp_hip.h).  Every entry point converts C++
// exceptions into (non-zero status, thread-local message); the Python shim raises RuntimeError
// with that message, matching the std::runtime_error -> RuntimeError mapping of pybind11 in the
// reference (bindings.cu).  This unit: the error channel, version and device, mean functions, the stand-alone kernel objects, the
// measurement hooks and the mogp_dev_* helpers; DenseGP_GPU is capi_densegp.hip, MultiOutputGP_GPU capi_mogp.hip and capi_mogp_predict.hip;
// what they share is capi_internal.h.
#include "capi_internal.h"

using namespace mogp;
using namespace mogp::capi;

thread_local std::string mogp::capi::g_err;

static void kernel_eval_impl(int kernel_type, int what, const double* x1, int n1, const double* x2, int n2, int D, const double* params,
                             int n_params, double* out) {
  if (kernel_type < 0 || kernel_type > 4) throw std::runtime_error("Unrecognized kernel type\n");
  if (what < 0 || what > 2) throw std::runtime_error("kernel_eval: what must be 0 (f), 1 (deriv) or 2 (inputderiv)");
  if (n1 < 1 || n2 < 1 || D < 1) throw std::runtime_error("kernel inputs must have shape (n, D) with n, D >= 1");
  const bool uniform = kernel_type >= 3;
  const int nc = uniform ? 1 : D;
  if (n_params != nc + 1) throw std::runtime_error("Expected params list of length " + std::to_string(nc + 1));
  const int dk = kernel_type == 3 ? 0 : (kernel_type == 4 ? 1 : kernel_type);
  std::vector<double> P(D + 1);
  for (int d = 0; d < D; ++d) P[d] = std::exp(params[uniform ? 0 : d]);
  P[D] = std::exp(params[nc]);
  const size_t planes = what == 0 ? 1 : (what == 1 ? (size_t)D + 1 : (size_t)D);
  const size_t cnt = planes * (size_t)n1 * n2;
  DevBuf<double> d1((size_t)n1 * D), d2((size_t)n2 * D), dP(P.size()), dO(cnt);
  hip_check(hipMemcpy(d1, x1, (size_t)n1 * D * 8, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(d2, x2, (size_t)n2 * D * 8, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dP, P.data(), P.size() * 8, hipMemcpyHostToDevice), "hipMemcpy");
  launch_kernel_object(dk, d1, n1, d2, n2, D, dP, what, dO, nullptr);
  std::vector<double> tmp(cnt);
  hip_check(hipMemcpy(tmp.data(), dO, cnt * 8, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipGetLastError(), "kernel_object_kernel");
  if (what == 1 && uniform) {
    // one shared length scale: d/dtheta_0 = sum of the per-dimension planes (Kernel.py:338-376); then the sigma^2 plane
    const size_t pl = (size_t)n1 * n2;
    for (size_t e = 0; e < pl; ++e) {
      double s = 0.;
      for (int d = 0; d < D; ++d) s += tmp[(size_t)d * pl + e];
      out[e] = s;
      out[pl + e] = tmp[(size_t)D * pl + e];
    }
  } else {
    std::memcpy(out, tmp.data(), cnt * 8);
  }
}

extern "C" {

const char* mogp_last_error(void) { return g_err.c_str(); }
const char* mogp_version(void) { return "mogp-hip 0.1 (gfx950)"; }

int mogp_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}
int mogp_have_compatible_device(void) {
  int c = mogp_device_count();
  for (int d = 0; d < c; ++d) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, d) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) return 1;
  }
  return 0;
}
int mogp_set_device(int device) { return guarded([&] { hip_check(hipSetDevice(device), "hipSetDevice"); }); }

// ---- mean functions ---------------------------------------------------------------------------
mogp_meanfunc* mogp_meanfunc_zero(void) { auto* m = new mogp_meanfunc; m->mf.kind = 0; return m; }
mogp_meanfunc* mogp_meanfunc_fixed(double v) { auto* m = new mogp_meanfunc; m->mf.kind = 1; m->mf.value = v; return m; }
mogp_meanfunc* mogp_meanfunc_const(void) { auto* m = new mogp_meanfunc; m->mf.kind = 2; return m; }
mogp_meanfunc* mogp_meanfunc_poly(const int* dims, const int* powers, int nterms) {
  auto* m = new mogp_meanfunc;
  m->mf.kind = 3;
  m->mf.dims.assign(dims, dims + nterms);
  m->mf.powers.assign(powers, powers + nterms);
  return m;
}
void mogp_meanfunc_destroy(mogp_meanfunc* m) { delete m; }
int mogp_meanfunc_n_params(const mogp_meanfunc* m) { return m->mf.n_params(); }
int mogp_meanfunc_mean_f(const mogp_meanfunc* m, const double* xs, int mm, int D, const double* p, int np, double* out) {
  return guarded([&] { m->mf.mean_f(xs, mm, D, p, np, out); });
}
int mogp_meanfunc_mean_deriv(const mogp_meanfunc* m, const double* xs, int mm, int D, const double* p, int np, double* out) {
  return guarded([&] { m->mf.mean_deriv(xs, mm, D, p, np, out); });
}
int mogp_meanfunc_mean_inputderiv(const mogp_meanfunc* m, const double* xs, int mm, int D, const double* p, int np, double* out) {
  return guarded([&] { m->mf.mean_inputderiv(xs, mm, D, p, np, out); });
}
int mogp_pivot_cholesky(const double* A, int n, double* L_out, int* P_out, int* rank_out) {
  return guarded([&] { Engine::pivot_cholesky(A, n, L_out, P_out, rank_out); });
}
int mogp_set_fit_options(int max_iter, double ftol, double gtol, unsigned long long seed) {
  FitOptions& o = fit_options();
  if (max_iter > 0) o.max_iter = max_iter;
  if (ftol > 0) o.ftol = ftol;
  if (gtol > 0) o.gtol = gtol;
  o.seed = seed;
  return 0;
}

// ---- stand-alone kernel objects (bindings.cu:340-361, kernel.hpp:47-107) --------------------------------------
// kernel_type as in the enum (0 SqExp, 1 Matern52, 2 ProductMat52, 3 UniformSqExp, 4 UniformMat52); params = [corr_raw.., log sigma^2]
// (n_corr + 1 entries, n_corr = 1 for the uniform kernels); what = 0 kernel_f -> out (n1, n2), 1 kernel_deriv -> out
// (n_corr + 1, n1, n2), 2 kernel_inputderiv -> out (n2, n1, D) (the reference's flat order)
int mogp_kernel_eval(int kernel_type, int what, const double* x1, int n1, const double* x2, int n2, int D, const double* params, int n_params,
                     double* out) {
  return guarded([&] { kernel_eval_impl(kernel_type, what, x1, n1, x2, n2, D, params, n_params, out); });
}

int mogp_gkdr_R(const double* X, int n, int m, const double* y, int nx, const double* sgx2, int ny, const double* sgy2, double eps,
                int max_pairs_per_pass, double* R_out, int* info_out) {
  return guarded([&] { gkdr_R(X, n, m, y, nx, sgx2, ny, sgy2, eps, max_pairs_per_pass, R_out, info_out); });
}

int mogp_design_min_pdist(const double* designs, int T, int n, int D, double* out) {
  return guarded([&] { design_min_pdist(designs, T, n, D, out); });
}

int mogp_design_anneal_lhs(const int* start, int C, int n, int D, long long n_steps, int q, double theta0, double rho, long long stage,
                           unsigned long long seed, unsigned int stream, int* best_out, double* phi_out, long long* minr_out,
                           long long* pairs_out, long long* accepted_out) {
  return guarded([&] {
    design_anneal_lhs(start, C, n, D, n_steps, q, theta0, rho, stage, seed, stream, best_out, phi_out, minr_out, pairs_out, accepted_out);
  });
}

// ---- measurement hooks ----------------------------------------------------------------------------
int mogp_profile_enable(int on) { prof_enable(on != 0); return 0; }
int mogp_profile_reset(void) { prof_reset(); return 0; }
int mogp_profile_schedule(int schedule, int single_stream) {
  schedule_override().schedule = schedule;
  schedule_override().single_stream = single_stream != 0;
  return 0;
}
static int task_table_out(int n_plus_rhs, bool ahead, int* out, int capacity) {
  // host-only: the per-emulator task order of the one-launch Cholesky for a matrix of NP = roundup(n_plus_rhs, 128) rows
  const int NP = (n_plus_rhs + TILE - 1) / TILE * TILE;
  const std::vector<int> tb = mchol_task_table(NP, ahead);
  if (out)
    for (int i = 0; i < (int)tb.size() && i < capacity; ++i) out[i] = tb[i];
  return (int)tb.size();
}
int mogp_mchol_task_table(int n_plus_rhs, int* out, int capacity) { return task_table_out(n_plus_rhs, false, out, capacity); }
int mogp_mchol_task_table_ahead(int n_plus_rhs, int* out, int capacity) { return task_table_out(n_plus_rhs, true, out, capacity); }
int mogp_profile_counter(const char* name, long long* out) {
  const long long v = prof_counter(name);
  if (v < 0 || !out) {
    g_err = std::string("unknown counter ") + (name ? name : "(null)");
    return 1;
  }
  *out = v;
  return 0;
}
int mogp_profile_get(const char* tag, double* total_ms, long long* launches, double* alg_flops, double* alg_bytes) {
  return prof_get(tag, total_ms, launches, alg_flops, alg_bytes) ? 0 : 1;
}
void* mogp_dev_malloc(unsigned long long bytes) {
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { g_err = "hipMalloc failed"; return nullptr; }
  return p;
}
int mogp_dev_free(void* p) { return guarded([&] { hip_check(hipFree(p), "hipFree"); }); }
int mogp_dev_upload(void* d, const void* s, unsigned long long bytes) { return guarded([&] { hip_check(hipMemcpy(d, s, bytes, hipMemcpyHostToDevice), "upload"); }); }
int mogp_dev_download(void* d, const void* s, unsigned long long bytes) { return guarded([&] { hip_check(hipMemcpy(d, s, bytes, hipMemcpyDeviceToHost), "download"); }); }
int mogp_dev_synchronize(void) { return guarded([&] { hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize"); }); }

}  // extern "C"
