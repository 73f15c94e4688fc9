// What engine.hip, engine_chol.hip, engine_fit.hip, engine_predict.hip, engine_hessian.hip, engine_local.hip, engine_iter*.hip and the analysis_*.hip units share and
// nobody else sees: small helpers and the process-wide diagnostic counters behind prof_counter (engine.hip).  What lives where: engine.hip the
// construction, the cached state, eval's steps, L^-1 / K^-1 and the gradient; engine_chol.hip the factorisation schedules; engine_fit.hip
// the optimiser, the slot pool, the replica engines and ScratchFactor; engine_predict.hip predict, full covariance, implausibility, Sobol and loo_variance;
// engine_hessian.hip the Hessian; engine_local.hip the LocalGP handle, which is no Engine: its design, local prediction and the Vecchia
// likelihood; engine_iter.hip the state of its iterative solver (IterSolver, iter_solver.h: the groups' reserve, the builds, the iteration)
// and the entry points kmatvec, precondition, solve, predict_exact and variance_bound; engine_iter_lik.hip loglik_exact.  The analyses that only read a fitted engine are
// free functions (analysis.h), one unit per subject: analysis_mixture.hip the mixture over hyperparameter samples, analysis_cv.hip
// cross-validation, analysis_sample.hip joint posterior draws, analysis_active.hip active learning (predict_cov, alc, alc_batch).
// Whoever needs "factor a batch of matrices I wrote myself" and nothing else of an engine (gkdr_R,
// cross_validate's k-fold path, sample_posterior) takes a ScratchFactor, below.
#pragma once
#include "engine.h"
#include "predict_plan.h"

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <memory>

namespace mogp {

inline int roundup(int x, int m) { return (x + m - 1) / m * m; }

// sets a flag for the lifetime of a scope (cleared again when the scope is left through an exception)
struct FlagGuard {
  bool& b;
  explicit FlagGuard(bool& f) : b(f) { b = true; }
  ~FlagGuard() { b = false; }
};

// bytes one chunk of a prediction may take (12 GB: one cross-covariance chunk for 64 x n=2000 x m=10^4)
inline double ks_budget_bytes() {
  static const double budget = [] { const char* e = getenv("MOGP_KS_BUDGET_GB"); return (e ? atof(e) : 12.0) * 1e9; }();
  return budget;
}

// A replica engine of `slots` slots with the inputs, kernel and mean function of `src`, for the lifetime of a scope (engine_fit.hip): the
// cached one of the device when its shape matches (taken out of the cache, its inputs reset), else a new one -- whatever the cache held
// is freed first.  When the scope is left normally the engine goes back into the cache (MOGP_REPLICA_CACHE=0: never); an exception
// destroys it.  `targets` (slots, n), nug_type and nug_size only initialise a NEW engine: every slot is given its emulator by
// Engine::retarget before it is used.  Shared by fit_map_from and predict_mixture (analysis_mixture.hip).
class ReplicaLease {
 public:
  ReplicaLease(const Engine& src, long slots, const std::vector<double>& targets, int nug_type, double nug_size);
  ~ReplicaLease();
  ReplicaLease(const ReplicaLease&) = delete;
  ReplicaLease& operator=(const ReplicaLease&) = delete;
  Engine* operator->() const { return rep.get(); }
  Engine& operator*() const { return *rep; }

 private:
  std::unique_ptr<Engine> rep;
  bool cache_on;
};

// A batch of `slots` caller-filled symmetric matrices of `rows` rows to factor with the engine's batched Cholesky, for the lifetime of a
// scope (engine_fit.hip).  It owns the engine that does it -- one dummy input column, zero targets, nugget type "fixed" with nugget 0 --
// and shows nothing else of it.  A slot's matrix has the layout of the covariance build (launch.h) at NP = scratch_np(rows), MS = NP * NP
// doubles apart; everything runs on stream().
class ScratchFactor {
 public:
  ScratchFactor(int rows, long slots);
  const int rows, slots;
  int NP;
  size_t MS;
  hipStream_t stream() const { return eng.stream; }
  // Every slot's matrix is written into the factor buffer by `fill` -- it stands where the covariance build does -- and factored with the
  // schedule of the regime; info (indexed by slot): 0 where the slot factorised.  The slots that did form L^-1 (linv(), lower triangle).
  // only: the slots to factor instead of all -- the others keep their factor and state, info is meaningful for the listed slots alone;
  // want_linv = false: L^-1 is not formed.
  void factor(const CovFill& fill, std::vector<int>& info, const std::vector<int>* only = nullptr, bool want_linv = true);
  // behind factor, for the slots that factorised: the log-determinant words (launch_logdet) and the solution rows (launch_alpha_from_linv)
  void logdet_and_solve(const std::vector<int>& okslots);
  // the buffers a caller hands to its own kernels
  double* factor_buffer() const { return eng.dA; }
  const double* linv() const { return eng.dLinv; }
  const double* solution() const { return eng.dAlpha; }
  const double* logdet_words() const { return eng.dRes; }
  const int* status() const { return eng.dInfo; }

 private:
  ScratchFactor(int rows, long slots, const std::vector<double>& zeros);
  Engine eng;
};

// One pass of queries of a LocalGP entry point (local prediction, the rectangular product, exact prediction, the variance bound): the
// raw and the scaled rows of up to `points` queries of D coordinates on the device.  points = 0: nothing is allocated.
struct QueryPass {
  QueryPass(size_t points, int D_) : D(D_) {
    if (points) raw.reserve(points * D), scaled.reserve(points * D);
  }
  // uploads rows [c0, c0 + mc) of `testing` (host, row-major) and scales them with dScale on st; the scaled rows
  const double* load(const double* testing, long c0, long mc, const double* dScale, hipStream_t st) {
    HIPCK(hipMemcpyAsync(raw, testing + (size_t)c0 * D, (size_t)mc * D * sizeof(double), hipMemcpyHostToDevice, st));
    launch_local_scale(raw, mc, D, dScale, scaled, st);
    return scaled;
  }

 private:
  const int D;
  DevBuf<double> raw, scaled;
};

// throws std::runtime_error(message) unless the `count` values at p are all finite
inline void require_finite(const double* p, size_t count, const char* message) {
  for (size_t k = 0; k < count; ++k)
    if (!std::isfinite(p[k])) throw std::runtime_error(message);
}

inline std::atomic<long long> g_bs_timeouts{0}, g_obj_evals{0}, g_grad_evals{0}, g_mc_aborts{0}, g_alpha_solves{0};
inline std::atomic<long long> g_lb_iters{0}, g_ls_short{0}, g_ls_long{0}, g_lb_runs{0}, g_pool_rounds{0}, g_pool_slot_rounds{0}, g_rep_build_us{0}, g_rep_pool_us{0}, g_retarget_us{0}, g_retargets{0}, g_rep_reused{0};
inline std::atomic<long long> g_inputs_restored{0};

}  // namespace mogp
