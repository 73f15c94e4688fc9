// Engine: B independent zero/parametric-mean GPs that share one input matrix X, resident on one
// MI355X.  It is the device-side state behind both DenseGP_GPU (B = 1, densegp_gpu.hpp:36-123) and
// MultiOutputGP_GPU (B = n_emulators, multioutputgp_gpu.hpp:35-287).  Where the reference loops
// over emulators with OpenMP and serialises them on the default stream, every operation here is
// ONE batched launch sequence over an index list of emulators.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <random>
#include <string>
#include <map>
#include <vector>

#include "devmem.h"
#include "gp_state.h"
#include "hostmath.h"
#include "iter_solver.h"
#include "launch.h"

namespace mogp {

void hip_check(hipError_t e, const char* what);

// Makes `device` the calling thread's current HIP device and gives the caller's back when it goes out of scope.  HIP's current
// device belongs to each host thread, so every entry that touches an engine runs under one for the engine's device.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) hip_check(hipSetDevice(device), "hipSetDevice");
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

class ScratchFactor;   // engine_internal.h
// what build_cov runs instead of the covariance build when a factorisation is given one (ScratchFactor::factor): it writes every slot's
// matrix into the factor buffer, with the layout of the covariance build (launch.h)
using CovFill = std::function<void(const BatchView&)>;

class Engine {
 public:
  // analytic_mean: the coefficients of a const / polynomial mean are integrated out analytically (CPU
  // GaussianProcess semantics) instead of living in theta (reference GPU semantics)
  Engine(const double* X, int n, int D, const double* targets, int B, unsigned testing_size, const MeanFunc& mean,
         int kernel_type, int nug_type, double nug_size, bool analytic_mean = false);
  ~Engine();
  Engine(const Engine&) = delete;

  int n, D, NP, LD, PS, B, kernel_type;
  // kernel_type: 0 SquaredExponential, 1 Matern52 (reference enum, types.hpp:29-35) and the CPU-only kernels of
  // Kernel.py:946-997: 2 ProductMat52, 3 UniformSqExp, 4 UniformMat52.  NC = number of correlation parameters
  // (1 for the uniform kernels, which run the device kernels 0 / 1 with one shared length scale).
  int NC = 0;
  bool uniform() const { return kernel_type == 3 || kernel_type == 4; }
  int device_kernel() const { return kernel_type == 3 ? 0 : (kernel_type == 4 ? 1 : kernel_type); }
  size_t MS;
  unsigned testing_size;
  MeanFunc mean;
  std::vector<GPState> gp;
  std::vector<double> hX, hT;    // host copies (inputs()/targets())

  bool analytic = false;
  int q = 0, R = 1, RA = 1;      // analytic mean columns, right-hand-side rows (1 + q), rows of alpha per emulator
  // MeanPriors(mean = b, cov = B) of emulator i: b (q), B^-1 (q x q), B^-1 b (q), log|B|; q_in = 0 resets to weak
  void set_mean_priors(int i, int q_in, const double* b, const double* Binv, const double* Binvb, double logdetB);
  int n_mean() const { return analytic ? 0 : mean.n_params(); }
  int n_data(int i) const { return NC + 1 + (gp[i].nug_type == NUG_FIT ? 1 : 0); }
  int n_theta(int i) const { return n_mean() + n_data(i); }
  double nugget_size(int i) const;

  // Batched objective (+ gradient) at per-emulator thetas (full vectors [mean | data]).
  // ok[k] = 1 when the factorisation succeeded.  Never throws for numerical failure.
  // The objective needs log det K and |L^-1 t|^2 only, and the factorisation leaves both behind: without want_grad alpha = K^-1 t is NOT
  // solved (GPState::alpha stays false) -- whoever reads it asks ensure_alpha first.  With the analytic mean or nugget="pivot" it is solved
  // at once, as it is with want_grad (under the triangular inversion).
  void eval(const std::vector<int>& ids, const std::vector<const double*>& thetas, bool want_grad, double* f, double* grad,
            int grad_ld, int* ok);
  // fit(theta) for one emulator: throws std::runtime_error on failure (densegp_gpu.hpp:556-570).  An objective-only eval: the factor,
  // y = L^-1 t and the log-posterior are there afterwards, alpha when it is first asked for.
  void fit_one(int i, const double* theta, int len);
  void grad_current(const std::vector<int>& ids, double* grad, int grad_ld);

  // predictions for emulators `ids` (must be fitted). Xs host (m, D) unless xs_on_device.
  // means/vars: (ids.size(), m) row-major with leading dimension out_ld, derivs (ids.size(), m, D) or null; host unless
  // out_on_device.  Mean-function terms (parametric or analytic) are added on the device either way.
  void predict(const std::vector<int>& ids, const double* Xs, int m, bool xs_on_device, double* means, double* vars,
               long out_ld, bool out_on_device, double* derivs);

  void get_K(int i, double* out);
  // HistoryMatching.get_implausibility (HistoryMatching.py:197-276) fused behind the batched prediction:
  // obs / obs_var / discrepancy per entry of ids; out (m) host.  Query points are processed in device chunks.
  void implausibility(const std::vector<int>& ids, const double* Xs, int m, const double* obs, const double* obs_var,
                      const double* discrepancy, bool include_nugget, int rank, double* out);
  // the same for one part of a multi-part model: per query point the `keep` largest implausibilities of emulators `ids`, list r at
  // out[r * out_ld + j] in device memory of device `out_device` (-inf where there are fewer); no rank checks (the caller's)
  void implausibility_top(const std::vector<int>& ids, const double* Xs, int m, const double* obs, const double* obs_var,
                          const double* discrepancy, bool include_nugget, int keep, double* out, long out_ld, int out_device);
  // Sobol sensitivity indices of the predictive means of emulators `ids` (kernels_sobol.hip): A, B host (N, D) sample matrices;
  // S, ST (ids.size(), D), mean / variance (ids.size()) and -- with unc -- emulator_variance (ids.size(), the mean predictive variance
  // over A and B, as predict() reports it) are host buffers.  AB_i exists only as one chunk in device memory.
  void sobol(const std::vector<int>& ids, const double* A, const double* B, long N, bool unc, bool include_nugget, double* S, double* ST,
             double* mean_out, double* var_out, double* emvar_out);
  // Hessian of the negative log-posterior at thetas[k] of emulator ids[k] (kernels_hess.hip): H holds one ld x ld row-major block per
  // entry, the leading n_theta x n_theta block filled; ok[k] = 0 and NaN where the factorisation fails.  Throws for what it does not
  // cover (nugget="pivot", analytic mean, mean parameters in theta, ProductMat52).  The cached state of a fitted emulator is kept.
  void hessian(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, int* ok);
  // leave-one-out predictive variance of emulator i at its own training inputs (MICEFastGP.fast_predict for every index)
  void loo_variance(int i, double* out);
  // predict(full_cov=True), GaussianProcess.py:899-911: means (nb, m), covs (nb, m, m) host buffers, nugget NOT included
  void predict_full_cov(const std::vector<int>& ids, const double* Xs, int m, double* means, double* covs);
  void get_invQ(int i, double* out);
  void get_invQt(int i, double* out);
  void get_chol(int i, double* out);
  // pivot order P of the last fit (A[P][:, P] = L L^T, ChoInvPivot.P); identity for the other nugget types
  void get_pivot(int i, int* perm_out, int* rank_out);
  // pivot_cholesky(A) of linalg/cholesky.py:284-327 for an arbitrary symmetric matrix (host buffers, row-major)
  static void pivot_cholesky(const double* A, int n, double* L_out, int* P_out, int* rank_out);

  // multi-start MAP fit of emulators `ids` (fitting.hpp:61-128): all (emulator, start) runs through one slot pool
  void fit_map(const std::vector<int>& ids, int n_tries, const double* theta0, int theta0_len);
  // starting points x0[s][e] of a multi-start fit of emulators `emus` (engine, index): start 0 = theta0 if given, every other one
  // drawn from the emulator's priors with `rng`, in (start, emulator) order -- what fit_map draws from the engine's own rng
  using Starts = std::vector<std::vector<std::vector<double>>>;
  static Starts draw_starts(std::mt19937_64& rng, const std::vector<std::pair<const Engine*, int>>& emus, int n_tries, const double* theta0,
                            int theta0_len);
  // fit_map from given starting points x0[s][e] of emulator ids[e] (n_tries = x0.size())
  void fit_map_from(const std::vector<int>& ids, const Starts& x0);
  std::mt19937_64& random() { return rng; }
  int device_id() const { return device; }
  // the optimiser runs as a slot pool on emulators `slots` of this engine: next(pos, x0, tag) hands slot `pos` its next run (false: none
  // left), done(tag, f, x) receives a run's end point (f = +inf, x empty: failed)
  void run_pool(const std::vector<int>& slots, const std::function<bool(int, std::vector<double>&, int&)>& next,
                const std::function<void(int, double, const std::vector<double>&)>& done);
  // slot `slot` of this (replica) engine takes targets, nugget type and priors of emulator i of `src`
  void retarget(int slot, const Engine& src, int i);
  // new training inputs of the same shape (a cached replica engine taken by another fit): X, the analytic mean's design
  // matrix and every slot's pivot-ordered copy of the inputs
  void reset_inputs(const std::vector<double>& X);

  // For the analyses (analysis.h): bring cached state into being, select a group, launch on it.
  // what cross_validate, sample_posterior, predict_cov and alc refuse alike, as `who`: an emulator without a factor, the analytic mean
  // (`analytic_reason`: why the caller cannot cover it) and nugget="pivot"
  void require_plain_fit(const char* who, const std::vector<int>& ids, const char* analytic_reason) const;
  // alpha of the emulators of ids that hold a factor but not yet alpha: the one-launch chain on `stream`, its time-out words read back
  // (one small copy and synchronisation of its own), the repeat with the multi-launch path where a wait gave up
  void ensure_alpha(const std::vector<int>& ids);
  void ensure_linv(const std::vector<int>& ids);
  void ensure_kinv(const std::vector<int>& ids, bool for_gradient = false);
  void upload_idx(const std::vector<int>& ids);
  BatchView view(int nb) const;
  // free device memory in bytes; false: the runtime could not tell (the callers then keep their own fallback)
  bool free_device_bytes(double& free_bytes) const;
  // the same with the fallback of sample_posterior, predict_cov and alc: twice the prediction budget when the runtime cannot tell
  double free_bytes_or_twice_budget() const;
  // the two halves of predict_full_cov (engine_predict.hip), shared with sample_posterior.  fullcov_launches: the device part on `stream`
  // for the emulators in dIdx -- dC (nb, m, m) = Sigma*, dDots (nb, R, m) the dot products; dKf (nb, MP, LD) and dV (nb, NP, MP) are scratch.
  // fullcov_host_means: the means (nb, m) from the downloaded dot products, mean-function terms added; with the analytic mean its
  // covariance term goes into covs (host, may be null without it).
  void fullcov_launches(int nb, const double* dXf, int m, int MP, double* dKf, double* dV, double* dC, double* dDots);
  void fullcov_host_means(const std::vector<int>& ids, const double* Xs, int m, const double* dots, double* means, double* covs);
  int compute_units() const { return n_cu; }

  // (streams and events are declared in front of every buffer: members go in reverse order, so the streams are destroyed last)
  Stream stream;                     // main stream: covariance build, trailing updates, everything else
  Stream pstream;                    // look-ahead stream: panel factorisations
  std::vector<Event> evPanel, evUpd;
  std::vector<Stream> gstreams;      // extra streams for independent emulator groups
  Event evReady;
  Event evGroup[15];

 private:
  friend class ScratchFactor;      // factors matrices of its caller's with an engine of its own (engine_internal.h)
  void upload_params(const std::vector<int>& ids);
  // defer_info: leave the status words on the device (the caller reads them together with its own results: one
  // synchronisation per evaluation instead of two)
  void factorize(const std::vector<int>& ids, std::vector<int>& info, bool defer_info = false);
  // fill (everywhere below): what fills the factor buffer instead of the covariance build (build_cov); null: the covariance build
  void factorize_blocked(const std::vector<int>& ids, std::vector<int>& info, bool defer_info, const CovFill* fill = nullptr);
  // the schedules factorize_blocked chooses from (chol_schedule.h); every one leaves the status words in dInfo
  void chol_one_launch(const std::vector<int>& ids, const BatchView& v, std::vector<int>& info, bool defer_info, const CovFill* fill = nullptr);
  void chol_lookahead(const BatchView& v, const CovFill* fill = nullptr);
  void chol_two_groups(const BatchView& v, const CovFill* fill = nullptr);
  void chol_right_looking(const BatchView& v, const CovFill* fill = nullptr);
  // what the three multi-launch schedules start with: status words cleared, K built
  void begin_multi_launch(const BatchView& v, const CovFill* fill = nullptr);
  void grow_step_events(int K);                      // evPanel / evUpd hold at least K + 1 events each
  // the one-launch kernel aborted: count it and factorise again with the multi-launch schedule of the regime
  void refactor_after_abort(const std::vector<int>& ids, std::vector<int>& info, bool defer_info, const CovFill* fill = nullptr);
  void read_info(std::vector<int>& info, bool defer_info);
  // the steps of eval.  solve_and_collect: behind a factorisation of `list`, log-determinants and Gram matrices -- with want_grad, the
  // analytic mean or a pivoted emulator in the list also alpha (and L^-1 with want_grad) -- in ONE read-back; info_out (may be null)
  // receives the status words the factorisation left on the device
  void solve_and_collect(const std::vector<int>& list, std::vector<int>* info_out, bool want_grad, std::vector<double>& logdet,
                         std::vector<double>& gram);
  // the one-launch back substitution of `todo` on stream `st`; true: it also left log-det / status / Gram in dRes (never without
  // with_res: a deferred solve, whose words in dRes were final when the evaluation returned)
  bool launch_backsolve_chain_on(hipStream_t st, const BatchView& v, const std::vector<int>& todo, bool with_res = true);
  // whether solve_and_collect leaves alpha of `list` to ensure_alpha
  bool alpha_is_deferred(const std::vector<int>& list, bool want_grad) const;
  // the emulators of `timed_out` (their chain gave up on a wait) again with the multi-launch back substitution, on `stream`
  void resolve_alpha_after_timeout(const std::vector<int>& timed_out);
  // adaptive nugget: the emulators of `failed` with that nugget type are factored again with growing jitter; good[i] = 1 where it worked
  void jitter_ladder(const std::vector<int>& failed, std::vector<int>& info, std::vector<char>& good, bool want_grad,
                     std::vector<double>& logdet, std::vector<double>& gram);
  // gradient rows of the emulators of ids that are still good, each into its own row of grad
  void scatter_gradient(const std::vector<int>& ids, const std::vector<char>& good, double* grad, int grad_ld);
  std::vector<int> idx_on_device;          // what dIdx holds (upload_idx skips an identical list)
  void factorize_pivot(const std::vector<int>& ids, std::vector<int>& info);
  void ensure_pivot_buffers();
  void unpermute(int i, double* vec) const;          // vec (n) from pivoted to training order, in place
  void restore_order(int i);                         // emulator i's inputs back to training order (after a pivoted fit)
  void panel(const BatchView& v, int o, int w, hipStream_t st);
  void build_cov(const BatchView& v, const ZeroRanges& zero = ZeroRanges(), const CovFill* fill = nullptr);
  std::vector<char> z_armed;     // per emulator: its solution row holds the sentinel pattern of the one-launch back substitution
  void set_theta(int i, const double* theta);
  void require_factored(const std::vector<int>& ids) const;      // throws unless every emulator of ids holds a factor
  // the steps of predict (engine_predict.hip).  PredictPlace: where means / variances / derivatives / dot products live on the device
  struct PredictPlace {
    double *fm, *fv, *fd, *dots;
    long ld, dots_ld;
  };
  PredictPlace place_predict_outputs(int nb, int m, double* means, double* vars, double* derivs, long out_ld, bool out_on_device);
  void predict_chunks(const BatchView& v, const double* dXsrc, int m, const PredictPlace& o);
  void add_mean_terms(const std::vector<int>& ids, const double* dXsrc, int m, const PredictPlace& o);
  void copy_out_predictions(const PredictPlace& o, int nb, int m, double* means, double* vars, long out_ld, double* derivs);
  // implausibility / implausibility_top.  implausibility_chunk_points: their shared refusals, then MC, the query points per chunk (0: empty
  // input).  implausibility_chunks: the remaining validation, then per chunk the means and variances in dMean / dVar (nb, MC);
  // tail(dPrm, c0, mc) consumes them (the stream is synchronised after it: the next chunk reuses the buffers)
  int implausibility_chunk_points(const std::vector<int>& ids, int m) const;
  void implausibility_chunks(const std::vector<int>& ids, const double* Xs, int m, int MC, const double* obs, const double* obs_var,
                             const double* discrepancy, bool include_nugget, const std::function<void(const double*, int, int)>& tail);
  void ensure_predict_scratch(int nb, int MC);
  // the steps of hessian (engine_hessian.hip).  hessian_move_to: the emulators to their thetas -- fine[k] = 1 where ids[k] holds a factor
  // there, before[k] = the theta it has to be put back at (hessian_put_back).  hessian_group_sums: the device sums of one group of emulators
  // into their host copies (six launches behind the gradient's, six downloads, one synchronisation)
  struct HessianScratch;
  struct HessianSums;
  void hessian_move_to(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, std::vector<int>& fine,
                       std::vector<std::vector<double>>& before);
  void hessian_group_sums(const std::vector<int>& grp, HessianScratch& d, HessianSums& h);
  void hessian_put_back(const std::vector<int>& ids, const std::vector<std::vector<double>>& before);
  DevBuf<double> dX, dP, dT, dA, dLinv, dKinv, dAlpha;
  // signal word of the stream memory operations of the look-ahead schedule.  The one raw pointer of the engine: signal memory comes from
  // hipExtMallocWithFlags(hipMallocSignalMemory), not from the allocator behind DevBuf, and is freed in ~Engine.
  uint32_t* sigU1 = nullptr;
  uint32_t sig_epoch = 1;
  bool can_waitval = false;      // hipDeviceAttributeCanUseStreamWaitValue of the engine's device
  int device = 0;                // HIP device the engine was created on
  // one-launch Cholesky (kernels_mchol.hip): task table, control words, per-column packs
  DevBuf<int> dMcTable;          // the task order of one emulator (mchol_task_table)
  int mc_ntasks = 0;
  DevBuf<unsigned> dMcCtrl;
  int mc_slots = 0;              // batch slots dMcCtrl / dMcPacks are sized for (grown to the largest one-launch batch seen)
  DevBuf<double> dMcPacks;
  bool mc_used = false;          // the last factorisation of this engine went through the one-launch kernel (its abort word is live)
  bool mc_force_legacy = false;  // transient: repeat a factorisation with a multi-launch schedule after an abort
  int n_cu = 256;
  DevBuf<int> dBsStatus;         // time-out words of the one-launch back substitution (one per emulator), compared with bs_epoch
  int bs_epoch = 0;
  DevBuf<double> dRes;           // per emulator [log-det, status, Gram matrix] ...
  PinnedBuf<double> hRes;        // ... and its pinned host mirror
  DevBuf<double> dGradOut, dGradPartial;
  DevBuf<int> dInfo, dIdx;
  DevBuf<double> dLpack;
  DevBuf<double> dH, dZ, dM;
  // nugget="pivot": per-emulator inputs in pivot order (B*n*D), pivot order (B*n), rank (B), scratch (B*2*NP)
  DevBuf<double> dXp, dPivWork;
  DevBuf<int> dPerm, dRank;
  std::vector<int> hPerm;
  std::map<int, DevBuf<double>> w2;     // emulator -> (n - rank) x LD rows of L^-1 of the skipped pivots (gradient path)
  std::vector<double> hH;        // q x n design-matrix columns      // packed transposed diagonal block + reciprocal diagonal (potf2 -> trsm)
  PinnedBuf<double> hP;          // pinned host copy of the parameter blocks (B * PS doubles)
  // predict scratch
  DevBuf<double> dXs, dKs, dMean, dVar, dVarPartial, dDeriv;
  DevBuf<double> dMeanFin, dMeanAux;   // finished means when the dot products have their own rows; staging of the mean-function terms
  std::mt19937_64 rng;
};

// optimiser options (mogp_set_fit_options)
struct FitOptions {
  int max_iter = 200;
  double ftol = 1e-9;   // |f_k - f_{k+1}| <= ftol * max(1, |f|)   (dlib objective_delta_stop_strategy(1e-9), fitting.hpp:92)
  double gtol = 1e-6;
  unsigned long long seed = 0;
};
FitOptions& fit_options();

// gKDR (kernels_gkdr.hip): R of every (input scale, output scale) pair, row-major, into R_out (nx * ny * m * m); info_out[i] != 0 when
// A = Kx + n eps I of input scale i is not positive definite (its R are NaN).  max_pairs_per_pass = 0: sized by free device memory.
void gkdr_R(const double* X, int n, int m, const double* y, int nx, const double* sgx2, int ny, const double* sgy2, double eps,
            int max_pairs_per_pass, double* R_out, int* info_out);

// Maximin design scoring (kernels_design.hip): out[t] = the smallest pairwise Euclidean distance of design t of `designs` (T, n, D), host
// pointers.  The designs pass through the device DESIGN_SCRATCH_BYTES at a time (one design where a single one is larger), so T is unbounded.
constexpr size_t DESIGN_SCRATCH_BYTES = (size_t)64 << 20;
constexpr int DESIGN_MAX_PASS = 32768;      // designs per pass (the second grid dimension)
constexpr int DESIGN_MAX_N = 370688;        // points per design: 64 x 64 tiles of the lower triangle x 256 threads < 2^32 work-items
void design_min_pdist(const double* designs, int T, int n, int D, double* out);
// Optimised maximin Latin hypercubes (kernels_lhs.hip; DESIGN.md section 3 "Design"): C independent chains of column-swap threshold accepting on
// the level matrices `start` (C, n, D), host pointers throughout.  Chain c draws its proposals from Philox stream `stream + c` under `seed`.
// Outputs per chain: the best level matrix, its phi, min R and pairs at the minimum, and the accepted proposals.  Limits: lhs_plan.h.
void design_anneal_lhs(const int* start, int C, int n, int D, long long n_steps, int q, double theta0, double rho, long long stage,
                       unsigned long long seed, unsigned stream, int* best_out, double* phi_out, long long* minr_out, long long* pairs_out,
                       long long* accepted_out);

// Local approximate GP prediction (the handle: engine_local.hip, its kernels: kernels_local.hip; DESIGN.md section 3 "Local prediction"): the design (N, D) and E rows of residual
// targets stay on the device the handle was created on; every predict() finds the k nearest design points of each query in the metric
// of `scale` and predicts from that k-point GP alone.  No Engine: nothing here factors the whole design.
class LocalGP {
 public:
  LocalGP(const double* inputs, long N, int D, const double* resid, int E);
  // host pointers; var / nbr may be null.  kt: 0 squared exponential, 1 Matern 5/2.
  void predict(int e, int kt, const double* scale, double sigma2, double nugget, double jitter, bool include_nugget, const double* testing, long m,
               int k, int max_points, double* mean, double* var, int* ok, double* radius, int* nbr);
  // Vecchia likelihood (DESIGN.md section 3 "Vecchia fit"): the design counts as ORDERED, the neighbours of row t are rows < t.
  // vecchia_neighbours searches them in the metric of `scale` and keeps the (N, k) lists on the device (nbr_out: host, may be null);
  // vecchia_loglik evaluates sum_t log p(y_t | y_nbr(t)) of residual row e on those lists (k must be the k of the search): value_out (1),
  // grad_out (D + 2: d/d log s_d^2, d/d log sigma2, d/d log nugget; written with want_grad), terms_out (N) / ok_out (N) may be null.
  void vecchia_neighbours(const double* scale, int k, int* nbr_out);
  void vecchia_loglik(int e, int kt, const double* scale, double sigma2, double nugget, double jitter, int k, bool want_grad, int max_points,
                      double* value_out, double* grad_out, double* terms_out, int* ok_out);
  // Iterative exact prediction (engine_iter.hip; DESIGN.md section 3 "Iterative exact prediction"): conjugate gradients on A = sigma2 k(X, X)
  // + nugget I of the WHOLE design, A never stored.  Host pointers; matrices with several columns are row-major as the caller holds them.
  // The state of all of it is one IterSolver (iter_solver.h); the methods below are the entry points: refusals, plan, calls on the solver, copies.
  // kmatvec: out (M, r) = A V (N, r) with queries == null (M = N), else sigma2 k(queries (m, D), X) V (M = m, no nugget).
  void kmatvec(int kt, const double* scale, double sigma2, double nugget, const double* queries, long m, const double* V, int r, double* out);
  // Builds and keeps the preconditioner P = L L^T + nugget I of these hyperparameters, L (N, rank reached) the partial pivoted Cholesky
  // factor of sigma2 k(X, X); returns the rank reached (it stops early when the largest remaining diagonal is <= 0).  piv_out (rank) and
  // L_out (N, rank) row-major may be null; only the first `rank reached` entries / columns are written, the rest is zero.
  int precondition(int kt, const double* scale, double sigma2, double nugget, int rank, int* piv_out, double* L_out);
  // Column-wise preconditioned CG at the hyperparameters of the last precondition: x (N, c); per column iterations, converged (the recurrence
  // residual met |r| <= rtol |b| within max_iter) and residual = |b - A x| / |b| from one further product, as it is.
  void solve(const double* B, int c, double rtol, int max_iter, double* x, int* iterations, int* converged, double* residual);
  // alpha = A^-1 (residual row e) -- solved once and kept per emulator while hyperparameters, rank, rtol and max_iter stay -- and
  // mean (m) = sigma2 k(testing, X) alpha; with var: var (m) = max(sigma2 - k*^T A^-1 k* + (include_nugget ? nugget : 0), 0), the solves in
  // blocks of 32 queries.  stat_i (2) = iterations, converged and stat_r (1) = residual of the alpha solve; var_stat_i (2 m) and
  // var_stat_r (m) the same per query; alpha_out (N) may be null.  m = 0: alpha alone.
  void predict_exact(int e, int kt, const double* scale, double sigma2, double nugget, int rank, double rtol, int max_iter, bool include_nugget,
                     const double* testing, long m, int max_points, double* mean, double* var, int* stat_i, double* stat_r, int* var_stat_i,
                     double* var_stat_r, double* alpha_out);
  // The pieces of the exact log-likelihood of residual row e and of its gradient (engine_iter_lik.hip; DESIGN.md section 3 "Iterative exact
  // likelihood"): the preconditioner, the probes z_t = L g1_t + sqrt(nugget) g2_t (g1 (g1_rows, T) with g1_rows the rank the preconditioner
  // reaches, g2 (N, T), row-major standard normals; at rank 0 the preconditioner is the identity and z_t = g2_t), ONE solve of the panel
  // [y | z_1 .. z_T] with the step coefficients logged, the dots and -- with want_grad -- the sweep of launch_kgrad_forms.  C = 1 + T.
  //   scalars (4)     y^T alpha, alpha^T alpha, log|G| (G = nugget I + L^T L; 0 at rank 0), the rank reached
  //   stat_i (2 C)    iterations, converged per column;  residual (C)
  //   rho (T), uw (T) z_t^T w_t with w_t = P^-1 z_t, and u_t^T w_t with u_t = A^-1 z_t
  //   coef (max_iter, 2, C)  the CG step coefficients alpha_j, beta_j of every column while it was live, zero elsewhere
  //   forms (2 D)     with want_grad: alpha^T (dA/dtheta_d) alpha, then sum_t u_t^T (dA/dtheta_d) w_t; forms_each (T, D) or null: the
  //                   latter per probe, from one sweep each
  //   z_out (N, T), x_out (N, C), w_out (N, C) or null: the probes, the solutions [alpha | u_t] and the other side of the forms
  //                   [alpha | w_t], row-major.  alpha is kept as predict_exact keeps it.
  void loglik_exact(int e, int kt, const double* scale, double sigma2, double nugget, int rank, double rtol, int max_iter, const double* g1,
                    int g1_rows, const double* g2, int T, bool want_grad, double* scalars, int* stat_i, double* residual, double* rho, double* uw,
                    double* coef, double* forms, double* forms_each, double* z_out, double* x_out, double* w_out);
  // A conservative bound of the predictive variance from the preconditioner's factor (DESIGN.md section 3 "Variance bound"): with R (N, r)
  // such that R^T A R = I and span R = span L, var (m) = max(sigma2 + (include_nugget ? nugget : 0) - |R^T k*|^2, 0) >= the exact variance,
  // because R R^T is a Galerkin inverse of A.  R is built once per (hyperparameters, rank) and kept; no solve is involved.  rank >= 1;
  // var_rank_request: 0 for every column of the cache, else 1 .. the rank the preconditioner reached (the leading columns: R is nested).
  // *var_rank_out = the columns that entered.  R_out (N, rank) row-major or null: the cache, columns behind its rank zero.  m = 0: the cache alone.
  void variance_bound(int kt, const double* scale, double sigma2, double nugget, int rank, int var_rank_request, bool include_nugget,
                      const double* testing, long m, int max_points, double* var, int* var_rank_out, double* R_out);
  // Pathwise posterior draws (engine_rff.hip; DESIGN.md section 3 "Pathwise posterior draws").  Matrices of draws are (S, .) row-major.
  // rff: out (S, M) = (amp Phi(P) W^T)^T with Phi_if = cos(phase_f + omega_f . P_i) over the scaled rows P of the design (queries == null,
  // M = N) or of queries (m, D); omega (F, D), phase (F), W (S, F).  Column s depends on row s of W alone, entry (s, i) on point i alone;
  // max_points caps the points per pass (0: sized by the free memory) and changes no bit.
  void rff(const double* scale, const double* queries, long m, const double* omega, const double* phase, int F, const double* W, int S, double amp,
           int max_points, double* out);
  // The updates v_s = A^-1 (y_e - g_s(X) - sqrt(nugget) eps_s) of S paths, g_s = amp Phi(X) W_s: the preconditioner of these hyperparameters
  // (built unless held), the right-hand sides formed on the device, IterSolver::solve in blocks of 32.  W_in (S, F) / noise_in (S, N) or null:
  // then the normals of draw first_draw + s of the streams stream + 3 / stream + 4 under `seed` (philox_dev.h), generated on the device.
  // W_out (S, F) the weights' normals used, v_out (S, N), stat_i (2 S) iterations and converged, residual (S) = |b - A v| / |b|, *rank_out
  // the rank the preconditioner reached.  A column that does not converge is reported, not refused.
  void sample_paths(int e, int kt, const double* scale, double sigma2, double nugget, int rank, double rtol, int max_iter, const double* omega,
                    const double* phase, int F, int S, double amp, unsigned long long seed, unsigned stream, int first_draw, const double* W_in,
                    const double* noise_in, double* W_out, double* v_out, int* stat_i, double* residual, int* rank_out);
  // Input derivatives at large designs (DESIGN.md section 3 "Input derivatives at large designs"), with respect to the RAW query coordinates.
  // kmatvec_inputderiv: out (m, D, r) row-major, out[i][d][c] = d/dx_d [sigma2 k(q_i, X) V]_c = 2 s_d sum_j sigma2 k'(r2_ij) (q~_id - x~_jd) V_jc
  // for queries (m, D) and V (N, r); no nugget term.  rff_inputderiv: out (S, m, D), out[s][i][d] = d/dx_d of rff's entry (s, i)
  // = -amp s_d sum_f W_sf omega_fd sin(phase_f + omega_f . q~_i).  Column c / draw s depends on column c of V / row s of W alone, row i on
  // query i alone; max_points caps the queries per pass (0: sized by the free memory) and changes no bit.
  void kmatvec_inputderiv(int kt, const double* scale, double sigma2, const double* queries, long m, const double* V, int r, int max_points,
                          double* out);
  void rff_inputderiv(const double* scale, const double* queries, long m, const double* omega, const double* phase, int F, const double* W, int S,
                      double amp, int max_points, double* out);
  int device_id() const { return device; }
  const long N;
  const int D, E;

 private:
  void ensure_scaled(const double* scale, hipStream_t st);      // dXs = dX * scale, formed again only when the scales change
  void precondition_for(const IterKey& k, hipStream_t st);     // the scaled design of k's scales, then the solver's preconditioner of k
  IterSolver iter;                   // the whole state of the iterative solver (iter_solver.h); it sees dXs and dY through const pointers
  int device = 0, n_cu = 1;
  DevBuf<double> dX, dY, dXs, dScale;
  std::vector<double> hScale;        // the scales dXs was formed with (empty: not formed yet)
  int vk = 0;                        // the k of the Vecchia lists in dVnbr (0: none yet)
  DevBuf<int> dVnbr, dVok;
  DevBuf<double> dVout, dVred, dVscratch;
};

// measurement hooks (mogp_profile_schedule): force the Cholesky schedule / serialise it onto one stream so that the
// HIP-event time of a kernel is its time alone on the device; -1 / false = the library's own choice.
// FOR MEASUREMENT ONLY: process-global, read by every engine at the start of a factorisation and not synchronised --
// set it while no evaluation is in flight (bench.py does), never from a thread that races with one.
struct ScheduleOverride {
  int schedule = -1;       // 0 two emulator groups, 1 right-looking, 3 look-ahead, 4 one launch (task queue), 5 the multi-launch schedule of the regime
  bool single_stream = false;
};
ScheduleOverride& schedule_override();

void prof_enable(bool on);
void prof_reset();
bool prof_get(const char* tag, double* ms, long long* launches, double* flops, double* bytes);
// process-wide diagnostic counters (mogp_profile_counter): "backsolve_timeouts" = back substitutions repeated with the
// multi-launch path after a wait of the one-launch chain timed out; "alpha_solves" = emulators whose alpha was solved, at once
// (eval with gradient, analytic mean, pivot) or when a reader first asked (ensure_alpha)
long long prof_counter(const char* name);

}  // namespace mogp
