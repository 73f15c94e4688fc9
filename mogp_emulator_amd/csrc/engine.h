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

struct CvBuffers;      // engine_analysis.hip
struct CvFolds;        // predict_plan.h
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
  // Prediction averaged over S hyperparameter samples per emulator (kernels_mixture.hip).  thetas (E, S, ld): full vectors [mean | data]
  // of emulator ids[e], the first n_theta of each row used; EXACTLY ONE of weights (E, S, non-negative) and log_q (E, S, the log proposal
  // density up to a constant: self-normalised importance weights exp(-(F - F_min) - (log_q - log_q at the arg-min)), predict_plan.h
  // mixture_weights); Xs host (m, D).  The (emulator, sample) pairs are factored on a replica engine (as fit_map's starts are), emulator-major
  // and sample-ascending, `slots` at a time; THIS engine's emulators are not refitted -- factor, alpha, L^-1, K^-1, theta and logpost stay.
  // Per emulator and point, with the PIVOT mu_0 = the mean of sample 0 -- whatever its weight -- or, where sample 0 failed to factorise,
  // of the first sample that did, d_s = mu_s - mu_0 and v_s = max(variance + (include_nugget ? sample s's own nugget : 0), 0) as predict()
  // reports it:   mean = mu_0 + sum w_s d_s,  within = sum w_s v_s,  between = max(sum w_s d_s^2 - (sum w_s d_s)^2, 0)     -- (E, m) each.
  // Per sample (E, S): the normalised weights, F (the value eval returns, NaN where it failed) and ok.  A sample that fails gets weight 0;
  // an emulator whose samples all fail or whose weights sum to 0 gets NaN rows and ok_all[e] = 0 (ok_all may be null) -- not an error.
  // The sums are updated in sample order with one add per sample and no atomics: the same bits for every max_slots >= 1 (slots per pass)
  // and max_points >= 1 (query points per chunk); 0 = the library's choice.  Throws for nugget="pivot" and the analytic mean.
  void predict_mixture(const std::vector<int>& ids, const double* thetas, int S, int ld, const double* weights, const double* log_q,
                       const double* Xs, int m, bool include_nugget, int max_slots, int max_points, double* mean_out, double* within_out,
                       double* between_out, double* weights_out, double* logpost_out, int* ok_out, int* ok_all);
  // Leave-one-out / k-fold predictive errors of emulators `ids` at their fitted hyperparameters, without refitting (kernels_cv.hip).
  // labels (n): the fold of every training point, values 0 .. k-1, every fold non-empty, 2 <= k <= n.  With Q the factored matrix,
  // alpha = Q^-1 r and S = (Q^-1)_FF of a fold F: the held-out error is e_F = S^-1 alpha_F and the held-out covariance of the
  // observations S^-1.  mean / var (ids, n): mean_i = t_i - e_i and var_i = (S^-1)_ii -- with include_nugget false max(var_i - nugget
  // used, 0) --, in training order.  maha / log_score / ok (ids, k): e_F^T S e_F, the log predictive density of the fold given the
  // rest, and whether S factorised (0: NaN for the fold's points and scalars; no jitter, no exception).  Every fold a single point:
  // one pass over L^-1.  Otherwise K^-1 is formed and the (emulator, fold) pairs go, emulator-major and fold-ascending, `slots` per
  // pass (cv_plan of predict_plan.h; max_slots = 0: the library's choice) through a ScratchFactor of the call.  THIS engine is only
  // read, apart from gaining alpha / L^-1 / K^-1: theta, factor and logpost stay.  No atomics: the same call returns the same bits.
  // Throws for nugget="pivot", the analytic mean, an emulator that is not fit, bad k, a label outside [0, k) and an empty fold.
  void cross_validate(const std::vector<int>& ids, const int* labels, int k, bool include_nugget, int max_slots, double* mean, double* var,
                      double* maha, double* log_score, int* ok);
  // leave-one-out predictive variance of emulator i at its own training inputs (MICEFastGP.fast_predict for every index)
  void loo_variance(int i, double* out);
  // predict(full_cov=True), GaussianProcess.py:899-911: means (nb, m), covs (nb, m, m) host buffers, nugget NOT included
  void predict_full_cov(const std::vector<int>& ids, const double* Xs, int m, double* means, double* covs);
  // Joint posterior draws of emulators `ids` at the m query points Xs (host, (m, D)) -- kernels_sample.hip, DESIGN.md section 3 "Sampling".
  // With Sigma*_e, mu*_e what predict_full_cov returns (the same launches, the same bits; nugget not included):
  //   Sigma~_e = Sigma*_e + ((include_nugget ? nugget used by the fit : 0) + jitter + delta_e) I = L_e L_e^T,
  //   samples[e][s][:] = mu*_e + L_e z[e][s][:]                                              samples (ids, S, m), mean (ids, m).
  // delta_e = 0 on the first try; an emulator whose Sigma~ does not factorise is tried again -- it alone -- with delta_e =
  // sample_ladder_delta(t, mean diag Sigma*_e), t = 0 .. 4 (predict_plan.h); jitter_used[e] = jitter + delta_e; after the fifth failure
  // ok[e] = 0 and its samples are NaN (no exception).  The factor's diagonal is finished from its rows with the correctly rounded square root.  z: z_in (S, m) shared by all emulators or, with z_per_emulator, (ids, S, m); null:
  // generated on the device, value (e, s, j) from (seed, streams[e], s, j) alone (philox_dev.h).  z_out (ids, S, m) or null: the normals used.
  // The emulators go `slots` per pass and the draws `draws` per chunk (sample_plan; max_slots / max_draws = 0: the library's choice)
  // through a ScratchFactor of m rows; every buffer is scratch of the call.  THIS engine is only read, apart from gaining alpha / L^-1.  One writer
  // per output, no atomics: the same call returns the same bits, and max_draws changes none.  Throws for nugget="pivot", the analytic mean,
  // an emulator that is not fit, S < 1, jitter < 0, negative max_*, non-finite Xs / z_in and scratch beyond sample_plan's limits.
  void sample_posterior(const std::vector<int>& ids, const unsigned* streams, const double* Xs, int m, int S, unsigned long long seed,
                        const double* z_in, bool z_per_emulator, bool include_nugget, double jitter, int max_slots, int max_draws,
                        double* samples, double* mean, double* z_out, double* jitter_used, int* ok);
  // Posterior covariance of the latent function between two point sets, per emulator of `ids` (kernels_alc.hip, DESIGN.md section 3 "Active
  // learning"): out (ids, m1, m2) = sigma^2 k(X1, X2) - V_1^T V_2 with V = L^-1 K*^T as predict_full_cov stores it; nugget not included.
  // X2 == null: X2 = X1.  The emulators go in groups sized by the 64 GB rule of predict_full_cov (V_1, V_2, the output and the K* scratch
  // counted) and half of the free device memory; every buffer is scratch of the call.  THIS engine is only read, apart from gaining L^-1.
  // Throws for nugget="pivot", the analytic mean, an emulator that is not fit, m < 1, non-finite points, negative max_slots and one emulator
  // beyond either memory rule.
  void predict_cov(const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_slots, double* out);
  // The ALC design criterion of emulators `ids` at fixed hyperparameters: with c the covariance above, s^2(x) = max(c(x, x), 0) as predict()
  // reports it (the engine's own predictive-variance launches: the same bits) and tau[e] >= 0 the noise variance of one more run,
  //   reduction[e][i] = sum_j w_j c_e(r_j, c_i)^2 / (s_e^2(c_i) + tau[e])           candidates Xc (mc, D), reference Xr (mr, D), weights w (mr) >= 0
  // reduction / cand_var / degenerate (ids, mc), ref_var (ids, mr).  noise == null: tau[e] = nugget_size(ids[e]).  A candidate with
  // s^2 + tau <= (n + 2) 2^-52 sigma^2 -- the rounding of sigma^2 minus a sum of n squares -- gets reduction 0 and degenerate 1; no NaN.
  // The emulators go `slots` per group and the reference points `points` per chunk (alc_plan; max_slots / max_points = 0: the library's
  // choice); the partial sums are kept per 128-point tile of the WHOLE reference set and added in ascending tile order, so the same call
  // returns the same bits and neither number changes any.  Throws as predict_cov does, and for negative or non-finite weights or noise and
  // weights that sum to 0.
  void alc(const std::vector<int>& ids, const double* Xc, int mc, const double* Xr, int mr, const double* w, const double* noise, int max_slots,
           int max_points, double* reduction, double* cand_var, double* ref_var, int* degenerate);
  // Greedy ALC batches at fixed hyperparameters (kernels_alc.hip, DESIGN.md section 3 "Active learning: batches").  The predictive variance
  // does not depend on the targets, so conditioning on a run at p with noise tau appends one row to the Cholesky factor and one entry
  // u(x) = c(x, p) / sqrt(s^2(p) + tau) to every stored v(x): c_new(x, x') = c(x, x') - u(x) u(x'), s^2_new(x) = s^2(x) - u(x)^2.  V_c and V_r
  // are built once, with room for the rows of all T = forced + q steps behind their roundup(n, 16) base rows, and step t is alc's product
  // over n16 + t rows, alc_finish with the floor of n + t, the pick, and two rank-one updates: no n^3 and no (m_c + m_r) n^2 work per pick.
  // X (M, D): the candidates; the first `forced` of them are taken in order in steps 0 .. forced - 1 (points already submitted), the other
  // steps take the unmasked candidate with the largest score, ties to the lowest index.  A step whose best score is not above 0 or whose
  // denominator is at or below (n + t + 2) 2^-52 sigma^2 picks -1 and conditions on nothing; a picked candidate is masked.
  // AlcBatch is one group of emulators resident on the device for the whole batch; alc_batch runs the groups of alc_batch_plan one after
  // another, every step enqueued without a host synchronisation (select = "each").  select = "total" drives one AlcBatch per part from the
  // C ABI layer: scores() -> the host's sum and arg-max -> apply(pick).  THIS engine is only read, apart from gaining L^-1.
  struct AlcBatchOut {       // host arrays, rows of the group's emulators; T = forced + q.  red / deg may be null (scores not kept)
    int* picks;              // (E, T)   -1: nothing picked in that step
    double* pick_red;        // (E, T)   the score of the pick, 0 where there is none
    double* red;             // (E, T, M)
    int* deg;                // (E, T, M)
    double* cand_var;        // (E, M)   before any step: predict()'s own bits
    double* ref_var;         // (E, mr)  likewise
    double* ref_var_after;   // (E, mr)  after the last step, clipped at 0
    double* iv;              // (E, T + 1)  iv[0] = sum_j w_j ref_var[j] in ascending j, iv[t + 1] = iv[t] - pick_red[t]
    AlcBatchOut rows_from(size_t e0, int T, int M, int mr) const {
      return {picks + e0 * T, pick_red + e0 * T, red ? red + e0 * T * M : nullptr, deg ? deg + e0 * T * M : nullptr, cand_var + e0 * M,
              ref_var + e0 * mr, ref_var_after + e0 * mr, iv + e0 * (T + 1)};
    }
  };
  class AlcBatch {
   public:
    // builds V_c, V_r and both variances of emulators grp (tau: their noise variances) and starts the downloads of out.cand_var / ref_var;
    // out must outlive the object.  The caller has checked the arguments (alc_batch_check) and the memory (alc_batch_plan).
    AlcBatch(Engine& eng, const std::vector<int>& grp, const double* tau, const double* X, int M, int forced, const double* Xr, int mr,
             const double* w, int q, const AlcBatchOut& out);
    int steps() const { return T; }
    // the scores of step t on the device (product, finish); with out.red they are also on their way to the host
    void scores(int t);
    // the same, then waits: row_red / row_deg (E, M) of this step on the host
    void scores_to_host(int t, double* row_red, int* row_deg);
    // the pick of step t (forced >= 0: that candidate; -1: the arg-max on the device) and the conditioning on it
    void apply(int t, int forced);
    // waits for everything, fills the rest of out
    void finish();

   private:
    Engine& e;
    std::vector<int> ids;
    AlcBatchOut o;
    int cnt, M, mr, T, MPc, MPr, tiles_r, rows, n16;
    std::vector<double> hw;
    DevBuf<double> dXc, dXr, dW, dTau, dVc, dVr, dPart, dVarC, dVarR, dRed, dPickRed, dPickD;
    DevBuf<int> dDeg, dMask, dPicks;
  };
  // the refusals of a batch, as `alc_batch`; tau (ids) receives the noise variances
  void alc_batch_check(const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
                       const double* noise, int q, int max_slots, std::vector<double>& tau) const;
  long alc_batch_slots(long E, int M, int mr, int T, int max_slots, bool total) const;
  // select = "each": out holds the rows of ids
  void alc_batch(const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w, const double* noise,
                 int q, int max_slots, const AlcBatchOut& out);
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
  void upload_idx(const std::vector<int>& ids);
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
  // alpha of the emulators of ids that hold a factor but not yet alpha: the one-launch chain on `stream`, its time-out words read back
  // (one small copy and synchronisation of its own), the repeat with the multi-launch path where a wait gave up
  void ensure_alpha(const std::vector<int>& ids);
  void ensure_linv(const std::vector<int>& ids);
  void ensure_kinv(const std::vector<int>& ids, bool for_gradient = false);
  BatchView view(int nb) const;
  void build_cov(const BatchView& v, const ZeroRanges& zero = ZeroRanges(), const CovFill* fill = nullptr);
  std::vector<char> z_armed;     // per emulator: its solution row holds the sentinel pattern of the one-launch back substitution
  void set_theta(int i, const double* theta);
  void require_factored(const std::vector<int>& ids) const;      // throws unless every emulator of ids holds a factor
  // what cross_validate, sample_posterior, predict_cov and alc refuse alike, as `who`: an emulator without a factor, the analytic mean
  // (`analytic_reason`: why the caller cannot cover it) and nugget="pivot"
  void require_plain_fit(const char* who, const std::vector<int>& ids, const char* analytic_reason) const;
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
  // free device memory in bytes; false: the runtime could not tell (the callers then keep their own fallback)
  bool free_device_bytes(double& free_bytes) const;
  // the same with the fallback of sample_posterior, predict_cov and alc: twice the prediction budget when the runtime cannot tell
  double free_bytes_or_twice_budget() const;
  // the steps of hessian (engine_analysis.hip).  hessian_move_to: the emulators to their thetas -- fine[k] = 1 where ids[k] holds a factor
  // there, before[k] = the theta it has to be put back at (hessian_put_back).  hessian_group_sums: the device sums of one group of emulators
  // into their host copies (six launches behind the gradient's, six downloads, one synchronisation)
  struct HessianScratch;
  struct HessianSums;
  void hessian_move_to(const std::vector<int>& ids, const std::vector<const double*>& thetas, double* H, int ld, std::vector<int>& fine,
                       std::vector<std::vector<double>>& before);
  void hessian_group_sums(const std::vector<int>& grp, HessianScratch& d, HessianSums& h);
  void hessian_put_back(const std::vector<int>& ids, const std::vector<std::vector<double>>& before);
  // the two paths of cross_validate (engine_analysis.hip): every fold a single point / the folds of cf through a ScratchFactor
  void cv_leave_one_out(const std::vector<int>& ids, const int* labels, bool include_nugget, CvBuffers& b, double* mean_out, double* var_out,
                        double* maha_out, double* log_score_out, int* ok_out);
  void cv_kfold(const std::vector<int>& ids, const CvFolds& cf, int k, bool include_nugget, int max_slots, CvBuffers& b, double* mean_out,
                double* var_out, double* maha_out, double* log_score_out, int* ok_out);
  // the two halves of predict_full_cov (engine_predict.hip), shared with sample_posterior.  fullcov_launches: the device part on `stream`
  // for the emulators in dIdx -- dC (nb, m, m) = Sigma*, dDots (nb, R, m) the dot products; dKf (nb, MP, LD) and dV (nb, NP, MP) are scratch.
  // fullcov_host_means: the means (nb, m) from the downloaded dot products, mean-function terms added; with the analytic mean its
  // covariance term goes into covs (host, may be null without it).
  void fullcov_launches(int nb, const double* dXf, int m, int MP, double* dKf, double* dV, double* dC, double* dDots);
  void fullcov_host_means(const std::vector<int>& ids, const double* Xs, int m, const double* dots, double* means, double* covs);
  // the steps of sample_posterior (engine_analysis.hip)
  struct SamplePass;
  void sample_build(const std::vector<int>& grp, const double* Xs, const double* dXq, int m, SamplePass& p, double* mean_out);
  void sample_factor(ScratchFactor& sub, const std::vector<int>& grp, bool include_nugget, double jitter, SamplePass& p, double* jitter_used, int* ok);
  void sample_draws(ScratchFactor& sub, long e0, long cnt, int m, int S, int Sc, unsigned long long seed, const double* z_in, bool z_per_emulator,
                    SamplePass& p, double* samples, double* z_out);

  // what alc and predict_cov share (engine_analysis.hip): the refusals; and, for the nb emulators in dIdx and the m points at dXq, K*
  // (scratch), the predictive variance (dVar, rows var_ld apart; null: not wanted) and V = L^-1 K*^T, with predict()'s own launches
  void check_cov_args(const char* who, const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_a, int max_b) const;
  void points_v(int nb, const double* dXq, int m, int MP, double* dK, double* dDots, double* dPartial, double* dVar, int var_ld, double* dV);

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
  int device_id() const { return device; }
  const long N;
  const int D, E;

 private:
  void ensure_scaled(const double* scale, hipStream_t st);      // dXs = dX * scale, formed again only when the scales change
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
