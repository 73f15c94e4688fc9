// The analyses of a fitted engine that only READ it: prediction averaged over hyperparameter samples (analysis_mixture.hip),
// cross-validation (analysis_cv.hip), joint posterior draws (analysis_sample.hip), the posterior cross-covariance, the ALC criterion and
// its greedy batches (analysis_active.hip).  Free functions of an Engine: they see its public data and calls and the service block
// "for the analyses" of engine.h, and none of its device buffers.  (The Hessian moves emulators to other thetas and stays a member.)
#pragma once
#include <vector>

#include "devmem.h"
#include "engine.h"

namespace mogp {

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
void predict_mixture(Engine& eng, const std::vector<int>& ids, const double* thetas, int S, int ld, const double* weights, const double* log_q,
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
void cross_validate(Engine& eng, const std::vector<int>& ids, const int* labels, int k, bool include_nugget, int max_slots, double* mean,
                    double* var, double* maha, double* log_score, int* ok);
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
void sample_posterior(Engine& eng, const std::vector<int>& ids, const unsigned* streams, const double* Xs, int m, int S, unsigned long long seed,
                      const double* z_in, bool z_per_emulator, bool include_nugget, double jitter, int max_slots, int max_draws,
                      double* samples, double* mean, double* z_out, double* jitter_used, int* ok);
// Posterior covariance of the latent function between two point sets, per emulator of `ids` (kernels_alc.hip, DESIGN.md section 3 "Active
// learning"): out (ids, m1, m2) = sigma^2 k(X1, X2) - V_1^T V_2 with V = L^-1 K*^T as predict_full_cov stores it; nugget not included.
// X2 == null: X2 = X1.  The emulators go in groups sized by the 64 GB rule of predict_full_cov (V_1, V_2, the output and the K* scratch
// counted) and half of the free device memory; every buffer is scratch of the call.  THIS engine is only read, apart from gaining L^-1.
// Throws for nugget="pivot", the analytic mean, an emulator that is not fit, m < 1, non-finite points, negative max_slots and one emulator
// beyond either memory rule.
void predict_cov(Engine& eng, const std::vector<int>& ids, const double* X1, int m1, const double* X2, int m2, int max_slots, double* out);
// The ALC design criterion of emulators `ids` at fixed hyperparameters: with c the covariance above, s^2(x) = max(c(x, x), 0) as predict()
// reports it (the engine's own predictive-variance launches: the same bits) and tau[e] >= 0 the noise variance of one more run,
//   reduction[e][i] = sum_j w_j c_e(r_j, c_i)^2 / (s_e^2(c_i) + tau[e])           candidates Xc (mc, D), reference Xr (mr, D), weights w (mr) >= 0
// reduction / cand_var / degenerate (ids, mc), ref_var (ids, mr).  noise == null: tau[e] = nugget_size(ids[e]).  A candidate with
// s^2 + tau <= (n + 2) 2^-52 sigma^2 -- the rounding of sigma^2 minus a sum of n squares -- gets reduction 0 and degenerate 1; no NaN.
// The emulators go `slots` per group and the reference points `points` per chunk (alc_plan; max_slots / max_points = 0: the library's
// choice); the partial sums are kept per 128-point tile of the WHOLE reference set and added in ascending tile order, so the same call
// returns the same bits and neither number changes any.  Throws as predict_cov does, and for negative or non-finite weights or noise and
// weights that sum to 0.
void alc(Engine& eng, const std::vector<int>& ids, const double* Xc, int mc, const double* Xr, int mr, const double* w, const double* noise,
         int max_slots, int max_points, double* reduction, double* cand_var, double* ref_var, int* degenerate);
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
void alc_batch_check(const Engine& eng, const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
                     const double* noise, int q, int max_slots, std::vector<double>& tau);
long alc_batch_slots(const Engine& eng, long E, int M, int mr, int T, int max_slots, bool total);
// select = "each": out holds the rows of ids
void alc_batch(Engine& eng, const std::vector<int>& ids, const double* X, int M, int forced, const double* Xr, int mr, const double* w,
               const double* noise, int q, int max_slots, const AlcBatchOut& out);

}  // namespace mogp
