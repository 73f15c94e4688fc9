/*
 * mogp_hip.h -- C ABI of libmogp_hip.so: an MI355X (gfx950) native GP fit + predict
 * backend that drops in behind mogp_emulator's GPU seam.
 *
 * The seam it replaces is the pybind11 module `libgpgpu`
 * (reference: mogp_gpu/src/bindings.cu:13-621, imported by mogp_emulator/LibGPGPU.py:5-14).
 * Every entry point below names the reference binding (file:line) whose behaviour it
 * provides.  The signatures are plain C: pointers + sizes, no torch / numpy / Eigen types.
 *
 * Conventions
 *  - all arrays are IEEE double, C-contiguous (row major); outputs are caller-allocated
 *    buffers filled in place (Eigen::Ref semantics of types.hpp:15-18).
 *  - `theta` passed to fit = [mean params..., corr_raw (D), log sigma^2, (log nugget)],
 *    length n_mean + n_data (densegp_gpu.hpp:493-503).
 *  - every call returns 0 on success, non-zero on failure; mogp_last_error() returns the
 *    message of the last failure on the calling thread.  The Python shim turns that into
 *    RuntimeError(msg) exactly where the reference throws std::runtime_error.
 *  - calls on one handle are not thread safe; distinct handles may be used concurrently.
 *  - pointers whose name starts with `d_` are DEVICE pointers (HBM resident); all others
 *    are host pointers.
 */
#ifndef MOGP_HIP_H
#define MOGP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* enums: values are those of mogp_gpu/src/types.hpp:29-35 (bindings.cu:585-598) */
/* 2-4: kernels the reference only has on the CPU (Kernel.py:946-997); the uniform kernels have one correlation parameter */
enum mogp_kernel_type { MOGP_SQUARED_EXPONENTIAL = 0, MOGP_MATERN52 = 1, MOGP_PRODUCT_MATERN52 = 2, MOGP_UNIFORM_SQUARED_EXPONENTIAL = 3,
                        MOGP_UNIFORM_MATERN52 = 4 };
/* 3: the CPU class's nugget="pivot" (GPParams.py:185-186; cholesky_factor(..., "pivot"), linalg/cholesky.py:182-184) */
enum mogp_nugget_type { MOGP_NUG_ADAPTIVE = 0, MOGP_NUG_FIT = 1, MOGP_NUG_FIXED = 2, MOGP_NUG_PIVOT = 3 };
enum mogp_prior_type { MOGP_PRIOR_INVGAMMA = 0, MOGP_PRIOR_GAMMA = 1, MOGP_PRIOR_LOGNORMAL = 2, MOGP_PRIOR_WEAK = 3 };

typedef struct mogp_meanfunc mogp_meanfunc;   /* BaseMeanFunc   meanfunc.hpp:24-66            */
typedef struct mogp_densegp mogp_densegp;     /* DenseGP_GPU    densegp_gpu.hpp:36-867        */
typedef struct mogp_mogp mogp_mogp;           /* MultiOutputGP_GPU multioutputgp_gpu.hpp:35-287 */

/* ---- library-level ------------------------------------------------------------------ */
const char* mogp_last_error(void);
/* have_compatible_device(), bindings.cu:600 / util.hpp:40-47 */
int mogp_have_compatible_device(void);
int mogp_device_count(void);
/* select the HIP device used by handles created afterwards on this thread (one process per GPU) */
int mogp_set_device(int device);
const char* mogp_version(void);

/* ---- mean functions (bindings.cu:365-413, meanfunc.hpp) ------------------------------ */
mogp_meanfunc* mogp_meanfunc_zero(void);                       /* ZeroMeanFunc()  */
mogp_meanfunc* mogp_meanfunc_fixed(double value);              /* FixedMeanFunc(v) */
mogp_meanfunc* mogp_meanfunc_const(void);                      /* ConstMeanFunc()  */
/* PolyMeanFunc([[dim,power],...]); parameters = [const, coeff_1 .. coeff_nterms] */
mogp_meanfunc* mogp_meanfunc_poly(const int* dims, const int* powers, int nterms);
void mogp_meanfunc_destroy(mogp_meanfunc*);
int mogp_meanfunc_n_params(const mogp_meanfunc*);
/* mean_f(xs (m,D), params) -> out (m) ; wrong params length -> "Expected params list of length N" */
int mogp_meanfunc_mean_f(const mogp_meanfunc*, const double* xs, int m, int D, const double* params, int n_params, double* out);
/* mean_deriv -> out (n_params, m) ; mean_inputderiv -> out (D, m)   (meanfunc.hpp layouts) */
int mogp_meanfunc_mean_deriv(const mogp_meanfunc*, const double* xs, int m, int D, const double* params, int n_params, double* out);
int mogp_meanfunc_mean_inputderiv(const mogp_meanfunc*, const double* xs, int m, int D, const double* params, int n_params, double* out);

/* ---- DenseGP_GPU (bindings.cu:14-257) -------------------------------------------------- */
/* DenseGP_GPU(inputs(n,D), targets(n), testing_size, meanfunc, kernel_type, nugget_type, nugget_size)
 * bindings.cu:14-15 / densegp_gpu.hpp:777-865.  The mean function is cloned. */
mogp_densegp* mogp_densegp_create(const double* inputs, int n, int D, const double* targets, unsigned testing_size,
                                  const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size);
/* Same constructor, but the coefficients of a Const / Poly mean function are integrated out
 * analytically with weak (flat) mean priors -- the CPU class's semantics (GaussianProcess.py:640-700
 * fit, :860-940 predict; linalg_utils.py:5-121) instead of living in theta.  n_mean() is then 0 and
 * the fitted coefficients are read with mogp_densegp_get_beta.  At most 7 mean terms. */
mogp_densegp* mogp_densegp_create_analytic_mean(const double* inputs, int n, int D, const double* targets, unsigned testing_size,
                                                const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size);
/* MeanPriors(mean = b, cov = B) for the analytic mean (Priors.py:423-581, GPPriors.mean): the caller passes b (q),
 * B^-1 (q x q row-major), B^-1 b (q) and log|B|; q = 0 restores weak priors.  Works on borrowed handles
 * (mogp_mogp_emulator) too, so every emulator can carry its own prior. */
int mogp_densegp_set_mean_priors(mogp_densegp*, int q, const double* b, const double* Binv, const double* Binv_b, double logdetB);
int mogp_densegp_n_beta(const mogp_densegp*);                        /* GPParams.n_mean, GPParams.py */
int mogp_densegp_get_beta(const mogp_densegp*, double* out /* n_beta */);   /* theta.mean, GaussianProcess.py:669 */
/* the reference never frees (py::nodelete); the shim may.  Must not be called on a handle
 * obtained from mogp_mogp_emulator(). */
void mogp_densegp_destroy(mogp_densegp*);

int mogp_densegp_n(const mogp_densegp*);                 /* n()        bindings.cu:19 */
int mogp_densegp_D(const mogp_densegp*);                 /* D()        :23 */
int mogp_densegp_n_corr(const mogp_densegp*);            /* n_corr()   :27 */
int mogp_densegp_n_params(const mogp_densegp*);          /* n_params() :41  (D+1+[fit]) */
int mogp_densegp_n_mean(const mogp_densegp*);            /* get_theta().get_n_mean() */
int mogp_densegp_n_data(const mogp_densegp*);            /* get_theta().get_n_data() */
int mogp_densegp_inputs(const mogp_densegp*, double* out /* n*D */);   /* inputs()  :31 */
int mogp_densegp_targets(const mogp_densegp*, double* out /* n */);     /* targets() :36 */
int mogp_densegp_theta_fit_status(const mogp_densegp*);  /* :45 */
int mogp_densegp_reset_theta_fit_status(mogp_densegp*);  /* :50 */
/* get_theta() :55 -- copies: data (n_data) and mean (n_mean) */
int mogp_densegp_get_theta(const mogp_densegp*, double* data_out, double* mean_out);
/* create_gppriors(n_corr, [(type,[a,b])...], (type,[a,b]), (type,[a,b]))  :67 / densegp_gpu.hpp:214-232 */
int mogp_densegp_create_gppriors(mogp_densegp*, int n_corr, const int* corr_types, const double* corr_params /* 2*n_corr */,
                                 int cov_type, const double* cov_params /* 2 */, int nug_type, const double* nug_params /* 2 */);
/* GPPriors.logp / dlogpdtheta / sample of the attached priors (bindings.cu:547-566) */
int mogp_densegp_priors_logp(const mogp_densegp*, const double* theta_data, int len, double* out);
int mogp_densegp_priors_dlogpdtheta(const mogp_densegp*, const double* theta_data, int len, double* out /* len */);
int mogp_densegp_priors_sample(mogp_densegp*, double* out /* n_mean + n_data */);
/* fit(theta) :147-165 / densegp_gpu.hpp:483-612 */
int mogp_densegp_fit(mogp_densegp*, const double* theta, int len);
/* get_logpost(theta) :199-206 / densegp_gpu.hpp:639-661 (refits iff theta moved) */
int mogp_densegp_get_logpost(mogp_densegp*, const double* theta, int len, double* out);
/* logpost_deriv(out) :246-256 / densegp_gpu.hpp:663-767 ; out has n_mean + n_data entries */
int mogp_densegp_logpost_deriv(mogp_densegp*, double* out, int len);
/* predict(testing (D)) :71-80 ; predict_variance :83-95 */
int mogp_densegp_predict(mogp_densegp*, const double* testing, int D, double* mean_out);
int mogp_densegp_predict_variance(mogp_densegp*, const double* testing, int D, double* mean_out, double* var_out);
/* predict_batch(testing (m,D), out (m)) :98-110 / densegp_gpu.hpp:300-338 */
int mogp_densegp_predict_batch(mogp_densegp*, const double* testing, int m, int D, double* mean_out, int out_len);
/* predict_variance_batch(testing, mean, var) :113-129 / densegp_gpu.hpp:341-408 (var WITHOUT nugget) */
int mogp_densegp_predict_variance_batch(mogp_densegp*, const double* testing, int m, int D, double* mean_out, double* var_out, int out_len);
/* predict_deriv(testing, out (m,D)) :132-144 / densegp_gpu.hpp:411-448 */
int mogp_densegp_predict_deriv(mogp_densegp*, const double* testing, int m, int D, double* out, int out_rows, int out_cols);
/* predict(full_cov=True) of the CPU class, GaussianProcess.py:899-911: mean_out (m) and the
 * m x m predictive covariance sigma^2 k(X*,X*) - (L^-1 K*)^T (L^-1 K*) [+ analytic-mean term], nugget NOT added.
 * m is not limited by testing_size; the call fails if the device scratch (2 n m + m^2 doubles per emulator) exceeds 64 GB. */
int mogp_densegp_predict_full_cov(mogp_densegp*, const double* testing, int m, int D, double* mean_out, double* cov_out /* m*m */);
/* get_K :168 (sigma^2 k(X,X), no nugget) ; get_invQ :177 ; get_invQt :187 ; get_cholesky_lower :232
 * get_cholesky_lower fills `out` so that tril(out^T) == L  (densegp_gpu.hpp:478-481) */
/* Consumers of the batched prediction, fused on the device so that a query sweep returns one
 * score per point instead of means and variances:
 *  - implausibility |z - E f(x)| / sqrt(Var f(x) [+ nugget] + discrepancy + obs_var)  (HistoryMatching.py:197-276);
 *    zero / fixed mean functions only;
 *  - leave-one-out predictive variance at every training input, 1 / [K^-1]_ii: what MICEFastGP.fast_predict(index)
 *    computes for one index from a Woodbury downdate (SequentialDesign.py:705-747), for all indices at once. */
int mogp_densegp_implausibility(mogp_densegp*, const double* testing, int m, int D, double obs, double obs_var, double discrepancy,
                                int include_nugget, double* out /* m */);
int mogp_densegp_loo_variance(mogp_densegp*, double* out /* n */);
/* Variance-based sensitivity analysis of the predictive mean f (mean function included), fused behind the batched prediction: A, B are
 * two independent host (N, D) sample matrices of the input distribution, AB_i is A with column i of B (built on the device, a chunk
 * at a time).  With f0 = mean(fA | fB): variance_out = mean((fA | fB - f0)^2), mean_out = f0,
 *   S[i]  = mean((fB - f0)(fAB_i - fA)) / variance       first order (Saltelli 2010)
 *   ST[i] = mean((fA - fAB_i)^2) / (2 variance)           total effect (Jansen)
 * and, with unc != 0, emulator_variance_out = the mean over A and B of the predictive variance as predict() reports it (nugget added
 * when include_nugget != 0, clipped at zero); it may be NULL otherwise.  A constant emulator (variance 0) gives NaN indices.
 * Refused: N < 2, samples that are not finite, a D that is not the model's, an emulator that is not fit, and an N whose means do not
 * fit half of the free device memory.  The same inputs give the same bits in every call. */
int mogp_densegp_sobol(mogp_densegp*, const double* A, const double* B, int N, int D, int unc, int include_nugget, double* S /* D */,
                       double* ST /* D */, double* mean_out, double* variance_out, double* emulator_variance_out);
/* Hessian of the negative log-posterior at theta = [corr_raw | log sigma^2 | log nugget (fit only)] (len = n_params), computed on the
 * device from Q^-1, alpha and the planes Q^-1 dQ/dtheta_p: out (len, len) row-major, both triangles, exactly symmetric.  An adaptive or
 * fixed nugget is a constant, as in the gradient.  The cached state of an emulator that is fit stays what it was (one fit at exactly theta is
 * not evaluated again, one fit elsewhere is put back); an emulator that was not fit is left fit at theta.  The same inputs give the same
 * bits in every call.  Refused: nugget type "pivot", the analytic mean, a mean function with parameters in theta, the ProductMat52
 * kernel, and a theta at which the covariance matrix cannot be factorised. */
int mogp_densegp_logpost_hessian(mogp_densegp*, const double* theta, int len, double* out /* len*len */);
/* Prediction averaged over S hyperparameter samples (law of total variance), reduced over the samples on the device.  thetas (S, len): full
 * vectors [mean | data], len = n_params.  EXACTLY ONE of weights (S, non-negative, any scale) and log_q (S, the log proposal density up to
 * a constant) is not NULL; with log_q the weights are w_s ~ exp(-(F_s - F_min) - (log_q_s - log_q at the arg-min)), F the negative
 * log-posterior (self-normalised importance sampling).  Every sample is factored on a replica engine, S at a time or max_slots (0: the
 * library's choice) -- an adaptive nugget runs its jitter ladder per sample -- and the emulator itself, which must be fit, keeps its
 * factor, theta and log-posterior.  A sample that cannot be factorised gets ok_out = 0, weight 0 and logpost_out NaN; the others are
 * normalised to sum 1.  With mu_s, var_s the prediction of sample s, the PIVOT mu_0 = the mean of sample 0 (whatever its weight; the first
 * sample with ok = 1 where sample 0 failed) and d_s = mu_s - mu_0:
 *   mean_out = mu_0 + sum w_s d_s,   within_out = sum w_s max(var_s + (include_nugget ? nugget of sample s : 0), 0),
 *   between_out = max(sum w_s d_s^2 - (sum w_s d_s)^2, 0)                                    (m each; the total variance is their sum)
 * All samples failing, or weights that sum to 0, give NaN in all three and in weights_out -- status 0, not an error.  The sums are taken in
 * sample order with one add per sample and no atomics: the same inputs give the same bits in every call, for every max_slots >= 1 and
 * every max_points >= 1 (query points per chunk; 0: the library's choice).  Refused: nugget type "pivot", the analytic mean, S < 1,
 * non-finite thetas / weights / log_q / testing, negative weights, D other than the emulator's, an emulator that is not fit. */
int mogp_densegp_predict_mixture(mogp_densegp*, const double* thetas /* S*len */, int S, int len, const double* weights /* S or NULL */,
                                 const double* log_q /* S or NULL; exactly one of the two */, const double* testing, int m, int D,
                                 int include_nugget, int max_slots, int max_points, double* mean_out, double* within_out,
                                 double* between_out /* m each */, double* weights_out, double* logpost_out, int* ok_out /* S each */);
/* Leave-one-out / k-fold cross-validation of a fitted emulator at its fitted hyperparameters, on the device and without refitting.
 * labels (n_labels = n): the fold of every training point, values 0 .. k-1, every fold non-empty, 2 <= k <= n; k = n with one point per
 * fold is leave-one-out (one pass over L^-1).  With Q the factored matrix (nugget included), alpha = Q^-1 (t - m(X)) and
 * S = (Q^-1)_FF of a fold F, the held-out error is e_F = S^-1 alpha_F and the held-out covariance of the observations S^-1:
 *   mean_out[i] = t_i - e_i,   var_out[i] = (S^-1)_ii  (include_nugget = 0: max(that - the nugget used, 0))              (n each)
 *   maha_out[f] = e_F^T S e_F,   log_score_out[f] = log density of t_F given the other folds,   ok_out[f] = 1           (k each)
 * A fold whose S cannot be factorised gets NaN for its points and scalars and ok_out = 0 (no jitter, status 0).  The folds go through a
 * scratch engine max_slots at a time (0: the library's choice); the emulator keeps its factor, theta and log-posterior.  No atomics: the
 * same call returns the same bits.  Refused: nugget type "pivot", the analytic mean, an emulator that is not fit, k < 2 or k > n, a label
 * outside [0, k), an empty fold, n_labels != n. */
int mogp_densegp_cross_validate(mogp_densegp*, const int* labels, int n_labels, int k, int include_nugget, int max_slots,
                                double* mean_out, double* var_out /* n each */, double* maha_out, double* log_score_out,
                                int* ok_out /* k each */);
/* S joint draws f(X*) ~ N(mu*, Sigma~) of a fitted emulator at the m points testing (m, D), on the device.  With mu* and Sigma* what
 * mogp_densegp_predict_full_cov returns (the same launches, the same bits; nugget not included):
 *   Sigma~ = Sigma* + ((include_nugget ? nugget used by the fit : 0) + jitter + delta) I = L L^T,   samples_out[s][:] = mu* + L z[s][:]
 * Jitter ladder: delta = 0 on the first try; where Sigma~ does not factorise it is tried again with delta = mean(diag Sigma*) 1e-6 10^t,
 * t = 0 .. 4 (the adaptive-nugget rule of the fit); jitter_used_out = jitter + delta.  After the fifth failure ok_out = 0 and samples_out
 * is NaN -- status 0, not an error.
 * Normals: z_in (S, m), the caller's (z_in_per_emulator is ignored for a single emulator), or NULL: generated on the device by a
 * counter-based generator, so that a value depends on (seed, stream, draw s, point j) alone and never on how the work was cut:
 * Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed & 0xffffffff, seed >> 32),
 * counter = (p, s, stream0, 0) with p = j >> 1; from the output words x0 .. x3
 *   u1 = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53 in (0, 1],   u2 = ((x2 >> 5) 2^26 + (x3 >> 6)) 2^-53 in [0, 1),
 *   r = sqrt(-2 ln u1),   z[2p] = r cos(2 pi u2),   z[2p + 1] = r sin(2 pi u2)          (an odd m drops the last sine).
 * z_out (S, m) or NULL: the normals used.  mean_out (m) = mu*.  The draws go max_draws per chunk (0: the library's choice) through a
 * scratch engine of m rows; everything is scratch of the call, the emulator keeps its factor, theta and log-posterior.  One writer per
 * output, a fixed summation order, no atomics: the same call returns the same bits, and max_draws changes none.  Refused: nugget type
 * "pivot", the analytic mean, an emulator that is not fit, D other than the emulator's, non-finite testing or z_in, S < 1, jitter < 0,
 * negative max_slots / max_draws, scratch of more than half of the free device memory for one emulator and one tile of 64 draws, and
 * what predict_full_cov's 64 GB rule refuses. */
int mogp_densegp_sample_posterior(mogp_densegp*, const double* testing, int m, int D, int S, unsigned long long seed, unsigned int stream0,
                                  const double* z_in /* S*m or NULL */, int z_in_per_emulator, int include_nugget, double jitter,
                                  int max_slots, int max_draws, double* samples_out /* S*m */, double* mean_out /* m */,
                                  double* z_out /* S*m or NULL */, double* jitter_used_out /* 1 */, int* ok_out /* 1 */);
/* Posterior covariance of the latent function between two point sets at the fitted hyperparameters, on the device.  With Q = K + nugget I
 * = L L^T as the fit left it and v(x) = L^-1 k(x):
 *   cov_out[i][j] = c(x1_i, x2_j) = sigma^2 k(x1_i, x2_j) - v(x1_i)^T v(x2_j)                         X1 (m1, D), X2 (m2, D), cov_out (m1, m2)
 * -- the off-diagonal block of mogp_densegp_predict_full_cov on the stacked set, without the two diagonal blocks; nugget not included.
 * X2 = NULL: X2 = X1 (m2 is ignored).  V = L^-1 K*^T of either set is built with predict_full_cov's launches and the product runs on fp64
 * MFMA with sigma^2 k formed in its epilogue.  One writer per output, a fixed summation order: the same call returns the same bits.
 * Refused: nugget type "pivot", the analytic mean, an emulator that is not fit, D other than the emulator's, non-finite points, m < 1,
 * negative max_slots, and scratch (V of both sets, the output, the cross-covariance scratch) of more than 64 GB or more than half of the
 * free device memory for one emulator. */
int mogp_densegp_predict_cov(mogp_densegp*, const double* X1, int m1, const double* X2 /* or NULL */, int m2, int D, int max_slots,
                             double* cov_out /* m1*m2 */);
/* The ALC (active learning Cohn) design criterion: how much one more run at a candidate c, with noise variance tau >= 0, reduces the
 * latent predictive variance summed over reference points r_j with weights w_j >= 0.  With c(.,.) as above and s^2(x) = max(c(x, x), 0):
 *   reduction_out[i] = sum_j w_j c(r_j, c_i)^2 / (s^2(c_i) + tau)                        candidates (m_c, D), reference (m_r, D), weights (m_r)
 *   cand_var_out[i] = s^2(c_i),   ref_var_out[j] = s^2(r_j)     -- the predictive-variance launches of mogp_densegp_predict_variance_batch:
 *                                                                   the same bits as its variances clipped at 0
 * The integrated variance after the run is sum_j w_j s^2(r_j) - reduction_out[i].  noise (1) or NULL: the nugget of the fit
 * (mogp_densegp_get_nugget_size).  Floor: a candidate with s^2 + tau <= (n + 2) 2^-52 sigma^2 -- the rounding of sigma^2 minus a sum of n
 * squares -- gets reduction_out = 0 and degenerate_out = 1 (a candidate on a training point of an emulator without nugget); never NaN.
 * The m_c x m_r matrix is never formed: one workgroup per 128 x 128 tile squares, weights and sums it along the reference points, one
 * partial per (128-point tile of the WHOLE reference set, candidate), added in ascending tile order.  The reference points go max_points per
 * chunk (rounded down to a multiple of 128, at least 128; 0: the library's choice); no atomics: the same call returns the same bits, and
 * max_points changes none.  Refused: what mogp_densegp_predict_cov refuses (the scratch rule: one emulator with one 128-point chunk must
 * fit half of the free device memory), negative or non-finite weights or noise, weights that sum to 0, negative max_points. */
int mogp_densegp_alc(mogp_densegp*, const double* candidates, int m_c, const double* reference, int m_r, int D, const double* weights,
                     const double* noise /* 1 or NULL */, int max_slots, int max_points, double* reduction_out, double* cand_var_out /* m_c each */,
                     double* ref_var_out /* m_r */, int* degenerate_out /* m_c */);
/* A greedy ALC batch: n_points picks, the posterior conditioned on each pick before the next is scored, all on the device.  At fixed
 * hyperparameters the predictive variance does not depend on the targets: a run at p with noise tau appends one row to the Cholesky factor,
 * which gives every stored v(x) = L^-1 k(x) one more entry u(x) = c(x, p) / sqrt(s^2(p) + tau); c_new(x, x') = c(x, x') - u(x) u(x'),
 * s^2_new(x) = s^2(x) - u(x)^2.  candidates (m, D): the first n_forced of them are points already submitted -- steps 0 .. n_forced - 1
 * condition on them in order and mask them --, the other n_points steps pick the unmasked candidate with the largest reduction (ties: the
 * lowest index; a picked candidate is never picked again).  T = n_forced + n_points steps in all; step t scores with the ALC launches
 * over n + t rows (floor: (n + t + 2) 2^-52 sigma^2).  A step whose best score is not above 0 or whose denominator is at or below that
 * floor picks -1 and conditions on nothing (a forced step: only the floor is tested); never NaN, nothing raised.
 *   picks_out (T): candidate index or -1;   pick_red_out (T): its reduction, 0 for -1
 *   red_out / deg_out (T, m) or NULL: every step's reduction and degenerate flags
 *   cand_var_out (m), ref_var_out (m_r): s^2 before any step, the bits of mogp_densegp_alc;   ref_var_after_out (m_r): after the last
 *   iv_out (T + 1): iv[0] = sum_j w_j ref_var[j] in ascending j, iv[t + 1] = iv[t] - pick_red[t]
 * The picks are enqueued back to back: one download at the end (and each step's rows where red_out / deg_out are given).  No atomics:
 * the same call returns the same bits.  Refused: what mogp_densegp_alc refuses, n_points < 1, n_points > m - n_forced, and scratch beyond
 * half of the free device memory (V of both sets with roundup(T, 16) more rows, the whole reference set resident). */
int mogp_densegp_alc_batch(mogp_densegp*, const double* candidates, int m, int n_forced, const double* reference, int m_r, int D,
                           const double* weights, const double* noise /* 1 or NULL */, int n_points, int max_slots, int* picks_out,
                           double* pick_red_out, double* red_out, int* deg_out, double* cand_var_out, double* ref_var_out,
                           double* ref_var_after_out, double* iv_out);
int mogp_densegp_get_K(mogp_densegp*, double* out /* n*n */);
int mogp_densegp_get_invQ(mogp_densegp*, double* out /* n*n */);
int mogp_densegp_get_invQt(mogp_densegp*, double* out /* n */);
int mogp_densegp_get_cholesky_lower(mogp_densegp*, double* out /* n*n */);
/* ChoInvPivot.P of the current fit (linalg/cholesky.py:82-104): K[P][:, P] = L L^T with L = get_cholesky_lower; the identity
 * and rank n for the other nugget types.  rank_out may be NULL. */
int mogp_densegp_get_pivot(mogp_densegp*, int* P_out /* n */, int* rank_out);
/* pivot_cholesky(A), linalg/cholesky.py:284-327 (LAPACK dpstrf + the replacement diagonal of the skipped rows), for any
 * symmetric matrix with positive diagonal: host buffers, row-major; L_out lower triangular, P_out zero-based. */
int mogp_pivot_cholesky(const double* A, int n, double* L_out /* n*n */, int* P_out /* n */, int* rank_out);
double mogp_densegp_get_nugget_size(const mogp_densegp*);     /* :209 */
int mogp_densegp_set_nugget_size(mogp_densegp*, double);      /* :213 */
int mogp_densegp_get_nugget_type(const mogp_densegp*);        /* :217 */
int mogp_densegp_set_nugget_type(mogp_densegp*, int);         /* :221 */
int mogp_densegp_get_kernel_type(const mogp_densegp*);        /* :225 */
/* fit_GP_MAP(DenseGP_GPU&, n_tries, theta0)  bindings.cu:602-603 / fitting.hpp:61-120.
 * theta0_len == 0 means "no theta0".  Failed starts are skipped; if all fail the emulator is
 * left "not fit" (fitting.hpp:111-113) and the call still returns 0. */
int mogp_fit_single_GP_MAP(mogp_densegp*, int n_tries, const double* theta0, int theta0_len);

/* ---- MultiOutputGP_GPU (bindings.cu:260-337) ------------------------------------------- */
/* MultiOutputGP_GPU(inputs(n,D), targets (n_out,n), testing_size, meanfunc, kernel, nugget_type, nugget_size) */
mogp_mogp* mogp_mogp_create(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                            const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size);
mogp_mogp* mogp_mogp_create_analytic_mean(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                                          const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size);
/* The same model spread over several devices in one process: the emulators are split into contiguous blocks of ceil(n_out / n_devices)
 * (dist.shard_bounds), empty blocks are dropped, and part k holds one engine on devices[k] for its block.  A device may be repeated
 * (parts on one device run one after the other); an ordinal outside [0, device count) is refused.  analytic_mean as
 * mogp_mogp_create_analytic_mean.  Every mogp_mogp_* entry works on the result; each call runs the parts on one host thread each. */
mogp_mogp* mogp_mogp_create_on_devices(const double* inputs, int n, int D, const double* targets, int n_out, unsigned testing_size,
                                       const mogp_meanfunc* mean, int kernel_type, int nugget_type, double nugget_size, int analytic_mean,
                                       const int* devices, int n_devices);
void mogp_mogp_destroy(mogp_mogp*);
/* number of parts (1 for a handle created without a device list); part k: its device and emulator block [lo, hi) */
int mogp_mogp_n_parts(const mogp_mogp*);
int mogp_mogp_part(const mogp_mogp*, int k, int* device, int* lo, int* hi);
int mogp_mogp_n(const mogp_mogp*);
int mogp_mogp_D(const mogp_mogp*);
int mogp_mogp_n_emulators(const mogp_mogp*);
int mogp_mogp_inputs(const mogp_mogp*, double* out);
int mogp_mogp_targets(const mogp_mogp*, double* out /* n_out*n */);
/* emulator(i): borrowed DenseGP handle sharing the container's device state (bindings.cu:275) */
mogp_densegp* mogp_mogp_emulator(mogp_mogp*, int index);
int mogp_mogp_get_nugget_type(const mogp_mogp*);
double mogp_mogp_get_nugget_size(const mogp_mogp*);
/* get_fitted_indices / get_unfitted_indices: writes up to n_emulators ints, returns the count */
int mogp_mogp_get_fitted_indices(const mogp_mogp*, int* out);
int mogp_mogp_get_unfitted_indices(const mogp_mogp*, int* out);
int mogp_mogp_reset_fit_status(mogp_mogp*);
/* create_priors_for_emulator(i, ...) multioutputgp_gpu.hpp:124-134 */
int mogp_mogp_create_priors_for_emulator(mogp_mogp*, int index, int n_corr, const int* corr_types, const double* corr_params,
                                         int cov_type, const double* cov_params, int nug_type, const double* nug_params);
/* fit(thetas (n_out, n_params)) multioutputgp_gpu.hpp:223-228 : ONE batched device pass over all emulators */
int mogp_mogp_fit(mogp_mogp*, const double* thetas, int n_rows, int n_cols);
int mogp_mogp_fit_emulator(mogp_mogp*, int index, const double* theta, int len);
/* batched objective / gradient for all emulators at once (what fit_GP_MAP iterates on):
 * logpost_out (n_out), grad_out (n_out, n_params) may be NULL; ok_out (n_out) 1 = factorised */
int mogp_mogp_eval(mogp_mogp*, const double* thetas, int n_rows, int n_cols, double* logpost_out, double* grad_out, int* ok_out);
/* predict_batch(testing (m,D), out (n_out,m)) :170-179 ; predict_variance_batch :182-192 ; predict_deriv (n_out,m,D) :195-203
 * unfit emulators are skipped (their rows are left untouched), as in the reference. */
int mogp_mogp_predict_batch(mogp_mogp*, const double* testing, int m, int D, double* means);
int mogp_mogp_predict_variance_batch(mogp_mogp*, const double* testing, int m, int D, double* means, double* vars);
int mogp_mogp_predict_deriv(mogp_mogp*, const double* testing, int m, int D, double* derivs);
/* full predictive covariance of every fitted emulator in one batched pass: means (n_out, m), covs (n_out, m, m) */
/* multi-output implausibility: obs / obs_var / discrepancy (n_out); out[j] = the (rank+1)-th largest of the n_out
 * per-output implausibilities at query point j (rank 0 = maximum; forced to 0 for one output; rank <= 15) */
int mogp_mogp_implausibility(mogp_mogp*, const double* testing, int m, int D, const double* obs, const double* obs_var,
                             const double* discrepancy, int include_nugget, int rank, double* out /* m */);
int mogp_mogp_predict_full_cov(mogp_mogp*, const double* testing, int m, int D, double* means, double* covs);
/* mogp_densegp_sobol for every emulator in one batched pass per part: S, ST (n_out, D), mean_out, variance_out and
 * emulator_variance_out (n_out).  Rows of emulators that are not fit are filled with NaN. */
int mogp_mogp_sobol(mogp_mogp*, const double* A, const double* B, int N, int D, int unc, int include_nugget, double* S, double* ST,
                    double* mean_out, double* variance_out, double* emulator_variance_out);
/* mogp_densegp_logpost_hessian for every emulator in one batched call per part: thetas (n_rows = n_emulators, n_cols = the largest
 * n_params of the model), row i read up to emulator i's own n_params; hess_out (n_rows, n_cols, n_cols) with the leading block of every
 * emulator filled and NaN elsewhere.  ok_out[i] = 0 and a NaN block where the factorisation fails at row i, or where the row starts
 * with NaN (the emulator is then skipped); the other emulators are not affected. */
int mogp_mogp_hessian(mogp_mogp*, const double* thetas, int n_rows, int n_cols, double* hess_out /* n_rows*n_cols*n_cols */, int* ok_out);
/* mogp_densegp_predict_mixture for every emulator, all (emulator, sample) pairs of a part in one batched pass: thetas (n_out, S, n_cols),
 * n_cols = the largest n_params of the model, every row read up to its emulator's own n_params; weights / log_q (n_out, S);
 * mean_out / within_out / between_out (n_out, m); weights_out / logpost_out / ok_out (n_out, S); ok_all_out (n_out, may be NULL) = 0
 * where the emulator's rows are NaN.  Row e is bit for bit what the single-emulator call gives for emulator e.  Emulators that are not
 * fit give NaN rows, ok_out = 0 and ok_all_out = 0 (their thetas, weights and log_q are not read). */
int mogp_mogp_predict_mixture(mogp_mogp*, const double* thetas, int S, int n_cols, const double* weights, const double* log_q,
                              const double* testing, int m, int D, int include_nugget, int max_slots, int max_points, double* mean_out,
                              double* within_out, double* between_out, double* weights_out, double* logpost_out, int* ok_out,
                              int* ok_all_out);
/* mogp_densegp_cross_validate for every emulator with the same folds, all (emulator, fold) pairs of a part in batched passes: mean_out /
 * var_out (n_out, n), maha_out / log_score_out / ok_out (n_out, k).  Emulators that are not fit give NaN rows and ok_out = 0. */
int mogp_mogp_cross_validate(mogp_mogp*, const int* labels, int n_labels, int k, int include_nugget, int max_slots, double* mean_out,
                             double* var_out, double* maha_out, double* log_score_out, int* ok_out);
/* mogp_densegp_sample_posterior for every emulator, max_slots emulators per pass (0: the library's choice): samples_out (n_out, S, m),
 * mean_out (n_out, m), z_out (n_out, S, m) or NULL, jitter_used_out / ok_out (n_out).  z_in: (S, m) shared by all emulators, with
 * z_in_per_emulator (n_out, S, m), or NULL.  Emulator e draws from stream stream0 + e, e its index in the model whatever part it lies in:
 * its normals are those of the single-emulator call with that stream.  Only the emulators whose Sigma~ fails are tried again on the
 * jitter ladder.  Emulators that are not fit give NaN rows, jitter_used_out NaN and ok_out = 0. */
int mogp_mogp_sample_posterior(mogp_mogp*, const double* testing, int m, int D, int S, unsigned long long seed, unsigned int stream0,
                               const double* z_in, int z_in_per_emulator, int include_nugget, double jitter, int max_slots, int max_draws,
                               double* samples_out, double* mean_out, double* z_out, double* jitter_used_out, int* ok_out);
/* mogp_densegp_predict_cov for every emulator, max_slots emulators per group (0: the library's choice): cov_out (n_out, m1, m2).  Row e
 * is bit for bit the single-emulator call.  Emulators that are not fit give NaN rows. */
int mogp_mogp_predict_cov(mogp_mogp*, const double* X1, int m1, const double* X2 /* or NULL */, int m2, int D, int max_slots, double* cov_out);
/* mogp_densegp_alc for every emulator with the same candidates, reference points and weights: noise (n_out) or NULL (every emulator's own
 * nugget); reduction_out / cand_var_out / degenerate_out (n_out, m_c), ref_var_out (n_out, m_r).  Row e is bit for bit the single-emulator
 * call, whatever max_slots and max_points.  Emulators that are not fit give NaN rows and degenerate_out = 0 (their noise is not read). */
int mogp_mogp_alc(mogp_mogp*, const double* candidates, int m_c, const double* reference, int m_r, int D, const double* weights,
                  const double* noise /* n_out or NULL */, int max_slots, int max_points, double* reduction_out, double* cand_var_out,
                  double* ref_var_out, int* degenerate_out);
/* mogp_densegp_alc_batch for every emulator; arrays gain a leading n_out.  select_total = 0: every emulator its own batch; row e is bit
 * for bit the single-emulator call, whatever max_slots and the split over devices.  select_total = 1: ONE batch for the model: in each
 * free step the candidate with the largest sum over the fitted emulators of red_e / IV_e (IV_e: emulator e's integrated variance before
 * that step; an emulator whose IV is not above 0 adds nothing), formed on the host in ascending emulator order from the downloaded rows,
 * ties to the lowest index; total_picks_out (n_forced + n_points) receives it, -1 from the step at which no score is above 0.  An
 * emulator for which that candidate is at or below its own floor has picks_out = -1 in that step and is not conditioned.  All fitted
 * emulators of a device must fit one group; refused otherwise, with the bytes named.  Once stopped, the later rows of red_out are 0.
 * Emulators that are not fit: NaN rows, deg_out = 0, and picks_out left as the caller set them (their noise is not read). */
int mogp_mogp_alc_batch(mogp_mogp*, const double* candidates, int m, int n_forced, const double* reference, int m_r, int D,
                        const double* weights, const double* noise /* n_out or NULL */, int n_points, int select_total, int max_slots,
                        int* picks_out, double* pick_red_out, double* red_out /* or NULL */, int* deg_out /* or NULL */, double* cand_var_out,
                        double* ref_var_out, double* ref_var_after_out, double* iv_out, int* total_picks_out /* NULL with select_total = 0 */);
/* predict_variance_batch (multioutputgp_gpu.hpp:182-192) with DEVICE pointers: inputs already resident in HBM, results stay in HBM
 * (every mean function; rows of emulators that are not fit are filled with NaN, MultiOutputGP_GPU.py:288-296) */
int mogp_mogp_predict_variance_batch_dev(mogp_mogp*, const double* d_testing, int m, int D, double* d_means, double* d_vars);
/* the same with the input derivatives of predict_deriv (multioutputgp_gpu.hpp:195-203) in the same pass: d_derivs (n_out, m, D) device
 * buffer; d_vars and d_derivs may be NULL.  What one rank of a sharded predict hands to the single RCCL gather (dist.py). */
int mogp_mogp_predict_dev(mogp_mogp*, const double* d_testing, int m, int D, double* d_means, double* d_vars, double* d_derivs);
/* fit_GP_MAP(MultiOutputGP_GPU&, n_tries, theta0) bindings.cu:604-605 / fitting.hpp:122-128.
 * All emulators advance in lock-step: each L-BFGS iteration is one batched device evaluation. */
int mogp_fit_GP_MAP(mogp_mogp*, int n_tries, const double* theta0, int theta0_len);
/* optimiser controls (not in the reference API; defaults reproduce fitting.hpp's stop rule 1e-9) */
int mogp_set_fit_options(int max_iter, double ftol, double gtol, unsigned long long seed);

/* ---- stand-alone kernel objects: SquaredExponentialKernel / Matern52Kernel .kernel_f / kernel_deriv / kernel_inputderiv
   (mogp_gpu/src/bindings.cu:340-361, kernel.hpp:47-107; CPU counterparts Kernel.py:99-173).
   kernel_type as the enum above (+ 2 ProductMat52, 3 UniformSqExp, 4 UniformMat52); x1 (n1, D), x2 (n2, D) row-major;
   params = [corr_raw.., log sigma^2] (n_corr + 1, n_corr = D or 1 for the uniform kernels).
   what = 0: out (n1, n2)            = sigma^2 k(x1_i, x2_j)
   what = 1: out (n_corr + 1, n1, n2) = d/d theta_p (last plane: d/d log sigma^2 = K)
   what = 2: out (n2, n1, D)         = d/d x1_i[d]   (the flat order of the reference's CUDA kernel, kernel.cu:86-100) */
int mogp_kernel_eval(int kernel_type, int what, const double* x1, int n1, const double* x2, int n2, int D, const double* params,
                     int n_params, double* out);

/* ---- measurement hooks (bench.py only) -------------------------------------------------- */
/* when enabled, HIP events are recorded on the launch stream around every launch of the tagged kernels */
int mogp_profile_enable(int on);
int mogp_profile_reset(void);
/* force the Cholesky schedule (0 two emulator groups, 1 right-looking, 3 look-ahead, 4 one launch / task queue, 5 the multi-launch
   schedule the library would pick without the one-launch kernel, -1 the library's choice) and / or
   serialise it onto one stream, so that the HIP-event time of a kernel is its time alone on the device */
int mogp_profile_schedule(int schedule, int single_stream);
/* sums over launches since reset: total milliseconds, launch count, algorithmic flops and bytes */
int mogp_profile_get(const char* kernel_tag, double* total_ms, long long* launches, double* alg_flops, double* alg_bytes);
/* The per-emulator task order of the one-launch Cholesky (kernels_mchol.hip) for n_plus_rhs = n + number of right-hand-side rows,
   padded to a multiple of 128: entry = (type << 30) | (block column c << 15) | 64-row block r; type 0 D(c): diagonal block, 1 G(s, c): lower
   64 x 64 tile s = 0, 1, 2 of the diagonal block (s in the r field) receives the panels 0 .. c-2, 2 T(r, c): panel tile receives the panels 0 .. c-1 and is solved.  Writes up to
   `capacity` entries, returns the number of tasks.  Host-only (no device needed): the CPU suite checks that the order is
   topological, which is what the kernel's forward-progress argument rests on. */
int mogp_mchol_task_table(int n_plus_rhs, int* out, int capacity);
/* The order launches with enough workgroups per queue use (kernels_mchol.hip, mchol_task_table): the same tasks, the band tasks of an
   iteration -- entries with bit 29 set; the block column is bits 15..28 -- listed directly in front of the diagonal block they wait for, at
   most 6 places ahead of it with only such entries in between.  The CPU suite checks exactly that bound. */
int mogp_mchol_task_table_ahead(int n_plus_rhs, int* out, int capacity);
/* process-wide diagnostic counters: "backsolve_timeouts" = back substitutions that were repeated with the multi-launch
   path because a wait of the one-launch chain timed out (0 in normal operation); "mchol_aborts" = factorisations the
   one-launch Cholesky gave up on and a multi-launch schedule repeated (0 in normal operation); "objective_evals" / "gradient_evals" =
   emulator objective evaluations so far (all / with gradient), e.g. to turn a fit_GP_MAP wall time into evaluations/s;
   "alpha_solves" = emulators whose K^-1 t was solved -- with the evaluation (gradient, analytic mean, pivot) or by the first call that
   read it after an objective-only evaluation, which leaves it out;
   "lbfgs_runs" / "lbfgs_iterations" / "linesearch_shortened" / "linesearch_lengthened" = optimiser runs started by fit_GP_MAP,
   their accepted steps, and the line-search trial points that failed the sufficient-decrease / the curvature test;
   round 6, the slot pool of fit_GP_MAP: "pool_rounds" = batched optimiser rounds, "pool_slot_rounds" = sum over them of the runs that took
   part (/ rounds = mean batch), "retargets" / "retarget_us" = replica slots handed to another emulator and the host time that took,
   "replica_engine_build_us" / "replica_pool_us" = host time constructing (or re-taking) the replica engine / inside the pool,
   "replica_engines_reused" = multi-start fits that ran on the replica engine the previous one left behind (MOGP_REPLICA_CACHE) */
int mogp_profile_counter(const char* name, long long* out);
/* gKDR dimension reduction (mogp_emulator/DimensionReduction.py:132-236) over a grid of kernel scales, in one call.  X (n, m) and y (n)
   row-major; sgx2 (nx) / sgy2 (ny): the squared input / output kernel scales SGX^2, SGY^2 (positive); eps: the regularisation EPS >= 0
   (A = Kx + n eps I).  R_out (nx * ny, m, m): R of every pair (sgx2[i], sgy2[j]) at index i * ny + j.  info_out (nx): non-zero when A of
   input scale i is not positive definite (the R of its pairs are NaN).  max_pairs_per_pass: pairs per device pass, 0 = sized by the free
   device memory; R does not depend on it, bit for bit. */
int mogp_gkdr_R(const double* X, int n, int m, const double* y, int nx, const double* sgx2, int ny, const double* sgy2, double eps,
                int max_pairs_per_pass, double* R_out, int* info_out);
/* Maximin design scoring (mogp_emulator/ExperimentalDesign.py:663-668): designs (T, n, D) row-major, T >= 1 designs of n >= 2 points in
   1 <= D <= 80 dimensions; out (T): out[t] = min over i < j of the Euclidean distance of points i and j of design t (the squared
   differences summed in ascending d without fused multiply-add; one square root, of the minimum).  The designs pass through the device
   64 MiB at a time, so T is not bounded by device memory; the result does not depend on the split.  n <= 370688.  The designs must be
   finite and their squared distances must not overflow: a NaN coordinate is NOT reported (the minimum skips it), and out[t] is
   +infinity when every squared distance of design t overflows.  (The Python shim rejects non-finite designs before the call.) */
int mogp_design_min_pdist(const double* designs, int T, int n, int D, double* out);
/* Optimised maximin Latin hypercubes: C >= 1 independent chains of column-swap threshold accepting on Morris & Mitchell's criterion
   Phi = sum over i < j of 1 / R_ij^q, R_ij the integer squared distance of rows i and j of a level matrix (DESIGN.md section 3 "Design" states
   every operation; tests/lhs_restate.py restates it in NumPy, bit for bit).  start (C, n, D) row-major: the start of every chain, each column
   a permutation of 0 .. n-1.  2 <= n, 1 <= D <= 80, n_steps >= 0 proposals per chain, q >= 1, theta0 >= 0 the first threshold, multiplied by
   0 < rho <= 1 after every stage >= 1 proposals.  Chain c draws proposal t from the Philox4x32-10 block of counter (t low, t high, stream + c, 0)
   under key `seed`, so chain c of a call equals a one-chain call with stream + c and start c.  The level matrix must fit the LDS of one
   workgroup: n * D <= 75264 for n <= 65536, n * D <= 70816 above; and (D (n - 1)^2)^q must stay below 2^1000.  Outputs per chain:
   best_out (C, n, D) the visited state of smallest running Phi (the first on a tie), phi_out (C) its Phi computed from scratch, minr_out (C)
   its smallest R_ij, pairs_out (C) the number of pairs i < j at that minimum, accepted_out (C) the accepted proposals.  n_steps = 0 returns the
   starts with their criteria. */
int mogp_design_anneal_lhs(const int* start, int C, int n, int D, long long n_steps, int q, double theta0, double rho, long long stage,
                           unsigned long long seed, unsigned int stream, int* best_out, double* phi_out, long long* minr_out,
                           long long* pairs_out, long long* accepted_out);

/* ---- local approximate GP prediction for large designs (mogp_emulator_amd/LocalGP.py) ---- */
/* The handle keeps the design `inputs` (N, D) and E rows of residual targets `residuals` (E, N) -- targets minus the mean function -- on
   device `device` (< 0: the current device); N < 2^31 - 256, 1 <= D <= 80.  NULL on failure. */
typedef struct mogp_local mogp_local;
mogp_local* mogp_local_create(const double* inputs, long long N, int D, const double* residuals, int E, int device);
/* Predict the residual of row `emulator` at `testing` (m, D) from the k nearest design points of every query, 1 <= k <= min(N, 126).
   kernel_type: 0 squared exponential, 1 Matern 5/2 of the scaled distance; scale (D): s_d = sqrt(exp(theta_d)).  The device forms
   x~ = x_d * s_d and q~ = q_d * s_d (one rounded multiply each) and r2 = ((0 + t_0 t_0) + t_1 t_1) + ..., t_d = x~_d - q~_d, in the order
   d = 0 .. D-1, every operation rounded on its own (no fused multiply-add).  The neighbours of a query are the k smallest pairs
   (r2, index) in lexicographic order, listed ascending: neighbours_out (m, k) or NULL, radius_out (m) = the r2 of the last one.
   mean_out (m) = y^T Q^-1 k*, var_out (m, or NULL) = max(sigma2 - k*^T Q^-1 k* + (include_nugget ? nugget : 0), 0) with
   Q = sigma2 k(.,.) + (nugget + jitter) I over the neighbours; ok_out (m) = 0 where Q is not positive definite (mean and variance NaN).
   max_points: queries per device pass, 0 = sized by the free device memory; no result bit depends on it. */
int mogp_local_predict(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, double jitter,
                       int include_nugget, const double* testing, int m, int D, int k, int max_points, double* mean_out, double* var_out,
                       int* ok_out, double* radius_out, int* neighbours_out);
/* ---- Vecchia likelihood on the same handle (mogp_emulator_amd/Vecchia.py) ----
   The design of the handle counts as ORDERED: log p(y) ~ sum_t log p(y_t | y_c(t)), c(t) = the min(t, k) nearest rows among the rows < t.
   mogp_local_vecchia_neighbours searches c(t) for every row in the metric of scale (D), s_d = sqrt(exp(theta_d)), 1 <= k <= min(N - 1, 126),
   and keeps the (N, k) lists on the device for every later mogp_local_vecchia_loglik.  The arithmetic is that of mogp_local_predict: x~ = x_d *
   s_d (one rounded multiply), r2 = ((0 + t_0 t_0) + t_1 t_1) + ... with t_d = x~_id - x~_td in the order d = 0 .. D-1, every operation rounded
   on its own (no fused multiply-add); the list of row t holds the min(t, k) smallest pairs (r2, i), i < t, in lexicographic order -- nearest
   first, ties to the lowest row -- and -1 behind them.  neighbours_out (N, k) or NULL.  A later search replaces the lists. */
int mogp_local_vecchia_neighbours(mogp_local* h, const double* scale, int k, int* neighbours_out);
/* The Vecchia log-likelihood of residual row `emulator` (zero mean) on the lists of the last search; k must be the k of that search, scale
   need not be its scale.  kernel_type: 0 squared exponential, 1 Matern 5/2 of the scaled distance.  Per row t with n_t = min(t, k) + 1 and
   A = sigma2 k(r2) + (nugget + jitter) I over (c(t), t), A = L L^T, e the last row:
     terms_out[t] = log N(y_t | y_c(t)) = -log L_ee - (L^-1 y)_e^2 / 2 - log(2 pi) / 2
   value_out (1) = the sum of the terms; with want_grad != 0, grad_out (D + 2) = its derivatives with respect to theta_d = log s_d^2
   (d < D: r2 = sum_d exp(theta_d) (x_id - x_jd)^2, one entry per dimension whatever the kernel), log sigma2 (entry D) and log nugget
   (entry D + 1; jitter is a constant), formed analytically from w = A^-1 e and alpha = A^-1 y.  ok_out (N, or NULL) = 0 where A is not
   positive definite or the term is not finite: that term and that row's derivatives are NaN, and so are value_out and grad_out; no other
   row is affected.  terms_out (N) or NULL.  No atomics: value and gradient are summed over the rows in blocks of 1024 in a fixed tree, an
   order that depends on N alone, so they are the same bits for a repeated call, for any max_points (rows per launch, 0 = the library's
   choice), and with or without terms_out / ok_out; value_out is the same bits with and without want_grad. */
int mogp_local_vecchia_loglik(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, double jitter, int k,
                              int want_grad, int max_points, double* value_out, double* grad_out, double* terms_out, int* ok_out);
/* ---- exact prediction for large designs on the same handle: matrix-free preconditioned conjugate gradients (mogp_emulator_amd/IterativeGP.py) ----
   A = sigma2 k(X, X) + nugget I over the WHOLE design is never stored: its entries are generated from the scaled design (x~ = x_d * s_d, r2 by
   fused multiply-adds over d) as they are multiplied.  kernel_type and scale as above.  No atomics anywhere: every output is the same bits
   for a repeated call, and column c of a result depends on column c of the right-hand sides alone.
   mogp_local_kmatvec: out (M, r) = A V with queries == NULL (M = N), else sigma2 k(queries (m, D), X) V (M = m, no nugget); V (N, r), r >= 1. */
int mogp_local_kmatvec(mogp_local* h, int kernel_type, const double* scale, double sigma2, double nugget, const double* queries, int m, int D,
                       const double* V, int r, double* out);
/* Builds and keeps the preconditioner P = L L^T + nugget I: L the partial pivoted Cholesky factor of sigma2 k(X, X) of rank
   0 <= rank <= min(N, 1024) (0: none, plain conjugate gradients); nugget > 0.  Every step takes the largest remaining diagonal entry, ties to
   the lowest index, and the factorisation stops early when that entry is <= 0: rank_out (1) = the rank reached.  pivots_out (rank) and
   L_out (N, rank) or NULL; entries / columns behind the rank reached are zero. */
int mogp_local_precondition(mogp_local* h, int kernel_type, const double* scale, double sigma2, double nugget, int rank, int* rank_out,
                            int* pivots_out, double* L_out);
/* Solves A x = b for the c columns of B (N, c) at the hyperparameters of the last mogp_local_precondition, in blocks of 32 columns that
   share each product with A.  Column j stops as soon as its recurrence residual satisfies |r_j| <= rtol |b_j| (a zero column at iteration 0
   with x = 0), or when p^T A p is not a positive finite number (converged_out 0), and is never touched again: its result does not depend
   on the other columns.  0 < rtol < 1, max_iter >= 1.  iterations_out (c), converged_out (c): the criterion was met within max_iter;
   residual_out (c) = |b - A x| / |b| from one further product with the returned x, as it is.  A column that did not converge is no error. */
int mogp_local_solve(mogp_local* h, const double* B, int c, double rtol, int max_iter, double* x_out, int* iterations_out, int* converged_out,
                     double* residual_out);
/* Exact prediction of residual row `emulator`: alpha = A^-1 y (solved once and kept per emulator while the hyperparameters, rank, rtol and
   max_iter stay), mean_out (m) = sigma2 k(testing, X) alpha and, with var_out != NULL, var_out (m) = max(sigma2 - k*^T A^-1 k* +
   (include_nugget ? nugget : 0), 0) from solves with blocks of 32 cross columns.  The preconditioner of these hyperparameters is built when
   it is not the one held.  stat_out (2) = iterations, converged and residual_out (1) of the alpha solve; var_stat_out (2 m) = iterations,
   converged per query and var_residual_out (m) (needed with var_out); alpha_out (N) or NULL.  m = 0: alpha and its figures alone.
   max_points: queries per device pass, 0 = sized by the free device memory; no result bit depends on it. */
int mogp_local_predict_exact(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, int rank, double rtol,
                             int max_iter, int include_nugget, const double* testing, int m, int D, int max_points, double* mean_out,
                             double* var_out, int* stat_out, double* residual_out, int* var_stat_out, double* var_residual_out,
                             double* alpha_out);
/* The pieces of the EXACT log-likelihood of residual row `emulator` and of its gradient, by one preconditioned CG solve and stochastic
   Lanczos quadrature (mogp_emulator_amd/IterativeGP.py log_likelihood assembles them):
     log p(y) = -1/2 y^T alpha - 1/2 log|A| - N/2 log 2 pi,   log|A| = log|G| + (N - r) log nugget + tr log(P^-1/2 A P^-1/2)
   with P = L L^T + nugget I the preconditioner of mogp_local_precondition, r the rank it reaches and G = nugget I + L^T L.  The probes are
   z_t = L g1_t + sqrt(nugget) g2_t for t < n_probes (1 .. 31): g1 (g1_rows, n_probes) with g1_rows = r -- call mogp_local_precondition
   first to learn it; another value is refused -- and g2 (N, n_probes), row-major standard normals of the caller.  At rank 0 the solver's
   preconditioner is the identity: then P = I, z_t = g2_t, log|G| = 0 and the term (N - r) log nugget is absent.  One solve of the panel
   [y | z_1 .. z_T] (C = 1 + n_probes columns) as mogp_local_solve runs it gives alpha (kept as mogp_local_predict_exact keeps it),
   u_t = A^-1 z_t, w_t = P^-1 z_t (the first preconditioned residual) and the step coefficients.
     scalars_out (4)      y^T alpha, alpha^T alpha, log|G|, r
     stat_out (2 C)       iterations, converged per column; residual_out (C) as mogp_local_solve reports it
     rho_out, uw_out (n_probes)   z_t^T w_t and u_t^T w_t
     coef_out (max_iter, 2, C)    the CG coefficients alpha_j, beta_j of column c at iteration j while the column was live, 0 elsewhere: the
                          Lanczos matrix of column c has T_jj = 1 / alpha_j + beta_(j-1) / alpha_(j-1) and T_j,j+1 = sqrt(beta_j) / alpha_j
     forms_out (2 D)      with want_grad != 0: alpha^T (dA/dtheta_d) alpha for d < D, then sum_t u_t^T (dA/dtheta_d) w_t, where
                          dA_ij/dtheta_d = sigma2 k'(r2_ij) (x~_id - x~_jd)^2, theta_d = log s_d^2 (one entry per dimension whatever the
                          kernel), from ONE sweep over the generated matrix; forms_each_out (n_probes, D) or NULL: the second group per
                          probe, from one sweep each
     z_out (N, n_probes), x_out (N, C), w_out (N, C) or NULL: the probes, the solutions [alpha | u_t] and the panel [alpha | w_t]
   No atomics: the same bits for a repeated call; the first D entries of forms_out do not depend on the probes. */
int mogp_local_loglik_exact(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, int rank, double rtol,
                            int max_iter, const double* g1, int g1_rows, const double* g2, int n_probes, int want_grad, double* scalars_out,
                            int* stat_out, double* residual_out, double* rho_out, double* uw_out, double* coef_out, double* forms_out,
                            double* forms_each_out, double* z_out, double* x_out, double* w_out);
/* A conservative bound of the predictive variance at the price of one rectangular product per batch of queries, with no solve:
     var_out (m) = max(sigma2 + (include_nugget ? nugget : 0) - |R^T k*|^2, 0) >= the exact predictive variance,
   R (N, r) with span R = span L (L the factor of mogp_local_precondition at precond_rank >= 1, built when it is not the one held) and
   R^T A R = I: R R^T is the Galerkin inverse of A on that subspace, and Q (Q^T A Q)^-1 Q^T never exceeds A^-1.  The bound tightens as
   the rank grows and is the exact variance at rank N.  R is built once per (hyperparameters, precond_rank) and kept on the handle, from two
   prefix Cholesky factorisations in natural column order (L^T L, stopped where the columns of L become dependent to 1e-10 of the first, then
   Q^T A Q): its rank may lie below the rank the preconditioner reached, and its leading r' columns are the cache of rank r'.
   var_rank_request: 0 for all of them, else 1 .. the rank the preconditioner reached (another value is refused); var_rank_out (1) = the
   columns that entered, min(request, rank of the cache).  R_out (N, precond_rank) row-major or NULL: the cache, zero behind its rank.
   m = 0: the cache alone.  No atomics: the same bits for a repeated call, whatever max_points (queries per pass, 0 = sized by the free
   device memory) and whatever the other queries; for r1 < r2 the bound at r2 never exceeds the bound at r1. */
int mogp_local_variance_bound(mogp_local* h, int kernel_type, const double* scale, double sigma2, double nugget, int precond_rank,
                              int var_rank_request, int include_nugget, const double* testing, int m, int D, int max_points, double* var_out,
                              int* var_rank_out, double* R_out);
/* Pathwise posterior draws (Matheron's rule with a random-Fourier-feature prior; Wilson et al. 2020): a draw is the function
     f_s(.) = g_s(.) + sigma2 k(., X) v_s,   g_s(x) = amp sum_f W[s][f] cos(phase[f] + omega[f] . (x * scale)),   v_s = A^-1 (y - g_s(X) - sqrt(nugget) eps_s).
   Matrices of draws are (S, .) row-major.
   mogp_local_rff: out (S, M) = g at the design's rows (queries NULL, M = N) or at queries (m, D); omega (F, D) in scaled coordinates, phase (F),
   W (S, F), 1 <= F <= 65536.  The feature matrix is generated and never stored: one cosine per lane as the A operand of the fp64 MFMA, the
   features summed in one fixed ascending order, amp applied once at the end.  No atomics: entry (s, i) is the same bits for a repeated
   call, whatever the other draws, the other points and max_points (points per pass, 0 = sized by the free device memory). */
int mogp_local_rff(mogp_local* h, const double* scale, const double* queries, int m, int D, const double* omega, const double* phase, int n_features,
                   const double* W, int n_draws, double amp, int max_points, double* out);
/* mogp_local_sample_paths: the updates v_s of n_draws paths of residual row `emulator`: the preconditioner of mogp_local_precondition at
   precond_rank (built when it is not the one held), the right-hand sides formed on the device, the solver of mogp_local_solve in blocks of 32
   columns.  W_in (S, F) / noise_in (S, N) or NULL: then the standard normals of draw first_draw + s of the streams stream + 3 / stream + 4
   of the generator of mogp_*_sample_posterior under `seed`, generated on the device.  W_out (S, F): the weights' normals used; v_out (S, N);
   stat_out (2 S) iterations and converged per draw; residual_out (S) = |b - A v| / |b| recomputed; rank_out (1) the rank the preconditioner
   reached.  A draw that does not converge within max_iter is returned as it is with converged 0.  Draw s depends on (seed, stream,
   first_draw + s) and the features alone: no bit of it depends on the other draws of the call. */
int mogp_local_sample_paths(mogp_local* h, int emulator, int kernel_type, const double* scale, double sigma2, double nugget, int precond_rank,
                            double rtol, int max_iter, const double* omega, const double* phase, int n_features, int n_draws, double amp,
                            unsigned long long seed, unsigned stream, int first_draw, const double* W_in, const double* noise_in, double* W_out,
                            double* v_out, int* stat_out, double* residual_out, int* rank_out);
/* Input derivatives at large designs, with respect to the RAW coordinates of the queries (x~ = x * scale, r2_ij = sum_d (q~_id - x~_jd)^2):
     mogp_local_kmatvec_inputderiv: out (m, D, r) row-major,
       out[i][d][c] = d/dx_d [sigma2 k(q_i, X) V]_c = 2 s_d sum_j sigma2 k'(r2_ij) (q~_id - x~_jd) V_jc,   k' = dk/dr2,
     for queries (m, D) and V (N, r), r >= 1; there is no nugget term.  With V = alpha of mogp_local_predict_exact it is the derivative of the
     exact mean, with V = v_s of mogp_local_sample_paths that of a path's update.
     mogp_local_rff_inputderiv: out (S, m, D) row-major, the derivative of the entry (s, i) of mogp_local_rff at queries (m, D),
       out[s][i][d] = -amp s_d sum_f W[s][f] omega[f][d] sin(phase[f] + omega[f] . q~_i).
   Neither matrix is stored: a lane generates sigma2 k'(r2) -- or the sine of the argument mogp_local_rff builds, by the same operations in
   the same order -- once per entry and feeds it to the fp64 MFMAs of a group of 8 dimensions, as k' times the DIFFERENCE q~_id - x~_jd (one
   rounded subtraction: the form does not cancel on designs away from the origin) against the rows of V, or as the sine against the
   rounded products omega_fd W_sf.  2 s_d and -amp s_d multiply once, at the end.  No atomics, and the summed index is not split: entry
   (i, d, c) is the same bits for a repeated call, whatever the other queries, the other columns of V (rows of W) and max_points (queries
   per pass, 0 = sized by the free device memory); a bit does depend on N, D, the kernel and the hyperparameters, nothing else.  A query
   that coincides with a design point gets an exact zero from that point (k' is finite at r2 = 0 for both kernels). */
int mogp_local_kmatvec_inputderiv(mogp_local* h, int kernel_type, const double* scale, double sigma2, const double* queries, int m, int D,
                                  const double* V, int r, int max_points, double* out);
int mogp_local_rff_inputderiv(mogp_local* h, const double* scale, const double* queries, int m, int D, const double* omega, const double* phase,
                              int n_features, const double* W, int n_draws, double amp, int max_points, double* out);
void mogp_local_destroy(mogp_local* h);
/* device memory helpers so a host program can hand device-resident buffers to the *_dev calls */
void* mogp_dev_malloc(unsigned long long bytes);
int mogp_dev_free(void* d_ptr);
int mogp_dev_upload(void* d_dst, const void* src, unsigned long long bytes);
int mogp_dev_download(void* dst, const void* d_src, unsigned long long bytes);
int mogp_dev_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif /* MOGP_HIP_H */
