"""
Exact GP prediction for designs far beyond what one dense factorisation holds: conjugate gradients on the covariance matrix of the WHOLE
design, matrix-free and preconditioned (Gardner et al. 2018; Wang et al. 2019).

    s_d = sqrt(exp(theta_d))                              (one shared value for the uniform kernels)
    A = sigma^2 k(r2(x_i s, x_j s)) + nugget I            N x N, never stored: its entries are generated as they are multiplied
    alpha = A^-1 (y - m(X))                               preconditioned CG, P = L L^T + nugget I, L a rank-p pivoted Cholesky factor
    mean = m(q) + k*^T alpha,    unc = max(sigma^2 - k*^T A^-1 k* + nugget, 0)
    bound = max(sigma^2 - |R^T k*|^2 + nugget, 0) >= unc  R (N, r), span R = span L, R^T A R = I: no solve, one product with the generated k*

``LocalGP`` answers from at most 126 neighbours of a query; this class gives what the dense ``predict`` would give at the same
hyperparameters -- the posterior of all N points -- at the price of one product with A (N^2 generated entries) per iteration.  The
hyperparameters come from a fitted ``GaussianProcessGPU`` / ``MultiOutputGP_GPU`` (typically fitted on a subsample) or from
``VecchiaGP.fit`` (``VecchiaGP.predict_exact``).  The design and the mean-subtracted targets go up once (``csrc/kernels_iter.hip``,
``csrc/engine_iter.hip``; the native handle is ``LocalGP``'s).

Every column of a solve is its own problem: it stops as soon as ITS recurrence residual satisfies |r| <= rtol |b| and is never touched again,
so a result depends neither on the columns it shares a block with nor on ``max_points``; nothing uses atomics, a repeated call returns the
same bits.  What is reported as ``residual`` is |b - A x| / |b| recomputed with one further product, as it is: a column that did not
converge within ``max_iter`` is not an error, it comes back with ``converged`` False and its honest residual.

The exact log-likelihood at those hyperparameters and its gradient come from ONE such solve (``log_likelihood``; ``VecchiaGP.loglik_exact`` and
``VecchiaGP.fit_exact`` evaluate and maximise it at any theta): the panel [y | z_1 .. z_T] with probes z_t = L g1_t + sqrt(nugget) g2_t ~ N(0, P),

    log p(y) = -1/2 y^T alpha - 1/2 log|A| - N/2 log 2 pi,        log|A| = log|P| + tr log(P^-1/2 A P^-1/2)
    tr log(.) ~ 1/T sum_t rho_t e_1^T log(T_t) e_1                rho_t = z_t^T P^-1 z_t, T_t the Lanczos matrix of column t's CG coefficients
    d/dtheta_q = 1/2 alpha^T dA_q alpha - 1/2 tr(A^-1 dA_q),      tr(A^-1 dA_q) ~ 1/T sum_t (A^-1 z_t)^T dA_q (P^-1 z_t)      (E[z z^T] = P)

(stochastic Lanczos quadrature in its CG form).  The forms with the length-scale derivatives are one further sweep over the generated matrix
for all probes together; those of log sigma^2 (dA = A - nugget I) and log nugget (dA = nugget I) are dots.  With ``precond_rank=0`` the
solver's preconditioner is the identity: P = I and z_t = g2_t.  The estimate is a deterministic function of (theta, probes).

An exact variance is one solve per query.  ``variance_bound`` (``predict(unc="bound")``) gives, at the price of the mean, a variance that is
never below the exact one: for any full-column-rank Q the Galerkin inverse Q (Q^T A Q)^-1 Q^T never exceeds A^-1, and with span Q = span L
-- the factor the handle holds already -- it is R R^T for a cache R that is built once per (hyperparameters, rank): G0 = L^T L,
a prefix Cholesky of it in natural column order (stopped where L's columns become dependent), Q = L C0^-T, H = Q^T A Q by ``rank / 32``
products with A, a prefix Cholesky of H, R = Q C^-T.  Both factors are prefixes, so the leading r columns of R are the cache of rank r:
the bound tightens monotonically with the rank, bit for bit, and is the exact variance at rank N.  How far it lies above the exact variance
depends on the design, the kernel and the rank; ``variance_gap`` measures it on the caller's own queries.

Joint draws of the posterior at these sizes are functions (``sample_paths``, ``PosteriorPaths``): pathwise conditioning, that is Matheron's rule
on a random-Fourier-feature prior (Wilson et al. 2020),

    f_s(.) = m(.) + g_s(.) + sigma^2 k(., X) v_s,    v_s = A^-1 (y - m(X) - g_s(X) - sqrt(nugget) eps_s)
    g_s(x) = sqrt(2 sigma^2 / F) sum_f W_sf cos(omega_f . (x * s) + b_f)

with the v_s as further columns of the solver, the feature matrix generated and never stored (``csrc/kernels_rff.hip``) and every random
input a named Philox sub-stream, so that a path is a deterministic function of (seed, stream, emulator, draw index, n_features).

Input derivatives come from one further sweep over the same generated matrices (``csrc/kernels_iter.hip`` kinderiv_kernel,
``csrc/kernels_rff.hip`` rff_inderiv_kernel), with respect to the RAW coordinates of a query:

    G_c(x)_d = d/dx_d [sigma^2 k(x, X) V]_c = 2 s_d sum_j sigma^2 k'(r2_j) (x~_d - x~_jd) V_jc      ``matvec_inputderiv``; k' = dk/dr2, no nugget term
    d mean / dx_d = dm/dx_d + G(x)_d at V = alpha                                                   ``predict(deriv=True)``
    d g_s / dx_d  = -sqrt(2 sigma^2 / F) s_d sum_f W_sf omega_fd sin(omega_f . x~ + b_f)            ``PosteriorPaths.prior_gradient`` (with dm/dx_d)
    d f_s / dx_d  = dm/dx_d + d g_s / dx_d + G_s(x)_d at V = v                                      ``PosteriorPaths.gradient``

The entry is k' times the DIFFERENCE of the scaled coordinates: the expanded form x~_d sum g V - sum g x~_jd V cancels on designs away
from the origin.

Not covered: joint draws of paths over hyperparameters, second derivatives and derivatives of the variance, bounds of
cross-covariances, a lower bound, more than 31 probes per evaluation (average over seeds), derivatives with respect to mean-function
parameters, the symmetry of A in the product, several devices per handle, ``ProductMat52``, ``analytic_mean=True``, ``nugget="pivot"``.
"""
import numpy as np

from .LocalGP import MAX_D, _KERNELS, _create_native, _emulator_type, _fit_state, _hyperparameters, _mean_at, _points


def _mean_inputderiv_at(meanfunc, params, x):
    """(m, D) d m(x) / d x of the fixed mean function; exact zeros for the zero mean"""
    if meanfunc is None or (meanfunc.get_n_params() == 0 and type(meanfunc).__name__ == "ZeroMeanFunc"):
        return np.zeros(x.shape)
    return np.ascontiguousarray(np.asarray(meanfunc.mean_inputderiv(x, params), dtype=np.float64).reshape(x.shape[1], x.shape[0]).T)

MAX_RANK = 1024
MAX_FEATURES = 65536     # random Fourier features of a path (csrc/predict_plan.h RFF_MAX_FEATURES)
MAX_PROBES = 31          # the data column and the probes share one panel of 32 columns
_PROBE_STREAM = 0x10c    # the Philox stream of the default probes (g1 from it, g2 from the next)
VAR_CHUNK = 64           # columns of the variance cache per workgroup of the bound's kernel (csrc/predict_plan.h ITER_VAR_CHUNK)
_NEEDS_FACTOR = "%s: the variance bound is built from the preconditioner's factor: precond_rank must be at least 1"


class IterativeSolve(object):
    """What ``IterativeGP.solve`` returns: ``x`` (N, c) (or (N,) for a vector), per column ``iterations``, ``residual`` = |b - A x| / |b|
    recomputed from x, ``converged`` (the recurrence residual met ``rtol`` within ``max_iter``), and ``precond_rank``, the rank the
    preconditioner reached."""

    def __init__(self, x, iterations, residual, converged, precond_rank):
        self.x, self.iterations, self.residual, self.converged, self.precond_rank = x, iterations, residual, converged, precond_rank


class IterativePrediction(object):
    """What ``IterativeGP.predict`` returns (shapes (m,) for a ``GaussianProcessGPU``, (E, m) for a ``MultiOutputGP_GPU``):

    * ``mean``, ``unc``                 predictive mean and variance; ``unc`` is None with ``unc=False``
    * ``converged``, ``residual``, ``iterations``   of the solve for the weights alpha (scalars, or (E,))
    * ``var_converged``, ``var_residual``           per query, of the solve behind its variance; None with ``unc=False`` and ``unc="bound"``
    * ``unc_kind``                      None, "exact" or "bound": what ``unc`` holds
    * ``var_rank``                      with ``unc="bound"``: the columns of the variance cache that entered (a scalar, or (E,)); else None
    * ``deriv``                         with ``deriv=True``: d mean / d x, (m, D) or (E, m, D), as the dense ``predict`` lays it out; else None"""

    def __init__(self, mean, unc, converged, residual, iterations, var_converged, var_residual, var_rank=None, unc_kind=None, deriv=None):
        self.mean, self.unc, self.converged, self.residual, self.iterations = mean, unc, converged, residual, iterations
        self.deriv = deriv
        self.var_converged, self.var_residual = var_converged, var_residual
        self.var_rank, self.unc_kind = var_rank, ("exact" if unc is not None else None) if unc_kind is None else unc_kind


class ExactLogLik(object):
    """What ``IterativeGP.log_likelihood`` and ``VecchiaGP.loglik_exact`` return:

    * ``value``           -fit_term / 2 - logdet / 2 - N log(2 pi) / 2; NaN when ``ok`` is False
    * ``grad``            (P,) in ``VecchiaLogLik.grad``'s layout -- the correlation parameters (D, or 1 for the uniform kernels), log sigma^2,
                          and log nugget when the nugget is fitted -- with ``grad=True``, else None
    * ``fit_term``        y^T alpha;   ``logdet`` the estimate of log|A|;   ``logdet_precond`` log|P|, its exact part
    * ``logdet_se``       the standard error of ``logdet`` over the probes (NaN with one probe)
    * ``trace``, ``trace_se``   (P,) the estimates of tr(A^-1 dA/dtheta_q) and their standard errors; the length-scale entries of
                          ``trace_se`` are NaN unless ``probe_terms=True``.  None without ``grad``
    * ``data_forms``      (P,) alpha^T (dA/dtheta_q) alpha, None without ``grad``
    * ``rho``, ``uw``     (T,) z_t^T P^-1 z_t and (A^-1 z_t)^T (P^-1 z_t) as the device returned them; ``quadrature`` (T,) rho_t e_1^T log(T_t) e_1
    * ``iterations``, ``converged``, ``residual``   per column of the solve, the data column first
    * ``precond_rank``    the rank the preconditioner reached
    * ``ok``              every column converged and every quadrature was finite"""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def _lanczos_quadrature(a, b):
    """e_1^T log(T) e_1 of the Lanczos matrix of one column's CG coefficients a_0 .. a_(m-1), b_0 .. b_(m-2)"""
    from scipy.linalg import eigh_tridiagonal
    m = a.shape[0]
    if m < 1 or not (np.all(np.isfinite(a)) and np.all(a > 0.) and np.all(np.isfinite(b[:m - 1])) and np.all(b[:m - 1] >= 0.)):
        return np.nan
    diag = 1. / a
    diag[1:] += b[:m - 1] / a[:m - 1]
    if m == 1:
        return float(np.log(diag[0])) if diag[0] > 0. else np.nan
    lam, vec = eigh_tridiagonal(diag, np.sqrt(b[:m - 1]) / a[:m - 1], lapack_driver="stev")      # (QR: the default MRRR driver can fail on these)
    if not np.all(lam > 0.):
        return np.nan
    return float(np.sum(vec[0] ** 2 * np.log(lam)))


def _check_probes(who, n_probes, seed, probes, N):
    """(T, seed, g2 or None, g1 or None) -- g1's row count is checked once the rank is known"""
    if probes is None:
        T = int(n_probes)
        if T != n_probes or T < 1 or T > MAX_PROBES:
            raise ValueError("%s: n_probes must be between 1 and %d" % (who, MAX_PROBES))
        if int(seed) != seed or int(seed) < 0:
            raise ValueError("%s: seed must be a non-negative integer" % who)
        return T, int(seed), None, None
    try:
        g1, g2 = probes
        g1, g2 = np.ascontiguousarray(g1, dtype=np.float64), np.ascontiguousarray(g2, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: probes must be a pair (g1 (rank reached, T), g2 (N, T)) of arrays" % who)
    if g2.ndim != 2 or g1.ndim != 2 or g2.shape[0] != N or g1.shape[1] != g2.shape[1]:
        raise ValueError("%s: probes must be a pair (g1 (rank reached, T), g2 (N, T)) of arrays with N = %d" % (who, N))
    if g2.shape[1] < 1 or g2.shape[1] > MAX_PROBES:
        raise ValueError("%s: n_probes must be between 1 and %d" % (who, MAX_PROBES))
    if not (np.all(np.isfinite(g1)) and np.all(np.isfinite(g2))):
        raise ValueError("%s: probes must be finite" % who)
    return g2.shape[1], 0, g2, g1


def _exact_loglik(who, native, e, hyper, layout, D, N, p, rtol, max_iter, grad, T, seed, g1, g2, probe_terms):
    """the device call and the assembly of an ``ExactLogLik``; every argument has been checked"""
    kt, s, sigma2, eta = hyper[:4]
    uniform, fit_nugget = layout
    rank = native.precondition(kt, s, sigma2, eta, p)[0]
    if g2 is None:
        from .Sampling import philox_normals
        g1 = np.ascontiguousarray(philox_normals(seed, _PROBE_STREAM, T, rank).T) if rank else np.zeros((0, T))
        g2 = np.ascontiguousarray(philox_normals(seed, _PROBE_STREAM + 1, T, N).T)
    elif g1.shape[0] != rank:
        raise ValueError("%s: g1 of probes must have as many rows as the rank the preconditioner reaches, %d" % (who, rank))
    r = native.loglik_exact(e, kt, s, sigma2, eta, p, rtol, max_iter, g1, g2, grad=grad, probe_terms=probe_terms)
    rho, uw, its = r["rho"], r["uw"], r["iterations"]
    quad = np.array([rho[t] * _lanczos_quadrature(r["coef"][:its[1 + t], 0, 1 + t], r["coef"][:its[1 + t], 1, 1 + t]) for t in range(T)])
    ok = bool(r["converged"].all() and np.all(np.isfinite(quad)) and np.isfinite(r["y_alpha"]))
    root = np.sqrt(T)
    se = (lambda v: float(np.std(v, ddof=1)) / root) if T > 1 else (lambda v: np.nan)
    logdet_p = r["logdet_g"] + (N - rank) * np.log(eta) if rank else 0.
    logdet = logdet_p + float(np.mean(quad))
    value = -0.5 * r["y_alpha"] - 0.5 * logdet - 0.5 * N * np.log(2. * np.pi) if ok else np.nan
    out_g = trace = trace_se = data = None
    if grad:
        def corr(v):                              # (.., D) per dimension -> the layout of theta: the uniform kernels share one parameter
            if not uniform:
                return v
            tot = 0. * v[..., 0]
            for d in range(D):                    # ascending in d
                tot = tot + v[..., d]
            return tot[..., None]
        tr_eta, tr_s2 = eta * np.mean(uw), np.mean(rho) - eta * np.mean(uw)
        trace = np.concatenate([corr(r["forms_probe"]) / T, [tr_s2], [tr_eta] if fit_nugget else []])
        each = corr(r["forms_each"]) if probe_terms else None
        nc = trace.shape[0] - 1 - (1 if fit_nugget else 0)
        trace_se = np.concatenate([[se(each[:, q]) for q in range(nc)] if probe_terms else np.full(nc, np.nan), [se(rho - eta * uw)],
                                   [se(eta * uw)] if fit_nugget else []])
        data = np.concatenate([corr(r["forms_data"]), [r["y_alpha"] - eta * r["alpha_alpha"]], [eta * r["alpha_alpha"]] if fit_nugget else []])
        out_g = 0.5 * data - 0.5 * trace if ok else np.full(trace.shape[0], np.nan)
    return ExactLogLik(value=float(value), grad=out_g, fit_term=r["y_alpha"], logdet=logdet if ok else np.nan, logdet_precond=float(logdet_p),
                       logdet_se=se(quad), trace=trace, trace_se=trace_se, data_forms=data, rho=rho, uw=uw, quadrature=quad,
                       iterations=its, converged=r["converged"], residual=r["residual"], precond_rank=rank, ok=ok)


def _check_options(who, N, precond_rank, rtol, max_iter):
    p = int(precond_rank)
    if p != precond_rank or p < 0 or p > min(N, MAX_RANK):
        raise ValueError("%s: precond_rank must be between 0 and min(N, %d) = %d" % (who, MAX_RANK, min(N, MAX_RANK)))
    rtol = float(rtol)
    if not (0. < rtol < 1.):
        raise ValueError("%s: rtol must lie between 0 and 1 (both excluded)" % who)
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError("%s: max_iter must be at least 1" % who)
    return p, rtol, int(max_iter)


def path_features(seed, stream, n_features, D, kt):
    """(omega (F, D), phase (F,)) of the random Fourier features of a path, from ``philox_normals`` under the sub-streams ``stream + j``:
    j = 0 (F, D) normals z; j = 1 (F, 5) normals g for the Matern-5/2 kernels (``kt`` 1), omega_f = z_f sqrt(5 / sum_i g_fi^2) -- the
    kernel's multivariate-t spectral measure; omega = z for the squared exponential (``kt`` 0) --; j = 2 (F, 2) normals h,
    phase_f = arctan2(h_f0, h_f1), uniform on (-pi, pi].  In the scaled coordinates x * s of the handle."""
    from .Sampling import philox_normals
    F = int(n_features)
    omega = philox_normals(seed, stream, F, D)
    if kt == 1:
        g = philox_normals(seed, stream + 1, F, 5)
        chi = np.zeros(F)
        for i in range(5):                        # ascending in i
            chi = chi + g[:, i] * g[:, i]
        omega = omega * np.sqrt(5. / chi)[:, None]
    h = philox_normals(seed, stream + 2, F, 2)
    return np.ascontiguousarray(omega), np.ascontiguousarray(np.arctan2(h[:, 0], h[:, 1]))


class PosteriorPaths(object):
    """What ``IterativeGP.sample_paths`` returns: ``n_draws`` functions drawn from the posterior of one emulator,

        f_s(x) = m(x) + g_s(x) + sigma^2 k(x, X) update[:, s],      g_s(x) = sqrt(2 sigma^2 / F) sum_f feature_normals[s, f] cos(omega_f . (x * s) + phase_f)

    Each may be evaluated at any query set, any number of times, consistently: ``evaluate(testing)`` (or calling the object) gives
    (n_draws, m) values of the latent f -- no nugget is added --, ``prior(testing)`` m + g_s alone.  Fields: ``n_draws``, ``n_features``,
    ``omega`` (F, D) in scaled coordinates, ``phase`` (F,), ``feature_normals`` (S, F), ``update`` (N, S), per draw ``iterations``,
    ``converged``, ``residual`` (|b - A v| / |b| recomputed) and ``ok`` (converged and finite), ``precond_rank`` (the rank reached),
    ``seed``, ``stream`` (of the emulator: the caller's plus 8 times its index), ``first_draw``, ``emulator``.  The paths hold on to the
    ``IterativeGP`` they came from and refuse by name once it is closed."""

    def __init__(self, gp, hyper, **fields):
        self._gp, self._hyper = gp, hyper
        self.__dict__.update(fields)

    def _native(self, who):
        if self._gp._native is None:
            raise RuntimeError("%s: the handle has been closed" % who)
        return self._gp._native

    def _queries(self, who, testing, max_points):
        testing = _points("testing", who, testing, self._gp._D)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if testing.shape[0] >= 2 ** 31:
            raise ValueError("%s: at most 2^31 - 1 testing points per call" % who)
        return testing, int(max_points), self._native(who)

    def _prior(self, native, testing, max_points):
        kt, s, sigma2, nugget, meanfunc, mparams = self._hyper
        g = native.rff(s, self.omega, self.phase, self.feature_normals, np.sqrt(2. * sigma2 / self.n_features), queries=testing,
                       max_points=max_points)
        return g + _mean_at(meanfunc, mparams, testing)[None, :]

    def prior(self, testing, max_points=0):
        """(n_draws, m) m(x) + g_s(x): the prior draws the paths are conditioned from"""
        testing, max_points, native = self._queries("PosteriorPaths.prior", testing, max_points)
        return self._prior(native, testing, max_points)

    def evaluate(self, testing, max_points=0):
        """(n_draws, m) f_s at ``testing`` (m, D).  ``max_points`` caps the queries per device pass (0: sized by the free device memory) and
        changes no bit; neither do the other queries or a repeated call."""
        testing, max_points, native = self._queries("PosteriorPaths.evaluate", testing, max_points)
        kt, s, sigma2, nugget, _, _ = self._hyper
        out = self._prior(native, testing, max_points)
        step = max_points if max_points else testing.shape[0]
        for c0 in range(0, testing.shape[0], step):
            out[:, c0:c0 + step] += native.kmatvec(kt, s, sigma2, nugget, self.update, queries=testing[c0:c0 + step]).T
        return out

    __call__ = evaluate

    def _prior_gradient(self, native, testing, max_points):
        kt, s, sigma2, nugget, meanfunc, mparams = self._hyper
        g = native.rff_inputderiv(s, self.omega, self.phase, self.feature_normals, np.sqrt(2. * sigma2 / self.n_features), testing,
                                  max_points=max_points)
        return g + _mean_inputderiv_at(meanfunc, mparams, testing)[None, :, :]

    def prior_gradient(self, testing, max_points=0):
        """(n_draws, m, D) d(m + g_s) / dx at ``testing`` (m, D): the input derivative of ``prior``, analytic, from one product with the
        sines of the features (never stored)"""
        testing, max_points, native = self._queries("PosteriorPaths.prior_gradient", testing, max_points)
        return self._prior_gradient(native, testing, max_points)

    def gradient(self, testing, max_points=0):
        """(n_draws, m, D) df_s / dx at ``testing`` (m, D), with respect to the raw coordinates: ``prior_gradient`` plus the derivative of
        sigma^2 k(x, X) ``update``, one sweep over the generated cross covariance for all dimensions and draws.  ``max_points`` caps the
        queries per device pass (0: sized by the free device memory) and changes no bit; neither do the other queries, the other draws or a
        repeated call."""
        testing, max_points, native = self._queries("PosteriorPaths.gradient", testing, max_points)
        kt, s, sigma2, nugget, _, _ = self._hyper
        out = self._prior_gradient(native, testing, max_points)
        out += np.transpose(native.kmatvec_inputderiv(kt, s, sigma2, self.update, testing, max_points=max_points), (2, 0, 1))
        return out

    def value_and_gradient(self, testing, max_points=0):
        """``(evaluate(testing), gradient(testing))``, bit for bit: two sweeps"""
        return self.evaluate(testing, max_points), self.gradient(testing, max_points)


def _check_normals(who, name, z, S, cols, what):
    if z is None:
        return None
    z = np.ascontiguousarray(z, dtype=np.float64)
    if z.shape != (S, cols):
        raise ValueError("%s: %s must have shape (n_draws, %s) = (%d, %d)" % (who, name, what, S, cols))
    if not np.all(np.isfinite(z)):
        raise ValueError("%s: %s must be finite" % (who, name))
    return z


def _check_nuggets(who, hyper):
    for h in hyper:
        if not (h[3] > 0. and np.isfinite(h[3])):
            raise ValueError("%s: the nugget must be positive (the preconditioner divides by it)" % who)


class IterativeGP(object):
    """``IterativeGP(gp, inputs, targets, precond_rank=256, rtol=1e-8, max_iter=1000, device=None)``

    ``gp``: a fitted ``GaussianProcessGPU`` (E = 1) or ``MultiOutputGP_GPU`` (E emulators), the source of the kernel, the hyperparameters and
    the mean function, exactly as ``LocalGP`` takes them; it is never modified.  ``inputs`` (N, D), ``targets`` (N,) or (E, N): the whole
    design.  ``precond_rank`` 0 .. min(N, 1024): the rank of the pivoted Cholesky preconditioner, 0 for plain conjugate gradients (it changes
    the number of iterations, never what a converged answer is judged by).  ``rtol`` in (0, 1) and ``max_iter`` >= 1: every column stops
    at |r| <= rtol |b| or after max_iter iterations.

    Every argument is checked before the device is touched.  ``RuntimeError`` for ``nugget="pivot"``, ``analytic_mean=True``,
    ``ProductMat52`` and an emulator that is not fit; ``ValueError`` for a nugget that is not positive, ``precond_rank``, ``rtol``,
    ``max_iter``, shapes and non-finite values.  The device needs 8 N precond_rank bytes for the factor and about eight N x 32 panels; what
    does not fit half of the free memory is refused by name.  The native handle is freed by ``close()`` (and on deletion)."""

    def __init__(self, gp, inputs, targets, precond_rank=256, rtol=1e-8, max_iter=1000, device=None):
        who = "IterativeGP"
        self._native = None
        single = _emulator_type(who, gp)
        D = int(gp.D)
        if D > MAX_D:
            raise ValueError("%s: at most %d input dimensions" % (who, MAX_D))
        inputs = _points("inputs", who, inputs, D)
        N = inputs.shape[0]
        if N >= 2 ** 31 - 256:
            raise ValueError("%s: the design must have fewer than 2^31 - 256 points" % who)
        natives = _fit_state(who, gp, single)
        E = len(natives)
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        if targets.shape != ((N,) if single else (E, N)) and not (E == 1 and targets.shape in ((N,), (1, N))):
            raise ValueError("%s: targets must have shape %s" % (who, "(N,) with N = %d" % N if single else "(E, N) with E = %d, N = %d" % (E, N)))
        targets = targets.reshape(E, N)
        if not np.all(np.isfinite(targets)):
            raise ValueError("%s: targets must be finite" % who)
        self._p, self._rtol, self._max_iter = _check_options(who, N, precond_rank, rtol, max_iter)
        if device is not None and (int(device) != device or int(device) < 0):
            raise ValueError("%s: device must be a device ordinal or None" % who)
        self._hyper = [_hyperparameters(em, D) for em in natives]
        fit_nugget = (gp.nugget_type if single else gp._nugget_name) == "fit"
        self._layout = [(_KERNELS[str(em.get_kernel_type()).split(".")[1]][1], fit_nugget) for em in natives]
        _check_nuggets(who, self._hyper)
        self._single, self._D, self._N, self._E = single, D, N, E
        resid = np.stack([targets[e] - _mean_at(h[4], h[5], inputs) for e, h in enumerate(self._hyper)])
        self._native = _create_native(inputs, np.ascontiguousarray(resid), None if device is None else int(device))

    @classmethod
    def _on_handle(cls, native, hyper, D, N, precond_rank=256, rtol=1e-8, max_iter=1000, layout=None):
        """Internal: a single-output view on a native handle that somebody else owns (``VecchiaGP.predict_exact``), at the hyperparameters
        ``hyper`` = [(kernel 0 / 1, s (D,), sigma^2, nugget, mean function or None, its parameters)] in place of a fitted ``gp``.
        ``layout`` = [(uniform kernel, fitted nugget)]: what ``log_likelihood`` lays its gradient out by (default: per-dimension, fitted).
        ``close()`` of the view leaves the handle open."""
        who = "IterativeGP"
        self = cls.__new__(cls)
        self._p, self._rtol, self._max_iter = _check_options(who, int(N), precond_rank, rtol, max_iter)
        _check_nuggets(who, hyper)
        self._single, self._D, self._N, self._E = True, int(D), int(N), 1
        self._hyper, self._native, self._borrowed = list(hyper), native, True
        self._layout = list(layout) if layout is not None else [(False, True)] * len(self._hyper)
        return self

    VAR_CHUNK = VAR_CHUNK              # ranks on both sides of a multiple of it take one more workgroup column in ``variance_bound``
    n = property(lambda self: self._N)
    D = property(lambda self: self._D)
    n_emulators = property(lambda self: self._E)
    precond_rank = property(lambda self: self._p)
    rtol = property(lambda self: self._rtol)
    max_iter = property(lambda self: self._max_iter)

    def close(self):
        native, self._native = getattr(self, "_native", None), None
        if native is not None and not getattr(self, "_borrowed", False):
            native.close()

    def __del__(self):
        self.close()

    # ---- checks that need no device --------------------------------------------------------------------------------------------------
    def _emulator(self, who, emulator):
        e = int(emulator)
        if e != emulator or e < 0 or e >= self._E:
            raise ValueError("%s: emulator must be between 0 and %d" % (who, self._E - 1))
        if self._native is None:
            raise RuntimeError("%s: the handle has been closed" % who)
        return e, self._hyper[e]

    def _columns(self, who, name, V):
        V = np.asarray(V, dtype=np.float64)
        vector = V.ndim == 1
        V = np.ascontiguousarray(V.reshape(-1, 1) if vector else V)
        if V.ndim != 2 or V.shape[0] != self._N or V.shape[1] < 1:
            raise ValueError("%s: %s must have shape (N,) or (N, c) with N = %d and at least one column" % (who, name, self._N))
        if not np.all(np.isfinite(V)):
            raise ValueError("%s: %s must be finite" % (who, name))
        return V, vector

    # ---- the operator, the preconditioner, the solver -----------------------------------------------------------------------------------
    def matvec(self, V, emulator=0, testing=None):
        """(sigma^2 k(X, X) + nugget I) V at the hyperparameters of ``emulator``; V (N,) or (N, c).  With ``testing`` (m, D) the rectangular
        product sigma^2 k(testing, X) V (m rows, no nugget).  Column c of the result depends on column c of V alone, bit for bit."""
        who = "IterativeGP.matvec"
        V, vector = self._columns(who, "V", V)
        if testing is not None:
            testing = _points("testing", who, testing, self._D)
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        out = self._native.kmatvec(kt, s, sigma2, nugget, V, queries=testing)
        return out[:, 0] if vector else out

    def matvec_inputderiv(self, V, testing, emulator=0, max_points=0):
        """d/dx [sigma^2 k(testing, X) V] with respect to the raw coordinates of ``testing`` (m, D) at the hyperparameters of ``emulator``:
        (m, D, c) for V (N, c), (m, D) for a vector V (N,); entry (i, d, c) = 2 s_d sum_j sigma^2 k'(r2_ij) (q~_id - x~_jd) V_jc, no nugget
        term.  Column c depends on column c of V alone and row i on query i alone, bit for bit; ``max_points`` caps the queries per device
        pass (0: sized by the free device memory) and changes no bit."""
        who = "IterativeGP.matvec_inputderiv"
        V, vector = self._columns(who, "V", V)
        testing = _points("testing", who, testing, self._D)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if testing.shape[0] >= 2 ** 31:
            raise ValueError("%s: at most 2^31 - 1 testing points per call" % who)
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        out = self._native.kmatvec_inputderiv(kt, s, sigma2, V, testing, max_points=int(max_points))
        return out[:, :, 0] if vector else out

    def preconditioner(self, emulator=0):
        """(L (N, rank reached), pivots (rank reached,) int64) of the partial pivoted Cholesky factor the solves of ``emulator`` are
        preconditioned with; the rank reached is below ``precond_rank`` when the remaining diagonal ran out."""
        who = "IterativeGP.preconditioner"
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        r, piv, L = self._native.precondition(kt, s, sigma2, nugget, self._p, return_factor=True)
        return L, piv

    def solve(self, B, emulator=0):
        """A^-1 B column by column; B (N,) or (N, c).  Returns an ``IterativeSolve``; ``solve(B).x[:, j]`` equals ``solve(B[:, [j]]).x[:, 0]``
        bit for bit, ``iterations`` included."""
        who = "IterativeGP.solve"
        B, vector = self._columns(who, "B", B)
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        rank = self._native.precondition(kt, s, sigma2, nugget, self._p)[0]
        x, it, cv, res = self._native.solve(B, self._rtol, self._max_iter)
        return IterativeSolve(x[:, 0] if vector else x, it, res, cv, rank)

    def weights(self, emulator=0):
        """alpha = A^-1 (y - m(X)) of ``emulator`` (N,), as ``predict`` uses it (solved once and kept on the handle)"""
        who = "IterativeGP.weights"
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        return self._native.predict_exact(e, kt, s, sigma2, nugget, self._p, self._rtol, self._max_iter, True, None, return_alpha=True)[4]

    # ---- the exact likelihood ---------------------------------------------------------------------------------------------------------------
    def log_likelihood(self, emulator=0, grad=False, n_probes=15, seed=0, probes=None, probe_terms=False):
        """The exact log-likelihood of the whole design at the hyperparameters of ``emulator`` (its log-determinant estimated by stochastic
        Lanczos quadrature) and, with ``grad=True``, its gradient; returns an ``ExactLogLik``.  The mean function is held fixed.

        ``n_probes`` 1 .. 31 (the default 15 makes 16 columns with the data: the product then runs on one block of 16); the normals come
        from ``philox_normals(seed, .)`` of ``Sampling.py`` unless ``probes=(g1 (rank reached, T), g2 (N, T))`` gives the caller's (common
        random numbers; ``preconditioner()`` tells the rank).  ``probe_terms=True`` also gives the length-scale traces a standard error,
        by one sweep per probe: T times the cost of the sweep.  A column that does not converge is reported (``ok`` False, ``value``
        NaN), never raised.  The weights of the solve are kept as ``weights()`` / ``predict`` keep them."""
        who = "IterativeGP.log_likelihood"
        T, seed, g2, g1 = _check_probes(who, n_probes, seed, probes, self._N)
        e, hyper = self._emulator(who, emulator)
        return _exact_loglik(who, self._native, e, hyper, self._layout[e], self._D, self._N, self._p, self._rtol, self._max_iter, bool(grad),
                             T, seed, g1, g2, bool(probe_terms) and bool(grad))

    # ---- pathwise posterior draws ------------------------------------------------------------------------------------------------------------
    def sample_paths(self, n_draws=1, emulator=0, n_features=2048, seed=0, stream=0x200, first_draw=0, feature_normals=None, noise_normals=None):
        """``n_draws`` functions from the posterior of ``emulator`` by pathwise conditioning (Matheron's rule on a random-Fourier-feature
        prior; Wilson et al. 2020); returns a ``PosteriorPaths``.  Conditional on the features the draws are Gaussian with the exact data
        term and a prior covariance that is off by O(sigma^2 / sqrt(n_features)).

        The random inputs are ``philox_normals(seed, stream + 8 emulator + j, ...)`` of ``Sampling.py``: j = 0, 1, 2 the frequencies and
        phases (``path_features``), j = 3 the (n_draws, n_features) weights' normals and j = 4 the (n_draws, N) noise normals, both at
        draw rows ``first_draw + s`` and generated on the device unless ``feature_normals`` / ``noise_normals`` give the caller's (common
        random numbers, antithetic pairs, exact tests; on a view of a ``VecchiaGP`` the columns of ``noise_normals`` are in the handle's
        order).  A path depends on (seed, stream, emulator, draw index, n_features) alone: ``sample_paths(4)`` equals ``sample_paths(2)``
        followed by ``sample_paths(2, first_draw=2)`` bit for bit, and a repeated call returns the same bits.  The updates are ``n_draws``
        further columns of the solver of ``solve`` (``precond_rank``, ``rtol``, ``max_iter`` of this object); a draw whose solve did not
        converge comes back with ``converged`` False, nothing is raised.  Every argument is checked before the device is touched."""
        who = "IterativeGP.sample_paths"
        S = int(n_draws)
        if S != n_draws or S < 1:
            raise ValueError("%s: n_draws must be at least 1" % who)
        F = int(n_features)
        if F != n_features or F < 1 or F > MAX_FEATURES:
            raise ValueError("%s: n_features must be between 1 and %d" % (who, MAX_FEATURES))
        if int(first_draw) != first_draw or int(first_draw) < 0 or int(first_draw) + S >= 2 ** 31:
            raise ValueError("%s: first_draw must not be negative (and first_draw + n_draws below 2^31)" % who)
        if int(seed) != seed or int(seed) < 0 or int(seed) >= 2 ** 64:
            raise ValueError("%s: seed must be an integer in [0, 2^64)" % who)
        if int(stream) != stream or int(stream) < 0 or int(stream) + 8 * self._E >= 2 ** 32:
            raise ValueError("%s: stream must be an integer in [0, 2^32 - 8 n_emulators)" % who)
        W = _check_normals(who, "feature_normals", feature_normals, S, F, "n_features")
        eps = _check_normals(who, "noise_normals", noise_normals, S, self._N, "N")
        e, hyper = self._emulator(who, emulator)
        kt, s, sigma2, nugget, _, _ = hyper
        sub = int(stream) + 8 * e
        omega, phase = path_features(int(seed), sub, F, self._D, kt)
        W, v, it, cv, res, rank = self._native.sample_paths(e, kt, s, sigma2, nugget, self._p, self._rtol, self._max_iter, omega, phase, S,
                                                            np.sqrt(2. * sigma2 / F), int(seed), sub, int(first_draw), W, eps)
        update = np.ascontiguousarray(v.T)
        return PosteriorPaths(self, hyper, n_draws=S, n_features=F, omega=omega, phase=phase, feature_normals=W, update=update, iterations=it,
                              converged=cv, residual=res, ok=cv & np.all(np.isfinite(update), axis=0), precond_rank=rank, seed=int(seed),
                              stream=sub, first_draw=int(first_draw), emulator=e)

    # ---- prediction ----------------------------------------------------------------------------------------------------------------------
    def predict(self, testing, unc=False, include_nugget=True, max_points=0, deriv=False):
        """Predict at ``testing`` (m, D) from the whole design; returns an ``IterativePrediction``.

        ``unc=True`` solves one system per query (in blocks of 32): exact, and as expensive as that sounds.  ``unc="bound"`` puts
        ``variance_bound(testing)`` there instead, bit for bit -- never below the exact variance, no solve; ``var_converged`` and
        ``var_residual`` are then None, ``var_rank`` tells the columns of the cache and ``unc_kind`` is "bound".  Any other string is a
        ``ValueError``.  The mean is the same bits whatever ``unc``.  ``include_nugget``: add the
        nugget to ``unc`` as ``predict`` of the emulator does.  ``max_points`` caps the queries per device pass (0: sized by the free device
        memory) and changes no bit of the result.  Emulator e of a ``MultiOutputGP_GPU`` uses its own hyperparameters and its own
        preconditioner; the emulators run one after another on the same handle, and row e equals the single-emulator call bit for bit.
        ``deriv=True``: ``deriv`` (m, D), or (E, m, D), the derivative of the mean with respect to the inputs as the dense ``predict``
        returns it -- the mean function's plus ``matvec_inputderiv`` at the kept weights --; every other field keeps its bits."""
        who = "IterativeGP.predict"
        if isinstance(unc, str):
            if unc != "bound":
                raise ValueError('%s: unc must be False, True or "bound"' % who)
            if self._p == 0:
                raise ValueError(_NEEDS_FACTOR % who)
        bound = isinstance(unc, str)
        exact = bool(unc) and not bound
        testing = _points("testing", who, testing, self._D)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if testing.shape[0] >= 2 ** 31:
            raise ValueError("%s: at most 2^31 - 1 testing points per call" % who)
        if self._native is None:
            raise RuntimeError("%s: the handle has been closed" % who)
        rows = []
        for e, (kt, s, sigma2, nugget, meanfunc, mparams) in enumerate(self._hyper):
            mean, var, (it, cv, res), vstats, alpha = self._native.predict_exact(e, kt, s, sigma2, nugget, self._p, self._rtol, self._max_iter,
                                                                                 include_nugget, testing, unc=exact, max_points=int(max_points),
                                                                                 return_alpha=bool(deriv))
            mean += _mean_at(meanfunc, mparams, testing)
            dm = None
            if deriv:
                dm = _mean_inputderiv_at(meanfunc, mparams, testing)
                dm += self._native.kmatvec_inputderiv(kt, s, sigma2, alpha.reshape(-1, 1), testing, max_points=int(max_points))[:, :, 0]
            vr = None
            if bound:
                var, vr, _ = self._native.variance_bound(kt, s, sigma2, nugget, self._p, include_nugget, testing, max_points=int(max_points))
            rows.append((mean, var, cv, res, it, vstats[1] if exact else None, vstats[2] if exact else None, vr, dm))
        kind = "bound" if bound else "exact" if exact else None
        if self._single:
            return IterativePrediction(*rows[0][:8], unc_kind=kind, deriv=rows[0][8])
        cols = list(zip(*rows))
        return IterativePrediction(np.stack(cols[0]), np.stack(cols[1]) if unc else None, np.array(cols[2]), np.array(cols[3]), np.array(cols[4]),
                                   np.stack(cols[5]) if exact else None, np.stack(cols[6]) if exact else None,
                                   np.array(cols[7]) if bound else None, kind, np.stack(cols[8]) if deriv else None)

    # ---- the variance bound -----------------------------------------------------------------------------------------------------------------
    def variance_bound(self, testing, emulator=0, include_nugget=True, rank=None, max_points=0):
        """(m,) max(sigma^2 [+ nugget] - |R^T k*|^2, 0) at ``testing`` (m, D): never below the exact predictive variance of ``emulator``, and
        no solve -- one product of the generated cross covariance with the cache R (built at the first call and kept while the
        hyperparameters and ``precond_rank`` stay; ``variance_cache``).  ``rank`` (default: all of the cache) 1 .. the rank the
        preconditioner reached: the bound of that many leading columns, which is the bound a handle of that ``precond_rank`` gives (to
        rounding); a larger rank never gives a larger value, bit for bit.  A value depends on its query alone, not on ``max_points``
        (queries per device pass, 0: sized by the free device memory) nor on the other queries.  Needs ``precond_rank`` >= 1."""
        who = "IterativeGP.variance_bound"
        r = self._bound_rank(who, rank)
        testing = _points("testing", who, testing, self._D)
        if int(max_points) != max_points or int(max_points) < 0:
            raise ValueError("%s: max_points must not be negative" % who)
        if testing.shape[0] >= 2 ** 31:
            raise ValueError("%s: at most 2^31 - 1 testing points per call" % who)
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        return self._native.variance_bound(kt, s, sigma2, nugget, self._p, include_nugget, testing, var_rank=r, max_points=int(max_points))[0]

    def variance_cache(self, emulator=0):
        """(R (N, var_rank), var_rank) of ``emulator``: R^T A R = I and span R = span of the leading columns of ``preconditioner()[0]``.
        ``var_rank`` lies below the rank the preconditioner reached when the trailing columns of L are linearly dependent to rounding."""
        who = "IterativeGP.variance_cache"
        self._bound_rank(who, None)
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        _, r, R = self._native.variance_bound(kt, s, sigma2, nugget, self._p, True, None, return_cache=True)
        return R, r

    def variance_gap(self, testing, emulator=0):
        """(m,) bound - exact variance at ``testing``, from one exact pass (a solve per query: meant for a few queries), both with the
        nugget: how much the bound gives away here.  Negative entries are rounding, or a variance solve that did not converge."""
        who = "IterativeGP.variance_gap"
        self._bound_rank(who, None)
        testing = _points("testing", who, testing, self._D)
        e, (kt, s, sigma2, nugget, _, _) = self._emulator(who, emulator)
        exact = self._native.predict_exact(e, kt, s, sigma2, nugget, self._p, self._rtol, self._max_iter, True, testing, unc=True)[1]
        return self._native.variance_bound(kt, s, sigma2, nugget, self._p, True, testing)[0] - exact

    def _bound_rank(self, who, rank):
        """the ``var_rank`` request of the native call: 0 for all; every refusal that needs no device"""
        if self._p == 0:
            raise ValueError(_NEEDS_FACTOR % who)
        if rank is None:
            return 0
        r = int(rank)
        if r != rank or r < 1 or r > self._p:
            raise ValueError("%s: rank must be between 1 and precond_rank = %d" % (who, self._p))
        return r
